// mixing.hip — mixing measures of the passive scalars on the device: per scalar plane the real cells of a window
// binned along x or y and reduced to one 160-byte record per (plane, bin) (armon_mixing_bin, include/armon_hip.h), and the
// histogram of one plane with the exact mass of every bin (armon_hip_scalar_pdf). Nothing is moved: rho and the plane are read,
// only the records are written.
//
// No reference counterpart: the reference carries no scalars and writes whole fields (ref src/io.jl:37-81).
//
// PER CELL at the global position (gx, gy) and per plane k, all arithmetic in fp64 (fp32 values converted first), one IEEE
// operation per operation written:
//     bin     X: gx / width       Y: gy / width       a cell with b >= nbins is skipped and counted nowhere
//     terms   t0 = rho, t1 = phi, t2 = phi phi, t3 = rho phi, t4 = t3 phi
//     Q_j     = round-half-even(t_j / 2^s_kj), an exact integer; the cell is BAD for plane k when rho, phi or a term is not
//             finite or a |Q_j| >= 2^95: it adds 1 to that plane's n_bad and nothing else
//     limbs   exact::quantise / exact::add_limbs, as in profile.hip; phi enters phi_min / phi_max through its order key
// PDF, per cell: bad when rho or phi is not finite or |Q(rho)| >= 2^95; else "below" when phi < lo; else
//     fb = floor((phi - lo) inv_w), "above" when !(fb < nbins), else bin (int64)fb; the row takes 1 and the limbs of Q(rho).
//
// MERGE: every word merges by integer addition, unsigned minimum or unsigned maximum, so a record is a function of the
// planes, the spec and the scale only, WORD FOR WORD (profile.hip says why the limbs are kept apart from the first cell on).
//
// Launch: binned.hpp states the main pass, the bounds pass and the grid; here two loads per row and a record with one (min, max)
// pair, phi: 19 words of 20. The tiles go down the rows of a span for X and along the spans of a row block for Y. ONE LAUNCH
// PER PLANE: a lane holds one record, never ns of them, and the words of a call with ns planes are those of ns calls by
// construction. rho is read once per plane: 16 ns B per fp64 cell.
// The PDF pass is the window walk: a lane keeps a run (row, count, three limbs) and adds it to a table of nbins + 2 rows in
// LDS when the row changes; the table goes out once, at the end, one global atomic per word that is not zero. Equal rows of
// neighbouring lanes are not combined before the LDS. No scratch, no host synchronisation, integer atomics only.
#include "binned.hpp"

#include <cmath>

using namespace armon;

namespace {

using binned::kTileRows;
using binned::lane_rec;
using exact::u64;
using exact::u128;
using exact::quantise;
using red::order_key;
using win::bits_of;
using win::finite;
using win::load_cells;
using win::wide;
constexpr int kPairs = 1, kRecWords = 20;   // phi; sizeof(armon_mixing_bin) / 8
constexpr int kPdfRowWords = 4;             // count, three limbs
constexpr int kPdfTable = (ARMON_PDF_MAX_BINS + 2) * kPdfRowWords + 1;

static_assert(sizeof(armon_mixing_bin) == kRecWords * 8, "armon_mixing_bin is 20 words");
static_assert(binned::layout<kPairs>::used == 19, "phi_min, phi_max are words 17 and 18");
static_assert(sizeof(armon_mixing_spec) == 24 + 20 * ARMON_MAX_SCALARS, "armon_mixing_spec has no padding");
static_assert(sizeof(armon_pdf_spec) == 24, "armon_pdf_spec is 24 bytes");

template <typename T>
struct mix_args {
    binned::pass_args<T, 2> p;      // rho and ONE plane per launch
    int64_t nbins, width;
    int scale_exp[5];               // the plane's
};

// what binned.hpp asks of a measure
template <typename T, int AXIS>
struct measure {
    static constexpr int NF = 2, NX = kPairs, kRecWords = ::kRecWords;
    static constexpr bool kAlongRows = AXIS == ARMON_PROFILE_Y;
    struct place {};
    const mix_args<T>& a;
    __device__ __forceinline__ int64_t tile_base(int64_t gxa, int64_t, int64_t gya, int64_t) const
    {
        return (AXIS == ARMON_PROFILE_X ? gxa : gya) / a.width;     // the smallest bin of the tile
    }
    __device__ __forceinline__ int64_t bin(int64_t gx, int64_t gy, place&) const
    {
        const int64_t b = (AXIS == ARMON_PROFILE_X ? gx : gy) / a.width;
        return b < a.nbins ? b : -1;
    }
    // the five terms of a cell → false when the cell is bad
    __device__ __forceinline__ bool terms(const T c[2], const place&, double t[5]) const
    {
        const double rho = (double)c[0], phi = (double)c[1];
        t[0] = rho; t[1] = phi; t[2] = phi * phi; t[3] = rho * phi; t[4] = t[3] * phi;
        return finite(rho) && finite(phi) && finite(t[2]) && finite(t[3]) && finite(t[4]);
    }
    __device__ __forceinline__ void add(const T c[2], const place& pl, lane_rec<kPairs>& acc) const
    {
        double t[5];
        const bool ok = terms(c, pl, t);
        if (binned::add_terms(t, ok, a.scale_exp, 5, acc)) acc.take(0, order_key(t[1]));
    }
};

template <typename T, bool WIDE, int AXIS>
__global__ void __launch_bounds__(kBlock, 2)
k_mixing(mix_args<T> a)
{
    binned::main_pass<measure<T, AXIS>, T, WIDE>(measure<T, AXIS>{a}, a.p);
}

template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock, 4)
k_mixing_bounds(mix_args<T> a)
{
    binned::bounds_pass<measure<T, ARMON_PROFILE_X>, T, WIDE>(measure<T, ARMON_PROFILE_X>{a}, a.p);
}

template <typename T>
struct pdf_args {
    const T *rho, *phi;
    win::window w;
    armon_pdf_spec s;
    u64* out;                       // [(nbins + 2) * 4 + 1]
};

template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock, 4)
k_scalar_pdf(pdf_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 table[kPdfTable];
    const int tid = (int)threadIdx.x;
    const int nbins = a.s.nbins, words = (nbins + 2) * kPdfRowWords + 1;
    for (int i = tid; i < words; i += kBlock) table[i] = 0;
    __syncthreads();
    const T* __restrict__ rho = a.rho + a.w.first;
    const T* __restrict__ phi = a.phi + a.w.first;
    const double lo = a.s.lo, inv_w = a.s.inv_w, top = (double)nbins;
    int cur = -1;                                                   // the row of the lane's run
    u64 count = 0, bad = 0;
    long long mass[3] = {0, 0, 0};
    const auto run_out = [&]() {
        if (cur < 0) return;
        u64* dst = table + cur * kPdfRowWords;
        atomicAdd(dst, count);
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (mass[j]) atomicAdd(dst + 1 + j, (u64)mass[j]);
        count = 0;
        mass[0] = mass[1] = mass[2] = 0;
        cur = -1;
    };
    win::walk<V>(a.w, [&](int64_t r, int64_t x, int64_t left) {
        if (left <= 0) return;
        T fr[V], fp[V];
        const int64_t at = r * a.w.pitch + x;
        load_cells<T, WIDE>(rho + at, left >= V, left, fr);
        load_cells<T, WIDE>(phi + at, left >= V, left, fp);
#pragma unroll
        for (int c = 0; c < V; c++) {
            if (c >= left) break;
            const double d = (double)fr[c], f = (double)fp[c];
            u128 q;
            if (!quantise(d, a.s.rho_scale_exp, q) || !finite(f)) {     // (quantise refuses a rho that is not finite)
                bad += 1;
                continue;
            }
            int row;
            if (f < lo) row = nbins;
            else {
                const double fb = floor((f - lo) * inv_w);
                row = !(fb < top) ? nbins + 1 : (int)(int64_t)fb;
            }
            if (row != cur) {
                run_out();
                cur = row;
            }
            count += 1;
            exact::add_limbs(mass, q, bits_of(d) >> 63);
        }
    });
    run_out();
    if (bad) atomicAdd(table + words - 1, bad);
    __syncthreads();
    for (int i = tid; i < words; i += kBlock) {
        const u64 v = table[i];
        if (v) atomicAdd(a.out + i, v);
    }
}

template <typename T, bool BOUNDS, bool WIDE>
int launch_axis(armon_ctx* ctx, int axis, int64_t work, const mix_args<T>& a)
{
    if (BOUNDS) return binned::launch_resident(ctx, k_mixing_bounds<T, WIDE>, work, a);
    return axis == ARMON_PROFILE_X ? binned::launch_resident(ctx, k_mixing<T, WIDE, ARMON_PROFILE_X>, work, a)
                                   : binned::launch_resident(ctx, k_mixing<T, WIDE, ARMON_PROFILE_Y>, work, a);
}

template <typename T, bool BOUNDS>
int mixing_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const T* rho, int ns, const T* const* phi,
                int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0,
                const armon_mixing_spec* spec, void* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(rho && phi && spec && out_dev, "NULL argument");
    ARMON_REQUIRE(ns >= 1 && ns <= ARMON_MAX_SCALARS, "mixing: ns = %d leaves 1..%d", ns, ARMON_MAX_SCALARS);
    for (int k = 0; k < ns; k++) ARMON_REQUIRE(phi[k] != nullptr, "mixing: phi[%d] is NULL", k);
    mix_args<T> a;
    binned::pass_args<T, 2>& p = a.p;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, p.w);
    if (rc == ARMON_OK) rc = win::check_global_cell(global_col0, global_row0);
    if (rc != ARMON_OK) return rc;
    const armon_mixing_spec& s = *spec;
    ARMON_REQUIRE(s.axis == ARMON_PROFILE_X || s.axis == ARMON_PROFILE_Y, "mixing: unknown axis %d", s.axis);
    ARMON_REQUIRE(s.nbins >= 1 && s.nbins < (1ll << 48), "mixing: nbins = %lld", (long long)s.nbins);
    ARMON_REQUIRE(s.width >= 1, "mixing: width = %lld", (long long)s.width);
    for (int k = 0; k < ns; k++)
        for (int j = 0; j < 5; j++)
            ARMON_REQUIRE(s.scale_exp[k][j] >= -4096 && s.scale_exp[k][j] <= 4096, "mixing: scale_exp[%d][%d] = %d leaves [-4096, 4096]", k, j,
                          s.scale_exp[k][j]);
    p.f[0] = rho;
    p.nrb = (wny + kTileRows - 1) / kTileRows;
    p.gx0 = global_col0; p.gy0 = global_row0;
    a.nbins = s.nbins; a.width = s.width;
    uintptr_t mis = (uintptr_t)rho;
    for (int k = 0; k < ns; k++) mis |= (uintptr_t)phi[k];          // one alignment path for the whole call
    const bool wide_ok = win::rows_are_16B(p.w, mis, wide<T>::n);
    const int64_t work = binned::pass_work(p.w, p.nrb, BOUNDS);
    for (int k = 0; k < ns; k++) {
        p.f[1] = phi[k];
        for (int j = 0; j < 5; j++) a.scale_exp[j] = s.scale_exp[k][j];
        p.bins = BOUNDS ? nullptr : static_cast<u64*>(out_dev) + (int64_t)k * s.nbins * kRecWords;
        p.bounds = BOUNDS ? static_cast<u64*>(out_dev) + 5 * k : nullptr;
        rc = wide_ok ? launch_axis<T, BOUNDS, true>(ctx, s.axis, work, a) : launch_axis<T, BOUNDS, false>(ctx, s.axis, work, a);
        if (rc == ARMON_OK) rc = check_launch(BOUNDS ? "mixing_bounds" : "mixing");
        if (rc != ARMON_OK) return rc;
    }
    return ARMON_OK;
}

template <typename T>
int pdf_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const T* rho, const T* phi, int64_t col0,
             int64_t row0, int64_t wnx, int64_t wny, const armon_pdf_spec* spec, uint64_t* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(rho && phi && spec && out_dev, "NULL argument");
    pdf_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
    if (rc != ARMON_OK) return rc;
    const armon_pdf_spec& s = *spec;
    ARMON_REQUIRE(s.nbins >= 1 && s.nbins <= ARMON_PDF_MAX_BINS, "scalar_pdf: nbins = %d leaves 1..%d", s.nbins, ARMON_PDF_MAX_BINS);
    ARMON_REQUIRE(std::isfinite(s.lo) && std::isfinite(s.inv_w) && s.inv_w > 0, "scalar_pdf: lo = %g must be finite, 1/w = %g finite and > 0",
                  s.lo, s.inv_w);
    ARMON_REQUIRE(s.rho_scale_exp >= -4096 && s.rho_scale_exp <= 4096, "scalar_pdf: rho_scale_exp = %d leaves [-4096, 4096]", s.rho_scale_exp);
    a.rho = rho; a.phi = phi;
    a.s = s;
    a.out = reinterpret_cast<u64*>(out_dev);
    const bool wide_ok = win::rows_are_16B(a.w, (uintptr_t)rho | (uintptr_t)phi, wide<T>::n);
    const int64_t work = binned::pass_work(a.w, 0, true);           // a walk, as the bounds passes
    rc = wide_ok ? binned::launch_resident(ctx, k_scalar_pdf<T, true>, work, a) : binned::launch_resident(ctx, k_scalar_pdf<T, false>, work, a);
    return rc == ARMON_OK ? check_launch("scalar_pdf") : rc;
}

}  // namespace

extern "C" {

int armon_hip_mixing_reset(armon_ctx* ctx, int ns, int64_t nbins, armon_mixing_bin* bins_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(ns >= 1 && ns <= ARMON_MAX_SCALARS && nbins >= 1 && nbins < (1ll << 48) && bins_dev,
                  "mixing_reset: ns = %d, nbins = %lld, bins_dev = %p", ns, (long long)nbins, (void*)bins_dev);
    const int64_t words = (int64_t)ns * nbins * kRecWords;
    binned::launch_reset<kPairs, kRecWords>(ctx, words, bins_dev);
    return check_launch("mixing_reset");
}

int armon_hip_mixing(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, int ns,
                     const double* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                     int64_t global_row0, const armon_mixing_spec* spec, armon_mixing_bin* bins_dev)
{
    return mixing_impl<double, false>(ctx, row_length, nghost, nx, ny, rho, ns, phi, col0, row0, wnx, wny, global_col0, global_row0, spec, bins_dev);
}

int armon_hip_mixing_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, int ns,
                         const float* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                         int64_t global_row0, const armon_mixing_spec* spec, armon_mixing_bin* bins_dev)
{
    return mixing_impl<float, false>(ctx, row_length, nghost, nx, ny, rho, ns, phi, col0, row0, wnx, wny, global_col0, global_row0, spec, bins_dev);
}

int armon_hip_mixing_bounds(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, int ns,
                            const double* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                            int64_t global_row0, const armon_mixing_spec* spec, uint64_t* bounds_dev)
{
    return mixing_impl<double, true>(ctx, row_length, nghost, nx, ny, rho, ns, phi, col0, row0, wnx, wny, global_col0, global_row0, spec, bounds_dev);
}

int armon_hip_mixing_bounds_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, int ns,
                                const float* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                                int64_t global_row0, const armon_mixing_spec* spec, uint64_t* bounds_dev)
{
    return mixing_impl<float, true>(ctx, row_length, nghost, nx, ny, rho, ns, phi, col0, row0, wnx, wny, global_col0, global_row0, spec, bounds_dev);
}

int armon_hip_scalar_pdf_reset(armon_ctx* ctx, int nbins, uint64_t* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nbins >= 1 && nbins <= ARMON_PDF_MAX_BINS && out_dev, "scalar_pdf_reset: nbins = %d, out_dev = %p", nbins, (void*)out_dev);
    const int64_t words = (int64_t)(nbins + 2) * kPdfRowWords + 1;
    binned::launch_reset<0, 1>(ctx, words, out_dev);                // (no pairs: every word is neutral at 0)
    return check_launch("scalar_pdf_reset");
}

int armon_hip_scalar_pdf(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, const double* phi,
                         int64_t col0, int64_t row0, int64_t wnx, int64_t wny, const armon_pdf_spec* spec, uint64_t* out_dev)
{
    return pdf_impl<double>(ctx, row_length, nghost, nx, ny, rho, phi, col0, row0, wnx, wny, spec, out_dev);
}

int armon_hip_scalar_pdf_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, const float* phi,
                             int64_t col0, int64_t row0, int64_t wnx, int64_t wny, const armon_pdf_spec* spec, uint64_t* out_dev)
{
    return pdf_impl<float>(ctx, row_length, nghost, nx, ny, rho, phi, col0, row0, wnx, wny, spec, out_dev);
}

}  // extern "C"
