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
// Launch. The main pass is k_profile's (profile.hip) with two loads per row instead of four and a 19-word record: tiles of one
// span (64 lanes x 16 B) by 32 rows, walked down the rows of a span for X and along the spans of a row block for Y; a lane
// sums in registers while its bin does not change, then ds atomics into a table of 264 bins in LDS, then one global 64-bit
// atomic per word that is not neutral. ONE LAUNCH PER PLANE: a lane holds one record, never ns of them, and the words of a
// call with ns planes are those of ns calls by construction. rho is read once per plane: 16 ns B per fp64 cell.
// The bounds pass is the window walk. The PDF pass is the window walk too: a lane keeps a run (row, count, three limbs) and
// adds it to a table of nbins + 2 rows in LDS when the row changes; the table goes out once, at the end, one global atomic
// per word that is not zero. Equal rows of neighbouring lanes are not combined before the LDS. No scratch, no host
// synchronisation, integer atomics only.
#include "exact_sum.hpp"

#include <cmath>

using namespace armon;

namespace {

using win::kWave;
using win::kWavesPerBlock;
constexpr int kTileRows = 32, kRowsPerWave = kTileRows / kWavesPerBlock;
constexpr int kRec = 19;                    // words of a record that are not reserved
constexpr int kRecWords = 20;               // sizeof(armon_mixing_bin) / 8
constexpr int kTable = 264;                 // bins of the LDS table: X at width 1 needs a span's worth, 128 (fp64) or 256 (fp32)
constexpr int W_N = 0, W_BAD = 1, W_SUM = 2, W_PHI_MIN = 17, W_PHI_MAX = 18;
constexpr int kPdfRowWords = 4;             // count, three limbs
constexpr int kPdfTable = (ARMON_PDF_MAX_BINS + 2) * kPdfRowWords + 1;

using exact::u64;
using exact::u128;
using exact::quantise;
using red::order_key;
using win::bits_of;
using win::finite;
using win::load_cells;
using win::wide;

static_assert(sizeof(armon_mixing_bin) == kRecWords * 8, "armon_mixing_bin is 20 words");
static_assert(sizeof(armon_mixing_spec) == 24 + 20 * ARMON_MAX_SCALARS, "armon_mixing_spec has no padding");
static_assert(sizeof(armon_pdf_spec) == 24, "armon_pdf_spec is 24 bytes");

template <typename T>
struct mix_args {
    const T *rho, *phi;             // one plane per launch
    win::window w;
    int64_t nrb;                    // blocks of kTileRows rows
    int64_t gx0, gy0;               // global position of the window's first cell
    int64_t nbins, width;
    int scale_exp[5];               // the plane's
    u64* bins;                      // the plane's [nbins][kRecWords]
    u64* bounds;                    // the plane's [5] (the bounds pass)
};

struct lane_rec {
    u64 n, n_bad;
    long long sum[5][3];
    u64 phi_min, phi_max;
    __device__ __forceinline__ void reset()
    {
        n = n_bad = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) sum[k][0] = sum[k][1] = sum[k][2] = 0;
        phi_min = ~0ull;
        phi_max = 0;
    }
};

// the five terms of a cell → false when the cell is bad
template <typename T>
__device__ __forceinline__ bool cell_terms(T rho_, T phi_, double t[5])
{
    const double rho = (double)rho_, phi = (double)phi_;
    t[0] = rho; t[1] = phi; t[2] = phi * phi; t[3] = rho * phi; t[4] = t[3] * phi;
    return finite(rho) && finite(phi) && finite(t[2]) && finite(t[3]) && finite(t[4]);
}

template <typename T>
__device__ __forceinline__ void add_cell(const int scale_exp[5], T rho, T phi, lane_rec& acc)
{
    double t[5];
    u128 a[5];
    bool ok = cell_terms<T>(rho, phi, t);
#pragma unroll
    for (int k = 0; k < 5; k++) ok = quantise(t[k], scale_exp[k], a[k]) && ok;
    if (!ok) {
        acc.n_bad += 1;
        return;
    }
    acc.n += 1;
#pragma unroll
    for (int k = 0; k < 5; k++) exact::add_limbs(acc.sum[k], a[k], bits_of(t[k]) >> 63);
    const u64 key = order_key(t[1]);
    acc.phi_min = key < acc.phi_min ? key : acc.phi_min;
    acc.phi_max = key > acc.phi_max ? key : acc.phi_max;
}

__device__ __forceinline__ void merge_min(u64* dst, u64 v)
{
    if (v < __atomic_load_n(dst, __ATOMIC_RELAXED)) atomicMin(dst, v);    // the word only falls: a stale read costs an atomic, no more
}
__device__ __forceinline__ void merge_max(u64* dst, u64 v)
{
    if (v > __atomic_load_n(dst, __ATOMIC_RELAXED)) atomicMax(dst, v);
}

// a lane's record into a record in LDS or in bins_dev
__device__ __forceinline__ void merge_rec(u64* dst, const lane_rec& r)
{
    if (r.n_bad) atomicAdd(dst + W_BAD, r.n_bad);
    if (r.n == 0) return;
    atomicAdd(dst + W_N, r.n);
#pragma unroll
    for (int k = 0; k < 5; k++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (r.sum[k][j]) atomicAdd(dst + W_SUM + 3 * k + j, (u64)r.sum[k][j]);
    merge_min(dst + W_PHI_MIN, r.phi_min);
    merge_max(dst + W_PHI_MAX, r.phi_max);
}

template <typename T, bool WIDE, int AXIS>
__global__ void __launch_bounds__(kBlock, 2)
k_mixing(mix_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 table[kTable * kRec];
    __shared__ int table_hi;                                        // the last record of the table written since it last went out
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    for (int i = tid; i < kTable * kRec; i += kBlock) table[i] = i % kRec == W_PHI_MIN ? ~0ull : 0ull;
    if (tid == 0) table_hi = -1;
    int64_t table_base = -1;                                        // workgroup-uniform
    const auto table_out = [&]() {                                  // (between two barriers)
        const int used = (table_hi + 1) * kRec;
        __syncthreads();
        if (tid == 0) table_hi = -1;
        for (int i = tid; i < used; i += kBlock) {
            const int word = i % kRec;
            const u64 v = table[i], neutral = word == W_PHI_MIN ? ~0ull : 0ull;
            if (v == neutral) continue;
            u64* dst = a.bins + (table_base + i / kRec) * kRecWords + word;     // only bins < nbins were ever written
            if (word == W_PHI_MIN) merge_min(dst, v);
            else if (word == W_PHI_MAX) merge_max(dst, v);
            else atomicAdd(dst, v);
            table[i] = neutral;
        }
    };
    lane_rec acc;
    acc.reset();
    int64_t cur = -1;                                               // the bin `acc` belongs to
    const auto lane_out = [&]() {
        if (cur < 0) return;
        const int64_t at = cur - table_base;
        if (at >= 0 && at < kTable) {
            merge_rec(table + at * kRec, acc);
            if ((int)at > __atomic_load_n(&table_hi, __ATOMIC_RELAXED)) atomicMax(&table_hi, (int)at);
        } else {
            merge_rec(a.bins + cur * kRecWords, acc);
        }
        acc.reset();
        cur = -1;
    };
    __syncthreads();
    const int64_t ntiles = a.w.nspan * a.nrb, per = (ntiles + gridDim.x - 1) / gridDim.x;
    const int64_t t0 = (int64_t)blockIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    const T* __restrict__ rho = a.rho + a.w.first;
    const T* __restrict__ phi = a.phi + a.w.first;
    for (int64_t tile = t0; tile < t1; tile++) {
        const int64_t sp = AXIS == ARMON_PROFILE_Y ? tile % a.w.nspan : tile / a.nrb;
        const int64_t rb = AXIS == ARMON_PROFILE_Y ? tile / a.w.nspan : tile % a.nrb;
        const int64_t xa = sp * kWave * V;
        const int64_t ya = rb * kTileRows, yb = ya + kTileRows < a.w.wny ? ya + kTileRows : a.w.wny;
        const int64_t base = AXIS == ARMON_PROFILE_X ? (a.gx0 + xa) / a.width : (a.gy0 + ya) / a.width;   // the smallest bin of the tile
        if (base != table_base) {
            lane_out();
            __syncthreads();
            table_out();
            __syncthreads();
            table_base = base;
        }
        const auto [x, left] = win::lane_column<V>(a.w, sp, lane);
        if (left <= 0) continue;                                    // (no barrier below this line of the loop body)
        for (int i = 0; i < kRowsPerWave; i++) {
            const int64_t r = ya + (int64_t)w * kRowsPerWave + i;
            if (r >= yb) break;
            T fr[V], fp[V];                                         // both loads are issued before the first arithmetic
            const int64_t at = r * a.w.pitch + x;
            load_cells<T, WIDE>(rho + at, left >= V, left, fr);
            load_cells<T, WIDE>(phi + at, left >= V, left, fp);
#pragma unroll
            for (int c = 0; c < V; c++) {
                if (c >= left) break;
                const int64_t b = (AXIS == ARMON_PROFILE_X ? a.gx0 + x + c : a.gy0 + r) / a.width;
                if (b >= a.nbins) continue;
                if (b != cur) {
                    lane_out();
                    cur = b;
                }
                add_cell<T>(a.scale_exp, fr[c], fp[c], acc);
            }
        }
    }
    lane_out();
    __syncthreads();
    table_out();
}

// the bounds pass: the bit pattern of the largest finite |t_j| of the window, merged by unsigned maximum
template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock, 4)
k_mixing_bounds(mix_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 lds[kWavesPerBlock];
    const int tid = (int)threadIdx.x;
    const T* __restrict__ rho = a.rho + a.w.first;
    const T* __restrict__ phi = a.phi + a.w.first;
    u64 top[5] = {0, 0, 0, 0, 0};
    win::walk<V>(a.w, [&](int64_t r, int64_t x, int64_t left) {
        if (left <= 0) return;
        T fr[V], fp[V];
        const int64_t at = r * a.w.pitch + x;
        load_cells<T, WIDE>(rho + at, left >= V, left, fr);
        load_cells<T, WIDE>(phi + at, left >= V, left, fp);
#pragma unroll
        for (int c = 0; c < V; c++) {
            if (c >= left) break;
            double t[5];
            (void)cell_terms<T>(fr[c], fp[c], t);                   // every cell of the window counts, binned or not
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const u64 m = bits_of(fabs(t[k]));
                if (finite(t[k]) && m > top[k]) top[k] = m;
            }
        }
    });
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const u64 m = red::block_reduce<red::op_umax, kWavesPerBlock>(top[k], lds, tid);
        if (tid == 0 && m) merge_max(a.bounds + k, m);
    }
}

__global__ void k_mixing_reset(int64_t words, u64* __restrict__ bins)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) bins[i] = i % kRecWords == W_PHI_MIN ? ~0ull : 0ull;
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

__global__ void k_zero_words(int64_t words, u64* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) out[i] = 0;
}

// the grid = what is resident at once of the kernel launched, at most `work` workgroups and at most the profile kernels' cap
template <typename K>
int resident_blocks(armon_ctx* ctx, K kernel, int64_t work, int64_t& blocks)
{
    int per_cu = 0;
    ARMON_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0));
    blocks = (int64_t)ctx->n_cu * (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));
    if (ctx->tune_profile_wgs > 0 && blocks > ctx->tune_profile_wgs) blocks = ctx->tune_profile_wgs;     // PROFILE_WGS: no result bit changes
    if (blocks > work) blocks = work;
    return ARMON_OK;
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
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
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
    a.rho = rho;
    a.nrb = (wny + kTileRows - 1) / kTileRows;
    a.gx0 = global_col0; a.gy0 = global_row0;
    a.nbins = s.nbins; a.width = s.width;
    uintptr_t mis = (uintptr_t)rho;
    for (int k = 0; k < ns; k++) mis |= (uintptr_t)phi[k];          // one alignment path for the whole call
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n);
    // the bounds pass: a wave per (row, span) item; the main pass: a workgroup per tile
    const int64_t work = BOUNDS ? (a.w.wny * a.w.nspan + kWavesPerBlock - 1) / kWavesPerBlock : a.w.nspan * a.nrb;
    int64_t blocks = 0;
#define ARMON_MIXING_GRID(KERNEL)                                                       \
    do {                                                                                \
        rc = resident_blocks(ctx, KERNEL, work, blocks);                                \
        if (rc != ARMON_OK) return rc;                                                  \
    } while (0)
    for (int k = 0; k < ns; k++) {
        a.phi = phi[k];
        for (int j = 0; j < 5; j++) a.scale_exp[j] = s.scale_exp[k][j];
        a.bins = BOUNDS ? nullptr : static_cast<u64*>(out_dev) + (int64_t)k * s.nbins * kRecWords;
        a.bounds = BOUNDS ? static_cast<u64*>(out_dev) + 5 * k : nullptr;
        if (BOUNDS) {
            if (wide_ok) {
                ARMON_MIXING_GRID((k_mixing_bounds<T, true>));
                hipLaunchKernelGGL((k_mixing_bounds<T, true>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
            } else {
                ARMON_MIXING_GRID((k_mixing_bounds<T, false>));
                hipLaunchKernelGGL((k_mixing_bounds<T, false>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
            }
        } else if (s.axis == ARMON_PROFILE_X) {
            if (wide_ok) {
                ARMON_MIXING_GRID((k_mixing<T, true, ARMON_PROFILE_X>));
                hipLaunchKernelGGL((k_mixing<T, true, ARMON_PROFILE_X>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
            } else {
                ARMON_MIXING_GRID((k_mixing<T, false, ARMON_PROFILE_X>));
                hipLaunchKernelGGL((k_mixing<T, false, ARMON_PROFILE_X>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
            }
        } else {
            if (wide_ok) {
                ARMON_MIXING_GRID((k_mixing<T, true, ARMON_PROFILE_Y>));
                hipLaunchKernelGGL((k_mixing<T, true, ARMON_PROFILE_Y>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
            } else {
                ARMON_MIXING_GRID((k_mixing<T, false, ARMON_PROFILE_Y>));
                hipLaunchKernelGGL((k_mixing<T, false, ARMON_PROFILE_Y>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
            }
        }
        rc = check_launch(BOUNDS ? "mixing_bounds" : "mixing");
        if (rc != ARMON_OK) return rc;
    }
#undef ARMON_MIXING_GRID
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
    const int64_t work = (a.w.wny * a.w.nspan + kWavesPerBlock - 1) / kWavesPerBlock;
    int64_t blocks = 0;
    if (wide_ok) {
        rc = resident_blocks(ctx, k_scalar_pdf<T, true>, work, blocks);
        if (rc != ARMON_OK) return rc;
        hipLaunchKernelGGL((k_scalar_pdf<T, true>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
    } else {
        rc = resident_blocks(ctx, k_scalar_pdf<T, false>, work, blocks);
        if (rc != ARMON_OK) return rc;
        hipLaunchKernelGGL((k_scalar_pdf<T, false>), dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
    }
    return check_launch("scalar_pdf");
}

}  // namespace

extern "C" {

int armon_hip_mixing_reset(armon_ctx* ctx, int ns, int64_t nbins, armon_mixing_bin* bins_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(ns >= 1 && ns <= ARMON_MAX_SCALARS && nbins >= 1 && nbins < (1ll << 48) && bins_dev,
                  "mixing_reset: ns = %d, nbins = %lld, bins_dev = %p", ns, (long long)nbins, (void*)bins_dev);
    const int64_t words = (int64_t)ns * nbins * kRecWords;
    hipLaunchKernelGGL(k_mixing_reset, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, words,
                       reinterpret_cast<u64*>(bins_dev));
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
    hipLaunchKernelGGL(k_zero_words, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, words,
                       reinterpret_cast<u64*>(out_dev));
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
