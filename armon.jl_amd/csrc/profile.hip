// profile.hip — 1-D profiles of a 2-D state on the device: the real cells of a window, binned along x, along y or by the
// distance from a centre, and reduced to one 192-byte record per bin (armon_profile_bin, include/armon_hip.h). Nothing is
// moved: rho, u, v, E are read once (32 B per fp64 cell), only the records are written.
//
// No reference counterpart: the reference writes whole fields (ref src/io.jl:37-81) and leaves profiles to a plot script.
//
// PER CELL at the global position (gx, gy), all arithmetic in fp64 (fp32 values converted first), one IEEE operation per
// operation written, IEEE division and square root:
//     bin     X: gx / width       Y: gy / width
//             R: rx = ((double)gx + 0.5 - cx) dx, ry likewise, rr = sqrt(rx rx + ry ry), b = floor(rr inv_dr)
//             a cell with b >= nbins is skipped and counted nowhere
//     un, ut  X: u, v             Y: v, u        R: (u rx + v ry) / rr, (v rx - u ry) / rr, both 0 where rr == 0
//     terms   rho, rho un, rho ut, rho E, p — p = the EOS of the cell's (rho, E, u, v) evaluated IN THE DATA TYPE by
//             phys::perfect_gas / phys::bizarrium (the sound speed is dead code here), then converted; eos = -1: no p
//     Q_k     = round-half-even(t_k / 2^s_k), an exact integer; the cell is BAD when rho, u, v, E or a term is not finite or a
//             |Q_k| >= 2^95: it adds 1 to n_bad and nothing else
//     limbs   a = |Q_k| -> a & 0xffffffff, (a >> 32) & 0xffffffff, a >> 64, each negated when Q_k < 0, each added to its own
//             int64; rho and p also enter a minimum and a maximum through the order key bits ^ (sign ? ~0 : 1 << 63)
//
// MERGE: every word of a record merges by integer addition, unsigned minimum or unsigned maximum — associative and
// commutative, so the record is a function of the state, the spec and the scale only: not of the launch shape, the window
// split, the alignment path, the ghost width or the decomposition, and it is so WORD FOR WORD. That is why a lane keeps
// the three limb sums of a term apart from the first cell on instead of one 128-bit sum split at the end: the split of a
// sum of Q's is not the sum of the splits (2^32 and -1 give the limbs (-1, 1, 0), their sum gives (0xffffffff, 0, 0)), so
// limbs cut from partial sums would depend on which cells a lane happened to see. Same value, other words.
//
// Launch: binned.hpp states the main pass, the bounds pass and the grid. The record has two (min, max) pairs, rho and p: 21 words
// of 24. The tiles go down the rows of one span for X and R, along the spans of one row block for Y; the table's first bin
// changes once per span for X, once per row block for Y, once per tile for R.
#include "binned.hpp"

#include <cmath>

using namespace armon;

namespace {

using binned::kTileRows;
using binned::lane_rec;
using exact::u64;
using red::order_key;
using win::finite;
using win::wide;
constexpr int kPairs = 2, kRecWords = 24;   // rho and p; sizeof(armon_profile_bin) / 8

static_assert(sizeof(armon_profile_bin) == kRecWords * 8, "armon_profile_bin is 24 words");
static_assert(binned::layout<kPairs>::used == 21, "rho_min, rho_max, p_min, p_max are words 17 to 20");

template <typename T>
struct prof_args {
    binned::pass_args<T, 4> p;      // rho, u, v, E
    armon_profile_spec s;
};

// what the bin of a cell leaves for its terms: the radius, or nothing
struct no_place {};
struct r_place { double rx, ry, rr; };
template <int KIND> struct place_of { typedef no_place type; };
template <> struct place_of<ARMON_PROFILE_R> { typedef r_place type; };

__device__ __forceinline__ void normal_tangent(const no_place&, double, double, double&, double&) {}
__device__ __forceinline__ void normal_tangent(const r_place& pl, double u, double v, double& un, double& ut)
{
    if (pl.rr == 0.) { un = 0.; ut = 0.; }
    else { un = (u * pl.rx + v * pl.ry) / pl.rr; ut = (v * pl.rx - u * pl.ry) / pl.rr; }
}

// the five terms of a cell → false when the cell is bad
template <typename T, int KIND>
__device__ __forceinline__ bool cell_terms(const armon_profile_spec& s, T rho_, T u_, T v_, T E_, const typename place_of<KIND>::type& pl,
                                           double t[5])
{
    const double rho = (double)rho_, u = (double)u_, v = (double)v_, E = (double)E_;
    double un = u, ut = v;
    if (KIND == ARMON_PROFILE_Y) { un = v; ut = u; }
    normal_tangent(pl, u, v, un, ut);
    t[0] = rho; t[1] = rho * un; t[2] = rho * ut; t[3] = rho * E; t[4] = 0.;
    if (s.eos >= 0) {
        T p, c, g;
        if (s.eos == ARMON_EOS_PERFECT_GAS) phys::perfect_gas<T>((T)s.gamma, rho_, E_, u_, v_, p, c);
        else phys::bizarrium<false, T>(rho_, E_, u_, v_, p, c, g);
        t[4] = (double)p;
    }
    return finite(rho) && finite(u) && finite(v) && finite(E) && finite(t[1]) && finite(t[2]) && finite(t[3]) && finite(t[4]);
}

// the bin of a cell, < 0 = skipped; R also leaves rx, ry, rr
template <int KIND>
__device__ __forceinline__ int64_t cell_bin(const armon_profile_spec& s, int64_t gx, int64_t gy, no_place&)
{
    const int64_t b = (KIND == ARMON_PROFILE_X ? gx : gy) / s.width;
    return b < s.nbins ? b : -1;
}
template <int KIND>
__device__ __forceinline__ int64_t cell_bin(const armon_profile_spec& s, int64_t gx, int64_t gy, r_place& pl)
{
    pl.rx = ((double)gx + 0.5 - s.cx) * s.dx;
    pl.ry = ((double)gy + 0.5 - s.cy) * s.dy;
    pl.rr = sqrt(pl.rx * pl.rx + pl.ry * pl.ry);
    const double fb = floor(pl.rr * s.inv_dr);
    if (!(fb < (double)s.nbins)) return -1;                         // (a NaN is skipped too)
    const int64_t b = (int64_t)fb;
    return b < s.nbins ? b : -1;
}

// the smallest bin a tile can touch (a lower bound is enough: it only decides what goes through the LDS table)
template <int KIND>
__device__ __forceinline__ int64_t tile_base_of(const armon_profile_spec& s, int64_t gxa, int64_t gxb, int64_t gya, int64_t gyb)
{
    if (KIND == ARMON_PROFILE_X) return gxa / s.width;
    if (KIND == ARMON_PROFILE_Y) return gya / s.width;
    const double xa = (double)gxa + 0.5 - s.cx, xb = (double)gxb + 0.5 - s.cx, ya = (double)gya + 0.5 - s.cy, yb = (double)gyb + 0.5 - s.cy;
    const double ddx = (xa > 0. ? xa : (xb < 0. ? -xb : 0.)) * s.dx, ddy = (ya > 0. ? ya : (yb < 0. ? -yb : 0.)) * s.dy;
    const double fb = floor(sqrt(ddx * ddx + ddy * ddy) * s.inv_dr) - 1.;
    return fb > 0. ? (fb < 4e18 ? (int64_t)fb : (int64_t)4e18) : 0;
}

// what binned.hpp asks of a measure
template <typename T, int KIND>
struct measure {
    static constexpr int NF = 4, NX = kPairs, kRecWords = ::kRecWords;
    static constexpr bool kAlongRows = KIND == ARMON_PROFILE_Y;
    typedef typename place_of<KIND>::type place;
    const armon_profile_spec& s;
    __device__ __forceinline__ int64_t tile_base(int64_t gxa, int64_t gxb, int64_t gya, int64_t gyb) const
    {
        return tile_base_of<KIND>(s, gxa, gxb, gya, gyb);
    }
    __device__ __forceinline__ int64_t bin(int64_t gx, int64_t gy, place& pl) const { return cell_bin<KIND>(s, gx, gy, pl); }
    __device__ __forceinline__ bool terms(const T c[4], const place& pl, double t[5]) const
    {
        return cell_terms<T, KIND>(s, c[0], c[1], c[2], c[3], pl, t);
    }
    __device__ __forceinline__ void add(const T c[4], const place& pl, lane_rec<kPairs>& acc) const
    {
        double t[5];
        const bool ok = terms(c, pl, t);
        if (!binned::add_terms(t, ok, s.scale_exp, s.eos >= 0 ? 5 : 4, acc)) return;
        acc.take(0, order_key(t[0]));
        if (s.eos >= 0) acc.take(1, order_key(t[4]));
    }
};

template <typename T, bool WIDE, int KIND>
__global__ void __launch_bounds__(kBlock, 2)       // 148 to 187 VGPRs: capped lower, the 21-word record spills
k_profile(prof_args<T> a)
{
    binned::main_pass<measure<T, KIND>, T, WIDE>(measure<T, KIND>{a.s}, a.p);
}

template <typename T, bool WIDE, int KIND>
__global__ void __launch_bounds__(kBlock, 4)
k_profile_bounds(prof_args<T> a)
{
    binned::bounds_pass<measure<T, KIND>, T, WIDE>(measure<T, KIND>{a.s}, a.p);
}

template <typename T, bool BOUNDS, int KIND>
int launch_kind(armon_ctx* ctx, bool wide_ok, int64_t work, const prof_args<T>& a)
{
    using binned::launch_resident;
    if (BOUNDS)
        return wide_ok ? launch_resident(ctx, k_profile_bounds<T, true, KIND>, work, a) : launch_resident(ctx, k_profile_bounds<T, false, KIND>, work, a);
    return wide_ok ? launch_resident(ctx, k_profile<T, true, KIND>, work, a) : launch_resident(ctx, k_profile<T, false, KIND>, work, a);
}

template <typename T, bool BOUNDS>
int profile_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const T* rho, const T* u, const T* v, const T* E,
                 int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0,
                 const armon_profile_spec* spec, void* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(rho && u && v && E && spec && out_dev, "NULL argument");
    prof_args<T> a;
    binned::pass_args<T, 4>& p = a.p;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, p.w);
    if (rc == ARMON_OK) rc = win::check_global_cell(global_col0, global_row0);
    if (rc != ARMON_OK) return rc;
    const armon_profile_spec& s = *spec;
    ARMON_REQUIRE(s.kind == ARMON_PROFILE_X || s.kind == ARMON_PROFILE_Y || s.kind == ARMON_PROFILE_R, "unknown profile kind %d", s.kind);
    ARMON_REQUIRE(s.eos == -1 || s.eos == ARMON_EOS_PERFECT_GAS || s.eos == ARMON_EOS_BIZARRIUM, "unknown eos %d", s.eos);
    ARMON_REQUIRE(s.nbins >= 1 && s.nbins < (1ll << 48), "profile: nbins = %lld", (long long)s.nbins);
    ARMON_REQUIRE(s.width >= 1, "profile: width = %lld", (long long)s.width);
    if (s.kind == ARMON_PROFILE_R)
        ARMON_REQUIRE(std::isfinite(s.dx) && std::isfinite(s.dy) && std::isfinite(s.inv_dr) && s.dx > 0 && s.dy > 0 && s.inv_dr > 0 &&
                      std::isfinite(s.cx) && std::isfinite(s.cy), "profile: dx = %g, dy = %g, 1/dr = %g must be finite and > 0, the centre (%g, %g) finite",
                      s.dx, s.dy, s.inv_dr, s.cx, s.cy);
    for (int k = 0; k < 5; k++)
        ARMON_REQUIRE(s.scale_exp[k] >= -4096 && s.scale_exp[k] <= 4096, "profile: scale_exp[%d] = %d leaves [-4096, 4096]", k, s.scale_exp[k]);
    p.f[0] = rho; p.f[1] = u; p.f[2] = v; p.f[3] = E;
    p.nrb = (wny + kTileRows - 1) / kTileRows;
    p.gx0 = global_col0; p.gy0 = global_row0;
    a.s = s;
    p.bins = BOUNDS ? nullptr : static_cast<u64*>(out_dev);
    p.bounds = BOUNDS ? static_cast<u64*>(out_dev) : nullptr;
    const uintptr_t mis = (uintptr_t)rho | (uintptr_t)u | (uintptr_t)v | (uintptr_t)E;
    const bool wide_ok = win::rows_are_16B(p.w, mis, wide<T>::n);
    const int64_t work = binned::pass_work(p.w, p.nrb, BOUNDS);
    rc = s.kind == ARMON_PROFILE_X   ? launch_kind<T, BOUNDS, ARMON_PROFILE_X>(ctx, wide_ok, work, a)
         : s.kind == ARMON_PROFILE_Y ? launch_kind<T, BOUNDS, ARMON_PROFILE_Y>(ctx, wide_ok, work, a)
                                     : launch_kind<T, BOUNDS, ARMON_PROFILE_R>(ctx, wide_ok, work, a);
    if (rc != ARMON_OK) return rc;
    return check_launch(BOUNDS ? "profile_bounds" : "profile");
}

}  // namespace

extern "C" {

int armon_hip_profile_reset(armon_ctx* ctx, int64_t nbins, armon_profile_bin* bins_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nbins >= 1 && nbins < (1ll << 48) && bins_dev, "profile_reset: nbins = %lld, bins_dev = %p", (long long)nbins, (void*)bins_dev);
    binned::launch_reset<kPairs, kRecWords>(ctx, nbins * kRecWords, bins_dev);
    return check_launch("profile_reset");
}

int armon_hip_profile(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, const double* u,
                      const double* v, const double* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                      int64_t global_row0, const armon_profile_spec* spec, armon_profile_bin* bins_dev)
{
    return profile_impl<double, false>(ctx, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0, spec, bins_dev);
}

int armon_hip_profile_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, const float* u,
                          const float* v, const float* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                          int64_t global_row0, const armon_profile_spec* spec, armon_profile_bin* bins_dev)
{
    return profile_impl<float, false>(ctx, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0, spec, bins_dev);
}

int armon_hip_profile_bounds(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, const double* u,
                             const double* v, const double* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                             int64_t global_row0, const armon_profile_spec* spec, uint64_t* bounds_dev)
{
    return profile_impl<double, true>(ctx, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0, spec, bounds_dev);
}

int armon_hip_profile_bounds_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, const float* u,
                                 const float* v, const float* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                                 int64_t global_row0, const armon_profile_spec* spec, uint64_t* bounds_dev)
{
    return profile_impl<float, true>(ctx, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0, spec, bounds_dev);
}

}  // extern "C"
