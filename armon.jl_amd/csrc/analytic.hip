// analytic.hip — the state against an exact solution, on the device: armon_hip_exact_norms reduces the distance of a window
// of real cells from the solution to one 128-byte record per variable (armon_exact_norm, include/armon_hip.h), and
// armon_hip_exact_fill writes the solution into the window. Nothing is moved: rho, u, v, E are read once (32 B per fp64
// cell), only the records are written.
//
// No reference counterpart: the reference has no exact solutions (its tests compare with golden files, ref test/reference_data).
//
// PER CELL (the full rule is in the header; armon.jl_amd/analytic.py restates it in Python and the tests hold this file
// against that): the solution (rho, un, p) at `samples` points per axis, each by ref_point — a Riemann fan in integer
// powers or a table with linear interpolation — their mean, then the mean AS THE DATA TYPE STORES IT (ref_cell: u, v, E from
// un, p; converted to T). Both the stored reference and the state go through cell_vars (rho, un, ut, p with p = the EOS in T),
// d = the difference of the two, and d, |d|, d d enter exact sums (exact_sum.hpp) and |d| a pair maximum. One definition
// serves both entry points, so a filled state is at distance 0, exactly. All of it fp64 but the EOS, no contraction
// (-ffp-contract=off for the whole library), IEEE division and square root.
//
// MERGE: integer addition and red::op_pair_max only — associative and commutative, so the records are a function of the state
// and the spec: not of the launch shape, the alignment path, the ghost width or the decomposition.
//
// Launch: the window walk of window.hpp, the four loads of an item issued before its arithmetic, kPerCu workgroups per CU. A
// lane keeps its 46 words in registers; wave shuffle -> LDS over the four waves -> one partial of 52 words per workgroup in
// the context's reduction scratch (ensure_partials) -> k_norm_fold, one workgroup per variable, merges them into out_dev.
// No atomics.
#include "exact_sum.hpp"

#include <cmath>

using namespace armon;

namespace {

constexpr int kVars = 4;                    // rho, un, ut, p
constexpr int kWords = 13;                  // per variable and partial: n, n_bad, 3 x 3 limbs, max_abs, max_abs_at
constexpr int kPerCu = 2;                   // workgroups per CU: what the registers allow (launch bounds below)

using exact::u64;
using exact::u128;
using exact::quantise;
using win::bits_of;
using win::finite;
using win::kNone;
using win::kWave;
using win::kWavesPerBlock;
using win::load_cells;
using win::pick;
using win::wide;

static_assert(sizeof(armon_exact_norm) == 128, "armon_exact_norm is 16 words");

template <typename T>
struct ex_args {
    T *rho, *u, *v, *E;
    win::window w;
    int64_t gx0, gy0;               // global position of the window's first cell
    armon_exact_spec s;
    u64* partials;                  // [gridDim.x][kVars][kWords]
};

// the solution at the coordinate q
__device__ __forceinline__ void ref_point(const armon_exact_spec& s, double q, double& rho, double& un, double& p)
{
    if (s.form == ARMON_EXACT_RIEMANN) {
        const double xi = q / s.time;
        int K = -1;
        if (xi < s.speed[0]) { rho = s.side[0][0]; un = s.side[0][1]; p = s.side[0][2]; }
        else if (xi < s.speed[1]) K = 0;
        else if (xi < s.speed[2]) { rho = s.star[2]; un = s.star[1]; p = s.star[0]; }
        else if (xi < s.speed[3]) { rho = s.star[3]; un = s.star[1]; p = s.star[0]; }
        else if (xi < s.speed[4]) K = 1;
        else { rho = s.side[1][0]; un = s.side[1][1]; p = s.side[1][2]; }
        if (K >= 0) {
            const bool L = K == 0;                                  // (selects: an index would put the spec into scratch)
            const double rhoK = L ? s.side[0][0] : s.side[1][0], uK = L ? s.side[0][1] : s.side[1][1];
            const double pK = L ? s.side[0][2] : s.side[1][2], cK = L ? s.side[0][3] : s.side[1][3];
            const double t = (L ? s.g2[0] : s.g2[1]) * (uK - xi);
            const double r = L ? s.g1 + t : s.g1 - t;
            const double r2 = r * r, r4 = r2 * r2, r5 = r4 * r, r7 = r5 * r2;
            rho = rhoK * r5;
            p = pK * r7;
            const double w = s.g3 * uK;
            un = s.g1 * (((L ? cK : -cK) + w) + xi);
        }
    } else {
        const double lam = q * s.inv_scale;
        if (!(lam < 1.)) { rho = s.outer[0]; un = s.outer[1]; p = s.outer[2]; return; }
        const double sc = lam * (double)s.M, fj = floor(sc);
        const int64_t j = fj > 0. ? (fj < (double)(s.M - 1) ? (int64_t)fj : s.M - 1) : 0;        // 0 <= j <= M - 1: nodes j, j + 1 exist
        const double f = sc - (double)j;
        const double* __restrict__ t = s.table;
        const int64_t row = s.M + 1;
        const double a0 = t[j], b0 = t[j + 1], a1 = t[row + j], b1 = t[row + j + 1], a2 = t[2 * row + j], b2 = t[2 * row + j + 1];
        rho = a0 + f * (b0 - a0);
        un = a1 + f * (b1 - a1);
        p = a2 + f * (b2 - a2);
    }
}

// the centre of cell (gx, gy) → whether its coordinate lies in [coord_min, coord_max)
__device__ __forceinline__ bool cell_centre(const armon_exact_spec& s, int64_t gx, int64_t gy, double& rx, double& ry, double& rr)
{
    rx = (((double)gx + 0.5) - s.cx) * s.dx;
    ry = (((double)gy + 0.5) - s.cy) * s.dy;
    rr = 0.;
    double q;
    if (s.coord == ARMON_PROFILE_X) q = rx;
    else if (s.coord == ARMON_PROFILE_Y) q = ry;
    else q = rr = sqrt(rx * rx + ry * ry);
    return q >= s.coord_min && q < s.coord_max;
}

// the reference of cell (gx, gy) as the data type stores it: rho, u, v, E
template <typename T>
__device__ __forceinline__ void ref_cell(const armon_exact_spec& s, int64_t gx, int64_t gy, double rx, double ry, double rr, T out[4])
{
    const int ns = s.samples;
    const double inv = 1. / (double)ns;                             // 1, 1/2, 1/4: exact
    double a_rho = 0., a_un = 0., a_p = 0., rho, un, p;
    if (s.coord == ARMON_PROFILE_R) {
        for (int j = 0; j < ns; j++) {
            const double py = (((double)gy + ((double)j + 0.5) * inv) - s.cy) * s.dy;
            for (int i = 0; i < ns; i++) {
                const double px = (((double)gx + ((double)i + 0.5) * inv) - s.cx) * s.dx;
                ref_point(s, sqrt(px * px + py * py), rho, un, p);
                a_rho += rho; a_un += un; a_p += p;
            }
        }
        const double w = inv * inv;
        a_rho *= w; a_un *= w; a_p *= w;
    } else {
        const bool along_x = s.coord == ARMON_PROFILE_X;
        const double g = along_x ? (double)gx : (double)gy, c = along_x ? s.cx : s.cy, h = along_x ? s.dx : s.dy;
        for (int i = 0; i < ns; i++) {
            ref_point(s, ((g + ((double)i + 0.5) * inv) - c) * h, rho, un, p);
            a_rho += rho; a_un += un; a_p += p;
        }
        a_rho *= inv; a_un *= inv; a_p *= inv;
    }
    double u, v;
    if (s.coord == ARMON_PROFILE_X) { u = a_un; v = 0.; }
    else if (s.coord == ARMON_PROFILE_Y) { u = 0.; v = a_un; }
    else if (rr == 0.) { u = 0.; v = 0.; }
    else { u = a_un * rx / rr; v = a_un * ry / rr; }
    const double gm1 = s.gamma - 1.;
    const double E = a_p / (gm1 * a_rho) + 0.5 * (u * u + v * v);
    out[0] = (T)a_rho; out[1] = (T)u; out[2] = (T)v; out[3] = (T)E;
}

// rho, un, ut, p of a cell's (rho, u, v, E) → false when one of the eight is not finite
template <typename T>
__device__ __forceinline__ bool cell_vars(const armon_exact_spec& s, T rho_, T u_, T v_, T E_, double rx, double ry, double rr, double t[4])
{
    const double rho = (double)rho_, u = (double)u_, v = (double)v_, E = (double)E_;
    double un, ut;
    if (s.coord == ARMON_PROFILE_X) { un = u; ut = v; }
    else if (s.coord == ARMON_PROFILE_Y) { un = v; ut = u; }
    else if (rr == 0.) { un = 0.; ut = 0.; }
    else { un = (u * rx + v * ry) / rr; ut = (v * rx - u * ry) / rr; }
    T p, c;
    phys::perfect_gas<T>((T)s.gamma, rho_, E_, u_, v_, p, c);      // (the sound speed is dead code here)
    t[0] = rho; t[1] = un; t[2] = ut; t[3] = (double)p;
    return finite(rho) && finite(u) && finite(v) && finite(E) && finite(un) && finite(ut) && finite(t[3]);
}

struct norm_acc {
    u64 n, n_bad;
    long long sum[kVars][3][3];     // [variable][d, |d|, d d][limb]
    red::upair mx[kVars];
};

template <typename T>
__device__ __forceinline__ void add_cell(const armon_exact_spec& s, T rho, T u, T v, T E, int64_t gx, int64_t gy, double rx, double ry,
                                         double rr, norm_acc& acc)
{
    T ref[4];
    ref_cell<T>(s, gx, gy, rx, ry, rr, ref);
    double a[kVars], b[kVars], d[kVars], sq[kVars];
    u128 q1[kVars], q2[kVars];
    bool ok = cell_vars<T>(s, rho, u, v, E, rx, ry, rr, a);
    ok = cell_vars<T>(s, ref[0], ref[1], ref[2], ref[3], rx, ry, rr, b) && ok;
#pragma unroll
    for (int k = 0; k < kVars; k++) {
        d[k] = a[k] - b[k];
        sq[k] = d[k] * d[k];
        ok = quantise(d[k], s.scale_exp[k][0], q1[k]) && ok;       // (|d| has the same |Q|)
        ok = quantise(sq[k], s.scale_exp[k][1], q2[k]) && ok;
    }
    // no branch from here on: a bad cell adds zeros (a second path through 92 accumulators doubles their registers)
    acc.n += ok ? 1 : 0;
    acc.n_bad += ok ? 0 : 1;
    const u64 g = (u64)gy * (u64)s.global_nx + (u64)gx;
#pragma unroll
    for (int k = 0; k < kVars; k++) {
        const u128 z1 = ok ? q1[k] : (u128)0, z2 = ok ? q2[k] : (u128)0;
        exact::add_limbs(acc.sum[k][0], z1, bits_of(d[k]) >> 63);
        exact::add_limbs(acc.sum[k][1], z1, false);
        exact::add_limbs(acc.sum[k][2], z2, false);
        const u64 m = ok ? bits_of(fabs(d[k])) : 0;
        acc.mx[k] = red::op_pair_max::f(acc.mx[k], red::upair{m, m ? g : kNone});
    }
}

template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock, kPerCu)
k_exact_norms(ex_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 lds[kWavesPerBlock][kVars * kWords];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    const T* __restrict__ rho = a.rho + a.w.first;
    const T* __restrict__ u = a.u + a.w.first;
    const T* __restrict__ v = a.v + a.w.first;
    const T* __restrict__ E = a.E + a.w.first;
    norm_acc acc;
    acc.n = acc.n_bad = 0;
#pragma unroll
    for (int k = 0; k < kVars; k++) {
        acc.mx[k] = red::upair{0, kNone};
#pragma unroll
        for (int j = 0; j < 9; j++) acc.sum[k][j / 3][j % 3] = 0;
    }
    win::walk<V>(a.w, [&](int64_t r, int64_t x, int64_t left) {
        if (left <= 0) return;
        T fr[V], fu[V], fv[V], fE[V];                               // the four loads are issued before the first arithmetic
        const int64_t at = r * a.w.pitch + x;
        load_cells<T, WIDE>(rho + at, left >= V, left, fr);
        load_cells<T, WIDE>(u + at, left >= V, left, fu);
        load_cells<T, WIDE>(v + at, left >= V, left, fv);
        load_cells<T, WIDE>(E + at, left >= V, left, fE);
#pragma nounroll                                                    // one copy of the cell's arithmetic: its temporaries next to the 92
        for (int c = 0; c < V; c++) {                               // accumulator registers leave no room for V interleaved copies
            if (c >= left) break;
            double rx, ry, rr;
            const int64_t gx = a.gx0 + x + c, gy = a.gy0 + r;
            if (!cell_centre(a.s, gx, gy, rx, ry, rr)) continue;
            add_cell<T>(a.s, pick<V>(fr, c), pick<V>(fu, c), pick<V>(fv, c), pick<V>(fE, c), gx, gy, rx, ry, rr, acc);
        }
    });
    // lane -> wave -> LDS -> one partial per workgroup
    const u64 n = red::wave_reduce<red::op_sum>(acc.n), n_bad = red::wave_reduce<red::op_sum>(acc.n_bad);
#pragma unroll
    for (int k = 0; k < kVars; k++) {
        u64* row = lds[w] + k * kWords;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            const u64 sum = red::wave_reduce<red::op_sum>((u64)acc.sum[k][j / 3][j % 3]);
            if (lane == 0) row[2 + j] = sum;
        }
        const red::upair m = red::wave_reduce<red::op_pair_max>(acc.mx[k]);
        if (lane == 0) { row[0] = n; row[1] = n_bad; row[11] = m.v; row[12] = m.at; }
    }
    __syncthreads();
    if (tid < kVars * kWords) {
        const int word = tid % kWords;
        u64* part = a.partials + (int64_t)blockIdx.x * (kVars * kWords);
        if (word < 11) {
            u64 sum = 0;
#pragma unroll
            for (int i = 0; i < kWavesPerBlock; i++) sum += lds[i][tid];
            part[tid] = sum;
        } else if (word == 11) {
            red::upair m{0, kNone};
#pragma unroll
            for (int i = 0; i < kWavesPerBlock; i++) m = red::op_pair_max::f(m, red::upair{lds[i][tid], lds[i][tid + 1]});
            part[tid] = m.v;
            part[tid + 1] = m.at;
        }
    }
}

// one workgroup per variable: out[q] = merge(out[q], the partials)
__global__ void __launch_bounds__(kBlock)
k_norm_fold(const u64* __restrict__ partials, int n, armon_exact_norm* __restrict__ out)
{
    __shared__ u64 lds[kWavesPerBlock];
    __shared__ red::upair lds_pair[kWavesPerBlock];
    const int q = blockIdx.x, tid = (int)threadIdx.x;
    u64 sum[11];
#pragma unroll
    for (int j = 0; j < 11; j++) sum[j] = 0;
    red::upair m{0, kNone};
    for (int i = tid; i < n; i += kBlock) {
        const u64* p = partials + ((int64_t)i * kVars + q) * kWords;
#pragma unroll
        for (int j = 0; j < 11; j++) sum[j] += p[j];
        m = red::op_pair_max::f(m, red::upair{p[11], p[12]});
    }
#pragma unroll
    for (int j = 0; j < 11; j++) sum[j] = red::block_reduce<red::op_sum, kWavesPerBlock>(sum[j], lds, tid);
    m = red::block_reduce<red::op_pair_max, kWavesPerBlock>(m, lds_pair, tid);
    if (tid == 0) {
        armon_exact_norm d = out[q];
        d.n += sum[0]; d.n_bad += sum[1];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            d.sum_d[j] = (int64_t)((u64)d.sum_d[j] + sum[2 + j]);
            d.sum_abs[j] = (int64_t)((u64)d.sum_abs[j] + sum[5 + j]);
            d.sum_sq[j] = (int64_t)((u64)d.sum_sq[j] + sum[8 + j]);
        }
        const red::upair A = red::op_pair_max::f(red::upair{d.max_abs, d.max_abs_at}, m);
        d.max_abs = A.v; d.max_abs_at = A.at;
        out[q] = d;
    }
}

__global__ void k_norm_reset(armon_exact_norm* __restrict__ out)
{
    const int q = threadIdx.x;
    if (q < kVars) {
        armon_exact_norm d = {};
        d.max_abs_at = kNone;
        out[q] = d;
    }
}

template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock)
k_exact_fill(ex_args<T> a)
{
    constexpr int V = wide<T>::n;
    typedef typename wide<T>::type VT;
    T* __restrict__ dst[4] = {a.rho + a.w.first, a.u + a.w.first, a.v + a.w.first, a.E + a.w.first};
    // (the loop of win::walk written out: as a callable it changes this kernel's occupancy)
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave, nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t units = a.w.wny * a.w.nspan;
    for (int64_t unit = wave; unit < units; unit += nwaves) {
        const int64_t r = unit / a.w.nspan;
        const auto [x, left] = win::lane_column<V>(a.w, unit % a.w.nspan, lane);
        if (left <= 0) continue;
        const int64_t at = r * a.w.pitch + x;                         // at + c < the window's row end for c < left
        T val[V][4];
        bool keep[V], all = left >= V;
#pragma unroll
        for (int c = 0; c < V; c++) {
            keep[c] = false;
            if (c >= left) continue;
            double rx, ry, rr;
            const int64_t gx = a.gx0 + x + c, gy = a.gy0 + r;
            keep[c] = cell_centre(a.s, gx, gy, rx, ry, rr);
            if (keep[c]) ref_cell<T>(a.s, gx, gy, rx, ry, rr, val[c]);
            all = all && keep[c];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (WIDE && all) {
                VT wv;
#pragma unroll
                for (int c = 0; c < V; c++) wv[c] = val[c][q];
                *reinterpret_cast<VT*>(dst[q] + at) = wv;
            } else {
#pragma unroll
                for (int c = 0; c < V; c++)
                    if (keep[c]) dst[q][at + c] = val[c][q];
            }
        }
    }
}

template <typename T, bool FILL>
int exact_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, T* rho, T* u, T* v, T* E, int64_t col0, int64_t row0,
               int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0, const armon_exact_spec* spec, armon_exact_norm* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(rho && u && v && E && spec && (FILL || out_dev), "NULL argument");
    ex_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
    if (rc == ARMON_OK) rc = win::check_global_cell(global_col0, global_row0);
    if (rc != ARMON_OK) return rc;
    const armon_exact_spec& s = *spec;
    ARMON_REQUIRE(s.form == ARMON_EXACT_RIEMANN || s.form == ARMON_EXACT_TABLE, "unknown form %d of the exact solution", s.form);
    ARMON_REQUIRE(s.coord == ARMON_PROFILE_X || s.coord == ARMON_PROFILE_Y || s.coord == ARMON_PROFILE_R, "unknown coordinate %d", s.coord);
    ARMON_REQUIRE(s.samples == 1 || s.samples == 2 || s.samples == 4, "exact solution: samples = %d, not 1, 2 or 4", s.samples);
    ARMON_REQUIRE(s.eos == ARMON_EOS_PERFECT_GAS, "exact solution: eos = %d, only the perfect gas has one", s.eos);
    ARMON_REQUIRE(s.global_nx >= global_col0 + wnx && s.global_nx < (1ll << 40), "exact solution: global_nx = %lld", (long long)s.global_nx);
    ARMON_REQUIRE(std::isfinite(s.dx) && std::isfinite(s.dy) && s.dx > 0 && s.dy > 0 && std::isfinite(s.cx) && std::isfinite(s.cy),
                  "exact solution: dx = %g, dy = %g must be finite and > 0, the centre (%g, %g) finite", s.dx, s.dy, s.cx, s.cy);
    ARMON_REQUIRE(std::isfinite(s.gamma) && s.gamma > 1, "exact solution: gamma = %g", s.gamma);
    ARMON_REQUIRE(!std::isnan(s.coord_min) && !std::isnan(s.coord_max), "exact solution: coord_min / coord_max is NaN");
    if (s.form == ARMON_EXACT_RIEMANN) {
        ARMON_REQUIRE(s.gamma == 7. / 5., "exact Riemann solution: gamma = %.17g, the fans are written for 7/5 only", s.gamma);
        ARMON_REQUIRE(std::isfinite(s.time) && s.time > 0, "exact Riemann solution: time = %g must be finite and > 0", s.time);
    } else {
        ARMON_REQUIRE(s.M >= 1 && s.M < (1ll << 40) && s.table, "exact table: M = %lld, table = %p", (long long)s.M, (const void*)s.table);
        ARMON_REQUIRE(std::isfinite(s.inv_scale) && s.inv_scale > 0, "exact table: 1/scale = %g must be finite and > 0", s.inv_scale);
    }
    for (int k = 0; k < kVars && !FILL; k++)
        for (int j = 0; j < 2; j++)
            ARMON_REQUIRE(s.scale_exp[k][j] >= -4096 && s.scale_exp[k][j] <= 4096, "exact solution: scale_exp[%d][%d] = %d leaves [-4096, 4096]",
                          k, j, s.scale_exp[k][j]);
    a.rho = rho; a.u = u; a.v = v; a.E = E;
    a.gx0 = global_col0; a.gy0 = global_row0;
    a.s = s;
    a.partials = nullptr;
    const uintptr_t mis = (uintptr_t)rho | (uintptr_t)u | (uintptr_t)v | (uintptr_t)E;
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n);
    const int64_t blocks = win::walk_blocks(a.w, (int64_t)ctx->n_cu * kPerCu);
    const dim3 grid((unsigned)blocks), block(kBlock);
    if (FILL) {
        if (wide_ok) hipLaunchKernelGGL((k_exact_fill<T, true>), grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL((k_exact_fill<T, false>), grid, block, 0, ctx->stream, a);
        return check_launch("exact_fill");
    }
    rc = ensure_partials(ctx, (size_t)kVars * kWords * blocks);  // (doubles and 64-bit words have the same size)
    if (rc != ARMON_OK) return rc;
    a.partials = reinterpret_cast<u64*>(ctx->partials);
    if (wide_ok) hipLaunchKernelGGL((k_exact_norms<T, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_exact_norms<T, false>), grid, block, 0, ctx->stream, a);
    rc = check_launch("exact_norms");
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_norm_fold, dim3(kVars), block, 0, ctx->stream, a.partials, (int)blocks, out_dev);
    return check_launch("exact_norm_fold");
}

}  // namespace

extern "C" {

int armon_hip_exact_norms_reset(armon_ctx* ctx, armon_exact_norm* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(out_dev, "exact_norms_reset: out_dev is NULL");
    hipLaunchKernelGGL(k_norm_reset, dim3(1), dim3(kWave), 0, ctx->stream, out_dev);
    return check_launch("exact_norms_reset");
}

int armon_hip_exact_norms(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, const double* u,
                          const double* v, const double* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                          int64_t global_row0, const armon_exact_spec* spec, armon_exact_norm* out_dev)
{
    return exact_impl<double, false>(ctx, row_length, nghost, nx, ny, const_cast<double*>(rho), const_cast<double*>(u), const_cast<double*>(v),
                                     const_cast<double*>(E), col0, row0, wnx, wny, global_col0, global_row0, spec, out_dev);
}

int armon_hip_exact_norms_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, const float* u,
                              const float* v, const float* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
                              int64_t global_row0, const armon_exact_spec* spec, armon_exact_norm* out_dev)
{
    return exact_impl<float, false>(ctx, row_length, nghost, nx, ny, const_cast<float*>(rho), const_cast<float*>(u), const_cast<float*>(v),
                                    const_cast<float*>(E), col0, row0, wnx, wny, global_col0, global_row0, spec, out_dev);
}

int armon_hip_exact_fill(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, double* rho, double* u, double* v,
                         double* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0,
                         const armon_exact_spec* spec)
{
    return exact_impl<double, true>(ctx, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0, spec, nullptr);
}

int armon_hip_exact_fill_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, float* rho, float* u, float* v,
                             float* E, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0,
                             const armon_exact_spec* spec)
{
    return exact_impl<float, true>(ctx, row_length, nghost, nx, ny, rho, u, v, E, col0, row0, wnx, wny, global_col0, global_row0, spec, nullptr);
}

}  // extern "C"
