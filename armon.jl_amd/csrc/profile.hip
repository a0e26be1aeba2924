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
// Launch. The lanes, the loads and the alignment rule are those of the window walk (window.hpp), the four loads of a row
// issued before its first arithmetic; the bounds pass is that walk. The main pass has an item of its own: the window is cut
// into TILES of one span (64 lanes x 16 B) by 32 rows; a workgroup walks a contiguous run of tiles, its four waves taking 8
// rows each. The order of
// the tiles follows the kind: down the rows of one span for X and R, along the spans of one row block for Y, so a lane's
// bin (X) or the wave's (Y) stays the same for as long as possible. A lane sums in registers (21 words) while its bin does
// not change; when it changes the lane's record goes to a table of 264 bins in LDS (ds atomics: add, min, max on 64-bit
// words) whose first bin is the smallest bin the tile can touch, or straight to bins_dev where the bin falls outside the
// table. The table goes to bins_dev when its first bin changes (once per span for X, once per row block for Y, once per
// tile for R) and at the end: one 64-bit integer atomic per word that is not neutral, and for min / max only when a plain
// read says it can improve the word. Integer atomics only: whatever the order, the same words. No scratch, no host
// synchronisation. 264 bins cover a whole span in both types (X at width 1: 128 or 256 bins; R over square cells at dr = dx:
// 133 or 261), so only rings finer than a cell leave the table. 44.4 KB of LDS per workgroup = 3 workgroups per CU, which is
// also what the registers allow (148 to 209 VGPRs: 3, or 2 for the larger variants); the grid is what the occupancy query
// reports for the variant launched. Equal-bin neighbours of R are not combined across lanes before the LDS: a record is 21
// words, and the ds atomics of lanes in different bins do not serialise.
#include "exact_sum.hpp"

#include <cmath>

using namespace armon;

namespace {

using win::kWave;
using win::kWavesPerBlock;
constexpr int kTileRows = 32, kRowsPerWave = kTileRows / kWavesPerBlock;
constexpr int kRec = 21;                    // words of a record that are not reserved
constexpr int kRecWords = 24;               // sizeof(armon_profile_bin) / 8
constexpr int kTable = 264;                 // bins of the LDS table: a span is 128 (fp64) or 256 (fp32) columns, so X at width 1 needs 256
                                            // and R over square cells at dr = dx reaches 133 or 261
constexpr int W_N = 0, W_BAD = 1, W_SUM = 2, W_RHO_MIN = 17, W_RHO_MAX = 18, W_P_MIN = 19, W_P_MAX = 20;

using exact::u64;
using exact::u128;
using exact::quantise;
using red::order_key;
using win::bits_of;
using win::finite;
using win::load_cells;
using win::wide;

static_assert(sizeof(armon_profile_bin) == kRecWords * 8, "armon_profile_bin is 24 words");

__device__ __forceinline__ bool is_min_word(int w) { return w == W_RHO_MIN || w == W_P_MIN; }
__device__ __forceinline__ bool is_max_word(int w) { return w == W_RHO_MAX || w == W_P_MAX; }

template <typename T>
struct prof_args {
    const T *rho, *u, *v, *E;
    win::window w;
    int64_t nrb;                    // blocks of kTileRows rows
    int64_t gx0, gy0;               // global position of the window's first cell
    armon_profile_spec s;
    u64* bins;                      // [nbins][kRecWords]
    u64* bounds;                    // [5] (the bounds pass)
};

struct lane_rec {
    u64 n, n_bad;
    long long sum[5][3];
    u64 rho_min, rho_max, p_min, p_max;
    __device__ __forceinline__ void reset()
    {
        n = n_bad = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) sum[k][0] = sum[k][1] = sum[k][2] = 0;
        rho_min = p_min = ~0ull;
        rho_max = p_max = 0;
    }
};

// the five terms of a cell → false when the cell is bad
template <typename T, int KIND>
__device__ __forceinline__ bool cell_terms(const armon_profile_spec& s, T rho_, T u_, T v_, T E_, double rx, double ry, double rr,
                                           double t[5])
{
    const double rho = (double)rho_, u = (double)u_, v = (double)v_, E = (double)E_;
    double un, ut;
    if (KIND == ARMON_PROFILE_X) { un = u; ut = v; }
    else if (KIND == ARMON_PROFILE_Y) { un = v; ut = u; }
    else if (rr == 0.) { un = 0.; ut = 0.; }
    else { un = (u * rx + v * ry) / rr; ut = (v * rx - u * ry) / rr; }
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
__device__ __forceinline__ int64_t cell_bin(const armon_profile_spec& s, int64_t gx, int64_t gy, double& rx, double& ry, double& rr)
{
    rx = ry = rr = 0.;
    int64_t b;
    if (KIND == ARMON_PROFILE_X) b = gx / s.width;
    else if (KIND == ARMON_PROFILE_Y) b = gy / s.width;
    else {
        rx = ((double)gx + 0.5 - s.cx) * s.dx;
        ry = ((double)gy + 0.5 - s.cy) * s.dy;
        rr = sqrt(rx * rx + ry * ry);
        const double fb = floor(rr * s.inv_dr);
        if (!(fb < (double)s.nbins)) return -1;                     // (a NaN is skipped too)
        b = (int64_t)fb;
    }
    return b < s.nbins ? b : -1;
}

template <typename T, int KIND>
__device__ __forceinline__ void add_cell(const armon_profile_spec& s, T rho, T u, T v, T E, double rx, double ry, double rr, lane_rec& acc)
{
    double t[5];
    u128 a[5];
    bool ok = cell_terms<T, KIND>(s, rho, u, v, E, rx, ry, rr, t);
    const int nterms = s.eos >= 0 ? 5 : 4;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        a[k] = 0;
        if (k < nterms) ok = quantise(t[k], s.scale_exp[k], a[k]) && ok;
    }
    if (!ok) {
        acc.n_bad += 1;
        return;
    }
    acc.n += 1;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        exact::add_limbs(acc.sum[k], a[k], bits_of(t[k]) >> 63);
    }
    const u64 kr = order_key(t[0]);
    acc.rho_min = kr < acc.rho_min ? kr : acc.rho_min;
    acc.rho_max = kr > acc.rho_max ? kr : acc.rho_max;
    if (s.eos >= 0) {
        const u64 kp = order_key(t[4]);
        acc.p_min = kp < acc.p_min ? kp : acc.p_min;
        acc.p_max = kp > acc.p_max ? kp : acc.p_max;
    }
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
    merge_min(dst + W_RHO_MIN, r.rho_min);
    merge_max(dst + W_RHO_MAX, r.rho_max);
    merge_min(dst + W_P_MIN, r.p_min);                              // (neutral without p: the reads skip them)
    merge_max(dst + W_P_MAX, r.p_max);
}

// the smallest bin a tile can touch (a lower bound is enough: it only decides what goes through the LDS table)
template <int KIND>
__device__ __forceinline__ int64_t tile_base(const armon_profile_spec& s, int64_t gxa, int64_t gxb, int64_t gya, int64_t gyb)
{
    if (KIND == ARMON_PROFILE_X) return gxa / s.width;
    if (KIND == ARMON_PROFILE_Y) return gya / s.width;
    const double xa = (double)gxa + 0.5 - s.cx, xb = (double)gxb + 0.5 - s.cx, ya = (double)gya + 0.5 - s.cy, yb = (double)gyb + 0.5 - s.cy;
    const double ddx = (xa > 0. ? xa : (xb < 0. ? -xb : 0.)) * s.dx, ddy = (ya > 0. ? ya : (yb < 0. ? -yb : 0.)) * s.dy;
    const double fb = floor(sqrt(ddx * ddx + ddy * ddy) * s.inv_dr) - 1.;
    return fb > 0. ? (fb < 4e18 ? (int64_t)fb : (int64_t)4e18) : 0;
}

template <typename T, bool WIDE, int KIND>
__global__ void __launch_bounds__(kBlock, 2)       // 150 to 193 VGPRs: capped lower, the 21-word record spills
k_profile(prof_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 table[kTable * kRec];
    __shared__ int table_hi;                                        // the last record of the table written since it last went out
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    for (int i = tid; i < kTable * kRec; i += kBlock) table[i] = is_min_word(i % kRec) ? ~0ull : 0ull;
    if (tid == 0) table_hi = -1;
    int64_t table_base = -1;                                        // workgroup-uniform
    const auto table_out = [&]() {                                  // (between two barriers)
        const int used = (table_hi + 1) * kRec;
        __syncthreads();
        if (tid == 0) table_hi = -1;
        for (int i = tid; i < used; i += kBlock) {
            const int word = i % kRec;
            const u64 v = table[i], neutral = is_min_word(word) ? ~0ull : 0ull;
            if (v == neutral) continue;
            u64* dst = a.bins + (table_base + i / kRec) * kRecWords + word;     // only bins < nbins were ever written
            if (is_min_word(word)) merge_min(dst, v);
            else if (is_max_word(word)) merge_max(dst, v);
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
    const T* __restrict__ u = a.u + a.w.first;
    const T* __restrict__ v = a.v + a.w.first;
    const T* __restrict__ E = a.E + a.w.first;
    for (int64_t tile = t0; tile < t1; tile++) {
        const int64_t sp = KIND == ARMON_PROFILE_Y ? tile % a.w.nspan : tile / a.nrb;
        const int64_t rb = KIND == ARMON_PROFILE_Y ? tile / a.w.nspan : tile % a.nrb;
        const int64_t xa = sp * kWave * V, xb = xa + kWave * V < a.w.wnx ? xa + kWave * V : a.w.wnx;
        const int64_t ya = rb * kTileRows, yb = ya + kTileRows < a.w.wny ? ya + kTileRows : a.w.wny;
        const int64_t base = tile_base<KIND>(a.s, a.gx0 + xa, a.gx0 + xb - 1, a.gy0 + ya, a.gy0 + yb - 1);
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
            T fr[V], fu[V], fv[V], fE[V];                           // the four loads are issued before the first arithmetic
            const int64_t at = r * a.w.pitch + x;
            load_cells<T, WIDE>(rho + at, left >= V, left, fr);
            load_cells<T, WIDE>(u + at, left >= V, left, fu);
            load_cells<T, WIDE>(v + at, left >= V, left, fv);
            load_cells<T, WIDE>(E + at, left >= V, left, fE);
#pragma unroll
            for (int c = 0; c < V; c++) {
                if (c >= left) break;
                double rx, ry, rr;
                const int64_t b = cell_bin<KIND>(a.s, a.gx0 + x + c, a.gy0 + r, rx, ry, rr);
                if (b < 0) continue;
                if (b != cur) {
                    lane_out();
                    cur = b;
                }
                add_cell<T, KIND>(a.s, fr[c], fu[c], fv[c], fE[c], rx, ry, rr, acc);
            }
        }
    }
    lane_out();
    __syncthreads();
    table_out();
}

// the bounds pass: the bit pattern of the largest finite |t_k| of the window, merged by unsigned maximum
template <typename T, bool WIDE, int KIND>
__global__ void __launch_bounds__(kBlock, 4)
k_profile_bounds(prof_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 lds[kWavesPerBlock];
    const int tid = (int)threadIdx.x;
    const T* __restrict__ rho = a.rho + a.w.first;
    const T* __restrict__ u = a.u + a.w.first;
    const T* __restrict__ v = a.v + a.w.first;
    const T* __restrict__ E = a.E + a.w.first;
    u64 top[5] = {0, 0, 0, 0, 0};
    // (the loop of win::walk written out, lane arithmetic included: the fp64 element-path variant for R sits two registers above
    // an occupancy step, and the callable and win::lane_column each move it across)
    const int lane = tid & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + tid / kWave, nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t units = a.w.wny * a.w.nspan;
    for (int64_t unit = wave; unit < units; unit += nwaves) {
        const int64_t sp = unit % a.w.nspan, r = unit / a.w.nspan;
        const int64_t x = (sp * kWave + lane) * V, left = a.w.wnx - x;
        if (left <= 0) continue;
        T fr[V], fu[V], fv[V], fE[V];
        const int64_t at = r * a.w.pitch + x;
        load_cells<T, WIDE>(rho + at, left >= V, left, fr);
        load_cells<T, WIDE>(u + at, left >= V, left, fu);
        load_cells<T, WIDE>(v + at, left >= V, left, fv);
        load_cells<T, WIDE>(E + at, left >= V, left, fE);
#pragma unroll
        for (int c = 0; c < V; c++) {
            if (c >= left) break;
            double rx, ry, rr, t[5];
            (void)cell_bin<KIND>(a.s, a.gx0 + x + c, a.gy0 + r, rx, ry, rr);     // every cell of the window counts, binned or not
            (void)cell_terms<T, KIND>(a.s, fr[c], fu[c], fv[c], fE[c], rx, ry, rr, t);
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const u64 m = bits_of(fabs(t[k]));
                if (finite(t[k]) && m > top[k]) top[k] = m;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const u64 m = red::block_reduce<red::op_umax, kWavesPerBlock>(top[k], lds, tid);
        if (tid == 0 && m) merge_max(a.bounds + k, m);
    }
}

__global__ void k_profile_reset(int64_t nbins, u64* __restrict__ bins)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nbins * kRecWords) bins[i] = is_min_word((int)(i % kRecWords)) ? ~0ull : 0ull;
}

template <typename T, bool BOUNDS>
int profile_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, const T* rho, const T* u, const T* v, const T* E,
                 int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0,
                 const armon_profile_spec* spec, void* out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(rho && u && v && E && spec && out_dev, "NULL argument");
    prof_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
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
    a.rho = rho; a.u = u; a.v = v; a.E = E;
    a.nrb = (wny + kTileRows - 1) / kTileRows;
    a.gx0 = global_col0; a.gy0 = global_row0;
    a.s = s;
    a.bins = BOUNDS ? nullptr : static_cast<u64*>(out_dev);
    a.bounds = BOUNDS ? static_cast<u64*>(out_dev) : nullptr;
    const uintptr_t mis = (uintptr_t)rho | (uintptr_t)u | (uintptr_t)v | (uintptr_t)E;
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n);
    // the bounds pass: a wave per (row, span) item; the main pass: a workgroup per tile
    const int64_t work = BOUNDS ? (a.w.wny * a.w.nspan + kWavesPerBlock - 1) / kWavesPerBlock : a.w.nspan * a.nrb;
    const dim3 block(kBlock);
    // the grid = what is resident at once of THIS variant (registers allow 2 or 3 workgroups per CU of the main pass, its LDS 3)
#define ARMON_PROFILE_LAUNCH_1(KERNEL, W, KIND)                                                                 \
    do {                                                                                                        \
        int per_cu = 0;                                                                                         \
        ARMON_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, KERNEL<T, W, KIND>, kBlock, 0));    \
        int64_t blocks = (int64_t)ctx->n_cu * (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));                     \
        if (ctx->tune_profile_wgs > 0 && blocks > ctx->tune_profile_wgs) blocks = ctx->tune_profile_wgs;        \
        if (blocks > work) blocks = work;                                                                       \
        hipLaunchKernelGGL((KERNEL<T, W, KIND>), dim3((unsigned)blocks), block, 0, ctx->stream, a);             \
    } while (0)
#define ARMON_PROFILE_LAUNCH(KERNEL, KIND)                                                                      \
    do {                                                                                                        \
        if (wide_ok) ARMON_PROFILE_LAUNCH_1(KERNEL, true, KIND);                                                \
        else ARMON_PROFILE_LAUNCH_1(KERNEL, false, KIND);                                                       \
    } while (0)
    if (BOUNDS) {
        if (s.kind == ARMON_PROFILE_X) ARMON_PROFILE_LAUNCH(k_profile_bounds, ARMON_PROFILE_X);
        else if (s.kind == ARMON_PROFILE_Y) ARMON_PROFILE_LAUNCH(k_profile_bounds, ARMON_PROFILE_Y);
        else ARMON_PROFILE_LAUNCH(k_profile_bounds, ARMON_PROFILE_R);
    } else {
        if (s.kind == ARMON_PROFILE_X) ARMON_PROFILE_LAUNCH(k_profile, ARMON_PROFILE_X);
        else if (s.kind == ARMON_PROFILE_Y) ARMON_PROFILE_LAUNCH(k_profile, ARMON_PROFILE_Y);
        else ARMON_PROFILE_LAUNCH(k_profile, ARMON_PROFILE_R);
    }
#undef ARMON_PROFILE_LAUNCH
#undef ARMON_PROFILE_LAUNCH_1
    return check_launch(BOUNDS ? "profile_bounds" : "profile");
}

}  // namespace

extern "C" {

int armon_hip_profile_reset(armon_ctx* ctx, int64_t nbins, armon_profile_bin* bins_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nbins >= 1 && nbins < (1ll << 48) && bins_dev, "profile_reset: nbins = %lld, bins_dev = %p", (long long)nbins, (void*)bins_dev);
    const int64_t words = nbins * kRecWords;
    hipLaunchKernelGGL(k_profile_reset, dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, nbins,
                       reinterpret_cast<u64*>(bins_dev));
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
