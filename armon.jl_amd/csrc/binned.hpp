// binned.hpp — the binned-record pass of the exact per-bin measures (profile.hip, mixing.hip), stated once:
// the record, its merge, the main pass, the bounds pass, the reset and the grid rule. A MEASURE says what a cell is worth:
//     NF, NX, kRecWords     fields read per cell, (min, max) pairs of a record, words from one record to the next in bins_dev
//     kAlongRows            the order of the tiles: false = down the rows of one span, true = along the spans of one row block
//     place                 what bin() leaves for terms() / add() (rx, ry, rr of a radius; empty for an axis)
//     tile_base(gxa, gxb, gya, gyb)   a lower bound of the bins the cells [gxa, gxb] x [gya, gyb] can touch
//     bin(gx, gy, place&)   the bin of a cell, < 0 = skipped
//     terms(cell, place, t) the five terms of a cell → false when the cell is bad
//     add(cell, place, acc) the cell into a lane record (terms, then add_terms and acc.take)
//
// RECORD: word 0 = n, word 1 = n_bad, words 2..16 = the 5 x 3 limb sums (exact_sum.hpp), from word 17 the (min, max) pairs
// of order keys; 17 + 2 NX words are used, the rest of kRecWords is reserved. A min word is neutral at ~0, every other at 0.
// Every word merges by integer addition, unsigned minimum or unsigned maximum: whatever the order, the same words.
//
// MAIN PASS. The lanes, the loads and the alignment rule are those of the window walk (window.hpp), the NF loads of a row
// issued before its first arithmetic. The window is cut into TILES of one span (64 lanes x 16 B) by 32 rows; a workgroup
// walks a contiguous run of tiles, its four waves taking 8 rows each, in the measure's order, so that a lane's bin or the
// wave's stays the same for as long as possible. A lane sums in registers while its bin does not change; when it changes
// the lane's record goes to a table of 264 bins in LDS (ds atomics: add, min, max on 64-bit words) whose first bin is the
// tile's tile_base, or straight to bins_dev where the bin falls outside the table. The table goes to bins_dev when its
// first bin changes and at the end: one 64-bit integer atomic per word that is not neutral, and for min / max only when a
// plain read says it can improve the word. No scratch, no host synchronisation. 264 bins cover a whole span in both types
// (an axis at width 1: 128 or 256 bins; a radius over square cells at dr = dx: 133 or 261), so only rings finer than a cell
// leave the table. Equal-bin neighbours are not combined across lanes before the LDS: the ds atomics of lanes in different
// bins do not serialise. The table (40 to 44 KB) allows 3 workgroups per CU, the registers 2 or 3: the grid is what the
// occupancy query reports for the variant launched (launch_resident), capped by PROFILE_WGS and by the work.
// BOUNDS PASS: the window walk; the bit pattern of the largest finite |t_k| of the window, merged by unsigned maximum.
#pragma once

#include "exact_sum.hpp"

namespace armon {
namespace binned {

using exact::u128;
using exact::u64;
using win::bits_of;
using win::finite;
using win::kWave;
using win::kWavesPerBlock;
using win::load_cells;
using win::wide;

constexpr int kTileRows = 32, kRowsPerWave = kTileRows / kWavesPerBlock;
constexpr int kTable = 264;                 // bins of the LDS table
constexpr int W_N = 0, W_BAD = 1, W_SUM = 2, W_EXT = 17;

template <int NX>
struct layout {
    static constexpr int used = W_EXT + 2 * NX;     // words of a record that are not reserved
    static __device__ __forceinline__ bool is_min(int w) { return w >= W_EXT && w < used && ((w - W_EXT) & 1) == 0; }
    static __device__ __forceinline__ bool is_max(int w) { return w >= W_EXT && w < used && ((w - W_EXT) & 1) == 1; }
    static __device__ __forceinline__ u64 neutral(int w) { return is_min(w) ? ~0ull : 0ull; }
};

template <typename T, int NF>
struct pass_args {
    const T* f[NF];                 // the fields of a cell
    win::window w;
    int64_t nrb;                    // blocks of kTileRows rows
    int64_t gx0, gy0;               // global position of the window's first cell
    u64* bins;                      // [nbins][kRecWords]
    u64* bounds;                    // [5] (the bounds pass)
};

template <int NX>
struct lane_rec {
    u64 n, n_bad;
    long long sum[5][3];
    u64 lo[NX], hi[NX];
    __device__ __forceinline__ void reset()
    {
        n = n_bad = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) sum[k][0] = sum[k][1] = sum[k][2] = 0;
#pragma unroll
        for (int j = 0; j < NX; j++) { lo[j] = ~0ull; hi[j] = 0; }
    }
    __device__ __forceinline__ void take(int j, u64 key)
    {
        lo[j] = key < lo[j] ? key : lo[j];
        hi[j] = key > hi[j] ? key : hi[j];
    }
};

// the terms of a cell into a lane record, each rounded on its own, all or none → false when the cell was bad
template <int NX>
__device__ __forceinline__ bool add_terms(const double t[5], bool ok, const int scale_exp[5], int nterms, lane_rec<NX>& acc)
{
    u128 a[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        a[k] = 0;
        if (k < nterms) ok = exact::quantise(t[k], scale_exp[k], a[k]) && ok;
    }
    if (!ok) {
        acc.n_bad += 1;
        return false;
    }
    acc.n += 1;
#pragma unroll
    for (int k = 0; k < 5; k++) exact::add_limbs(acc.sum[k], a[k], bits_of(t[k]) >> 63);
    return true;
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
template <int NX>
__device__ __forceinline__ void merge_rec(u64* dst, const lane_rec<NX>& r)
{
    if (r.n_bad) atomicAdd(dst + W_BAD, r.n_bad);
    if (r.n == 0) return;
    atomicAdd(dst + W_N, r.n);
#pragma unroll
    for (int k = 0; k < 5; k++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (r.sum[k][j]) atomicAdd(dst + W_SUM + 3 * k + j, (u64)r.sum[k][j]);
#pragma unroll
    for (int j = 0; j < NX; j++) {
        merge_min(dst + W_EXT + 2 * j, r.lo[j]);                    // (a pair nothing entered is neutral: the reads skip it)
        merge_max(dst + W_EXT + 2 * j + 1, r.hi[j]);
    }
}

template <typename M, typename T, bool WIDE>
__device__ __forceinline__ void main_pass(const M& m, const pass_args<T, M::NF>& a)
{
    typedef layout<M::NX> L;
    constexpr int V = wide<T>::n, NF = M::NF, kRec = L::used, kRecWords = M::kRecWords;
    __shared__ u64 table[kTable * kRec];
    __shared__ int table_hi;                                        // the last record of the table written since it last went out
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), w = tid / kWave;
    for (int i = tid; i < kTable * kRec; i += kBlock) table[i] = L::neutral(i % kRec);
    if (tid == 0) table_hi = -1;
    int64_t table_base = -1;                                        // workgroup-uniform
    const auto table_out = [&]() {                                  // (between two barriers)
        const int used = (table_hi + 1) * kRec;
        __syncthreads();
        if (tid == 0) table_hi = -1;
        for (int i = tid; i < used; i += kBlock) {
            const int word = i % kRec;
            const u64 v = table[i], neutral = L::neutral(word);
            if (v == neutral) continue;
            u64* dst = a.bins + (table_base + i / kRec) * kRecWords + word;     // only bins < nbins were ever written
            if (L::is_min(word)) merge_min(dst, v);
            else if (L::is_max(word)) merge_max(dst, v);
            else atomicAdd(dst, v);
            table[i] = neutral;
        }
    };
    lane_rec<M::NX> acc;
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
    const T* __restrict__ src[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) src[k] = a.f[k] + a.w.first;
    for (int64_t tile = t0; tile < t1; tile++) {
        const int64_t sp = M::kAlongRows ? tile % a.w.nspan : tile / a.nrb;
        const int64_t rb = M::kAlongRows ? tile / a.w.nspan : tile % a.nrb;
        const int64_t xa = sp * kWave * V, xb = xa + kWave * V < a.w.wnx ? xa + kWave * V : a.w.wnx;
        const int64_t ya = rb * kTileRows, yb = ya + kTileRows < a.w.wny ? ya + kTileRows : a.w.wny;
        const int64_t base = m.tile_base(a.gx0 + xa, a.gx0 + xb - 1, a.gy0 + ya, a.gy0 + yb - 1);
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
            T f[NF][V];                                             // the NF loads are issued before the first arithmetic
            const int64_t at = r * a.w.pitch + x;
#pragma unroll
            for (int k = 0; k < NF; k++) load_cells<T, WIDE>(src[k] + at, left >= V, left, f[k]);
#pragma unroll
            for (int c = 0; c < V; c++) {
                if (c >= left) break;
                typename M::place pl;
                const int64_t b = m.bin(a.gx0 + x + c, a.gy0 + r, pl);
                if (b < 0) continue;
                if (b != cur) {
                    lane_out();
                    cur = b;
                }
                T cell[NF];
#pragma unroll
                for (int k = 0; k < NF; k++) cell[k] = f[k][c];
                m.add(cell, pl, acc);
            }
        }
    }
    lane_out();
    __syncthreads();
    table_out();
}

template <typename M, typename T, bool WIDE>
__device__ __forceinline__ void bounds_pass(const M& m, const pass_args<T, M::NF>& a)
{
    constexpr int V = wide<T>::n, NF = M::NF;
    __shared__ u64 lds[kWavesPerBlock];
    const int tid = (int)threadIdx.x;
    const T* __restrict__ src[NF];
#pragma unroll
    for (int k = 0; k < NF; k++) src[k] = a.f[k] + a.w.first;
    u64 top[5] = {0, 0, 0, 0, 0};
    win::walk<V>(a.w, [&](int64_t r, int64_t x, int64_t left) {
        if (left <= 0) return;
        T f[NF][V];
        const int64_t at = r * a.w.pitch + x;
#pragma unroll
        for (int k = 0; k < NF; k++) load_cells<T, WIDE>(src[k] + at, left >= V, left, f[k]);
#pragma unroll
        for (int c = 0; c < V; c++) {
            if (c >= left) break;
            typename M::place pl;
            double t[5];
            T cell[NF];
#pragma unroll
            for (int k = 0; k < NF; k++) cell[k] = f[k][c];
            (void)m.bin(a.gx0 + x + c, a.gy0 + r, pl);              // every cell of the window counts, binned or not
            (void)m.terms(cell, pl, t);
#pragma unroll
            for (int k = 0; k < 5; k++) {
                const u64 v = bits_of(fabs(t[k]));
                if (finite(t[k]) && v > top[k]) top[k] = v;
            }
        }
    });
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const u64 v = red::block_reduce<red::op_umax, kWavesPerBlock>(top[k], lds, tid);
        if (tid == 0 && v) merge_max(a.bounds + k, v);
    }
}

// `words` words of records of NX pairs, kRecWords apart, to their neutral values
template <int NX, int kRecWords>
__global__ void k_reset(int64_t words, u64* __restrict__ bins)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < words) bins[i] = layout<NX>::neutral((int)(i % kRecWords));
}

template <int NX, int kRecWords>
inline void launch_reset(armon_ctx* ctx, int64_t words, void* bins)
{
    hipLaunchKernelGGL((k_reset<NX, kRecWords>), dim3((unsigned)((words + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, words,
                       static_cast<u64*>(bins));
}

// the work of a pass, in workgroups: the bounds pass deals a wave per (row, span) item, the main pass a workgroup per tile
inline int64_t pass_work(const win::window& w, int64_t nrb, bool bounds)
{
    return bounds ? (w.wny * w.nspan + kWavesPerBlock - 1) / kWavesPerBlock : w.nspan * nrb;
}

// launch `kernel` on the grid that is resident at once of THIS kernel, at most `work` workgroups and at most PROFILE_WGS
template <typename A>
int launch_resident(armon_ctx* ctx, void (*kernel)(A), int64_t work, const A& a)
{
    int per_cu = 0;
    ARMON_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0));
    int64_t blocks = (int64_t)ctx->n_cu * (per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu));
    if (ctx->tune_profile_wgs > 0 && blocks > ctx->tune_profile_wgs) blocks = ctx->tune_profile_wgs;     // no result bit changes
    if (blocks > work) blocks = work;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, a);
    return ARMON_OK;
}

}  // namespace binned
}  // namespace armon
