// checkpoint.hip — checkpoint / restart: move a window of real cells between the block's vectors and a dense buffer, and
// digest what was moved, in one pass.
//
// No reference counterpart (the reference's only state files are text, ref src/io.jl:2-27). A window is the real cells
// [col0, col0 + wnx) x [row0, row0 + wny) of a block; the dense side is [nvars][wny][wnx]. Ghost cells are never read or
// written. `pack` reads the vectors (dense side optional: NULL = digest only), `unpack` writes them.
//
// THE DIGEST of variable k (its index in the call) is the sum mod 2^64, over the cells of the window, of
//     mix64(b + mix64(8 g + k + 1)),     g = gy NX + gx the GLOBAL 0-based index of the cell, b its bit pattern zero-extended,
//     mix64: z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31.
// Integer addition is associative: the digest is a function of the values and their global positions only — not of the
// launch shape, the band split, the alignment path, the ghost width or the decomposition — and the digest of a domain is the
// sum of the digests of its parts. Each call ADDS its window's digests to `digest_dev[k]` (the caller clears them once), so
// the bands of a checkpoint accumulate on the device with no host synchronisation.
//
// Launch: the window walk of window.hpp over the vectors and the dense buffer (16-B rows there need wnx to be a multiple of
// V), 8 workgroups per CU. Reduction as in reduce.hpp: lane -> wave shuffle -> LDS over the waves -> one partial per
// workgroup and variable -> fold kernel. No atomics.
// The partials live in the context's reduction scratch: the first call whose grid needs more of it than the context has
// (ensure_partials) synchronises the stream once to grow it, and is refused while a captured graph of the context is alive;
// apart from that the calls never synchronise with the host.
#include "window.hpp"

using namespace armon;

// sources are read once: non-temporal loads (0 = plain loads; A/B by -DARMON_CKPT_NT=0)
#ifndef ARMON_CKPT_NT
#define ARMON_CKPT_NT 1
#endif

namespace {

constexpr int kMaxVars = 8;

using win::bits_of;
using win::kWavesPerBlock;
using win::load_cells;
using win::store_cells;
using win::wide;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
    z ^= z >> 27; z *= 0x94d049bb133111ebull;
    z ^= z >> 31;
    return z;
}

template <typename T>
struct state_args {
    T* vars[kMaxVars];              // pack: read only
    T* dense;                       // [nvars][wny][wnx]; NULL (pack only) = digest only
    unsigned long long* partials;   // [kMaxVars][gridDim.x]
    win::window w;
    uint64_t g0, NX;                // global index of the window's first cell, global row length
    int nvars;
};

// One (row, span) item per wave and turn. UNPACK: dense -> vectors; otherwise vectors -> dense (when there is one).
template <typename T, bool WIDE, bool UNPACK>
__global__ void __launch_bounds__(kBlock)
k_state_move(state_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ unsigned long long lds[kWavesPerBlock];
    const int64_t plane = a.w.wny * a.w.wnx;
    const bool has_dense = a.dense != nullptr;
    unsigned long long acc[kMaxVars];
#pragma unroll
    for (int q = 0; q < kMaxVars; q++) acc[q] = 0;
    // (the loop of win::walk written out: as a callable it changes this kernel's occupancy)
    const int lane = threadIdx.x & (win::kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / win::kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock, units = a.w.wny * a.w.nspan;
    for (int64_t unit = wave; unit < units; unit += nwaves) {      // wave-uniform
        const int64_t r = unit / a.w.nspan;
        const auto [x, left] = win::lane_column<V>(a.w, unit % a.w.nspan, lane);
        if (left <= 0) continue;
        const bool whole = left >= V;
        const int64_t at = a.w.first + r * a.w.pitch + x, dat = r * a.w.wnx + x;
        const uint64_t g8 = 8 * (a.g0 + (uint64_t)r * a.NX + (uint64_t)x) + 1;
#pragma unroll
        for (int q = 0; q < kMaxVars; q++) {
            if (q < a.nvars) {                                     // uniform
                T f[V];
                if (UNPACK) {
                    load_cells<T, WIDE, ARMON_CKPT_NT>(a.dense + q * plane + dat, whole, left, f);
                    store_cells<T, WIDE>(a.vars[q] + at, whole, left, f);
                } else {
                    load_cells<T, WIDE, ARMON_CKPT_NT>(a.vars[q] + at, whole, left, f);
                    if (has_dense) store_cells<T, WIDE>(a.dense + q * plane + dat, whole, left, f);
                }
#pragma unroll
                for (int c = 0; c < V; c++)
                    if (c < left) acc[q] += mix64(bits_of(f[c]) + mix64(g8 + 8 * (uint64_t)c + (uint64_t)q));
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kMaxVars; q++) {
        if (q < a.nvars) {                                         // uniform
            const unsigned long long v = red::block_reduce<red::op_sum, kWavesPerBlock>(acc[q], lds, (int)threadIdx.x);
            if (threadIdx.x == 0) a.partials[(int64_t)q * gridDim.x + blockIdx.x] = v;
        }
    }
}

// one workgroup per variable: digest[q] += sum of its partials
__global__ void __launch_bounds__(kBlock)
k_digest_fold(const unsigned long long* __restrict__ partials, int n, unsigned long long* __restrict__ digest)
{
    __shared__ unsigned long long lds[kWavesPerBlock];
    const int q = blockIdx.x;
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < n; i += kBlock) acc += partials[(int64_t)q * n + i];
    acc = red::block_reduce<red::op_sum, kWavesPerBlock>(acc, lds, (int)threadIdx.x);
    if (threadIdx.x == 0) digest[q] += acc;
}

template <typename T, bool UNPACK>
int state_move_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars, T* const* vars,
                    int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first, int64_t global_nx,
                    T* dense_dev, uint64_t* digest_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nvars >= 1 && nvars <= kMaxVars, "nvars = %d: 1 to %d vectors", nvars, kMaxVars);
    ARMON_REQUIRE(vars && digest_dev && (dense_dev || !UNPACK), "NULL argument");
    state_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
    if (rc == ARMON_OK) rc = win::check_global_index(global_first, global_nx, wnx);
    if (rc != ARMON_OK) return rc;
    uintptr_t mis = (uintptr_t)dense_dev;
    for (int q = 0; q < kMaxVars; q++) {
        a.vars[q] = q < nvars ? vars[q] : nullptr;
        ARMON_REQUIRE(q >= nvars || vars[q], "NULL array");
        mis |= (uintptr_t)a.vars[q];
    }
    a.dense = dense_dev;
    a.g0 = (uint64_t)global_first; a.NX = (uint64_t)global_nx;
    a.nvars = nvars;
    // rows of the dense side start wnx apart: it only has 16-B rows when wnx is a multiple of V
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n) && (!dense_dev || wnx % wide<T>::n == 0);
    const int64_t blocks = win::walk_blocks(a.w, (int64_t)ctx->n_cu * 8);
    rc = ensure_partials(ctx, (size_t)kMaxVars * blocks);      // (doubles and 64-bit words have the same size)
    if (rc != ARMON_OK) return rc;
    a.partials = reinterpret_cast<unsigned long long*>(ctx->partials);
    const dim3 grid((unsigned)blocks), block(kBlock);
    if (wide_ok) hipLaunchKernelGGL((k_state_move<T, true, UNPACK>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_state_move<T, false, UNPACK>), grid, block, 0, ctx->stream, a);
    rc = check_launch(UNPACK ? "state_unpack" : "state_pack");
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_digest_fold, dim3((unsigned)nvars), block, 0, ctx->stream, a.partials, (int)blocks,
                       reinterpret_cast<unsigned long long*>(digest_dev));
    return check_launch("digest_fold");
}

template <typename T>
int state_pack_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars, const T* const* vars,
                    int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first, int64_t global_nx,
                    T* dense_dev, uint64_t* digest_dev)
{
    return state_move_impl<T, false>(ctx, row_length, nghost, nx, ny, nvars, const_cast<T* const*>(vars), col0, row0, wnx, wny,
                                     global_first, global_nx, dense_dev, digest_dev);
}

template <typename T>
int state_unpack_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars, T* const* vars,
                      int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first, int64_t global_nx,
                      const T* dense_dev, uint64_t* digest_dev)
{
    return state_move_impl<T, true>(ctx, row_length, nghost, nx, ny, nvars, vars, col0, row0, wnx, wny, global_first, global_nx,
                                    const_cast<T*>(dense_dev), digest_dev);
}

}  // namespace

#define ARMON_EXPORT(name, impl, PARAMS, ARGS)                                            \
    int armon_hip_##name(PARAMS(double)) { return impl<double> ARGS; }                    \
    int armon_hip_##name##_f32(PARAMS(float)) { return impl<float> ARGS; }

extern "C" {

#define P_SP(T) armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars, const T* const* vars, \
                int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first, int64_t global_nx,            \
                T* dense_dev, uint64_t* digest_dev
ARMON_EXPORT(state_pack, state_pack_impl, P_SP,
             (ctx, row_length, nghost, nx, ny, nvars, vars, col0, row0, wnx, wny, global_first, global_nx, dense_dev, digest_dev))

#define P_SU(T) armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars, T* const* vars, \
                int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first, int64_t global_nx,      \
                const T* dense_dev, uint64_t* digest_dev
ARMON_EXPORT(state_unpack, state_unpack_impl, P_SU,
             (ctx, row_length, nghost, nx, ny, nvars, vars, col0, row0, wnx, wny, global_first, global_nx, dense_dev, digest_dev))

}  // extern "C"
