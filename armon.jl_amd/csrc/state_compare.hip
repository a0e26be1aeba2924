// state_compare.hip — compare a window of real cells of the block's vectors with a dense reference, on the device, and reduce
// the difference to one 64-byte record per variable (armon_state_diff, include/armon_hip.h). Nothing is moved: both sides are
// read once, and only the records (and, on request, a count per window row) are written.
//
// No reference counterpart: the reference compares text files on the host (ref src/io.jl:113-227); the per-cell rule is its
// isapprox (ref test/reference_data/reference_functions.jl:54-57) with two NaNs counted as equal, as io.compare_host does.
//
// PER CELL, a = our value, b = the reference's, all arithmetic in T, one IEEE operation per operation written:
//     same = a == b, or both are NaN                       (then d = 0 and the relative difference is 0)
//     d    = |a - b|,  m = max(|a|, |b|),  rel = d / m     (otherwise; a NaN in d or rel becomes the canonical quiet NaN)
//     within tolerance = same, or both finite and d <= max(atol, rtol m)
// A cell counts for n_bits when the bit patterns differ (-0.0 against +0.0 does, and is within tolerance).
//
// MERGE: counts add, first_out is a minimum, (value, position) pairs take the larger bit pattern and on equal patterns the
// smaller global index (red::op_pair_max); the position of a value of 0 is UINT64_MAX. Differences are non-negative, so the
// unsigned order of their bit patterns is their numerical order with NaN on top. All four operations are associative and
// commutative: the record is a function of the two states and the tolerance only — not of the launch shape, the band split,
// the alignment path, the ghost width or the decomposition. Each call MERGES into diff_dev (state_diff_reset writes the
// neutral element), so the bands of a file accumulate on the device with no host synchronisation.
//
// Launch: the window walk of window.hpp over the vectors and the dense buffer (16-B rows there need wnx to be a multiple of
// V), 8 workgroups per CU shared by the variables; both loads of an item are issued before its first comparison. The
// variable is the grid's y index: a workgroup keeps the seven accumulators of ONE variable. Reduction as in reduce.hpp:
// lane -> wave shuffle -> LDS over the waves -> one partial per workgroup -> fold kernel, one workgroup per variable.
// The only atomic is the integer add into row_out (order-independent), issued by one lane per item that has a cell out of
// tolerance. The partials live in the context's reduction scratch (ensure_partials: one synchronisation to grow, refused
// inside a capture or while a graph of the context is alive).
#include "window.hpp"

#include <cmath>

using namespace armon;

#ifndef ARMON_CMP_NT
#define ARMON_CMP_NT 1
#endif

namespace {

constexpr int kMaxVars = 8;
constexpr int kWords = 7;                   // per partial: n_bits, n_out, first_out, max_abs, max_abs_at, max_rel, max_rel_at

typedef unsigned long long u64;
using win::bits_of;
using win::finite;
using win::kNone;
using win::kWave;
using win::kWavesPerBlock;
using win::load_cells;
using win::wide;

__device__ __forceinline__ double quotient(double n, double d) { return n / d; }
__device__ __forceinline__ float quotient(float n, float d) { return __fdiv_rn(n, d); }      // correctly rounded whatever the build's default
__device__ __forceinline__ u64 canonical_nan(double) { return 0x7ff8000000000000ull; }
__device__ __forceinline__ u64 canonical_nan(float) { return 0x7fc00000ull; }

template <typename T>
struct cmp_args {
    const T* vars[kMaxVars];
    const T* ref;                   // [nvars][wny][wnx]
    u64* partials;                  // [nvars][gridDim.x][kWords]
    unsigned* row_out;              // [nvars][wny] or NULL
    win::window w;
    u64 g0, NX;                     // global index of the window's first cell, global row length
    T rtol, atol;
};

struct cmp_acc {
    u64 n_bits = 0, n_out = 0, first_out = kNone;
    red::upair abs_{0, kNone}, rel{0, kNone};
};

// one cell into the lane's accumulators → whether it is out of tolerance
template <typename T>
__device__ __forceinline__ bool compare_cell(T a, T b, u64 g, T rtol, T atol, cmp_acc& acc)
{
    const bool both_nan = a != a && b != b, same = a == b || both_nan;
    acc.n_bits += bits_of(a) != bits_of(b);
    if (same) return false;                                     // d = rel = 0: nothing enters a maximum
    const T fa = fabs(a), fb = fabs(b);
    const T d = fabs(a - b), m = fa > fb ? fa : fb;
    const T rel = quotient(d, m);
    const T tol = rtol * m;
    const bool within = finite(a) && finite(b) && d <= (atol > tol ? atol : tol);
    const u64 db = d != d ? canonical_nan(d) : bits_of(d), rb = rel != rel ? canonical_nan(rel) : bits_of(rel);
    if (db != 0) acc.abs_ = red::op_pair_max::f(acc.abs_, red::upair{db, g});
    if (rb != 0) acc.rel = red::op_pair_max::f(acc.rel, red::upair{rb, g});
    if (!within) {
        acc.n_out += 1;
        acc.first_out = g < acc.first_out ? g : acc.first_out;
    }
    return !within;
}

// One (row, span) item per wave and turn; blockIdx.y = the variable.
template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock, 8)        // 8 waves per SIMD = the 8 workgroups per CU of the grid, all resident at once
k_state_compare(cmp_args<T> a)
{
    constexpr int V = wide<T>::n;
    __shared__ u64 lds[kWavesPerBlock];
    __shared__ red::upair lds_pair[kWavesPerBlock];
    const int lane = threadIdx.x & (kWave - 1), q = blockIdx.y;
    const T* __restrict__ ours = a.vars[q] + a.w.first;
    const T* __restrict__ ref = a.ref + (int64_t)q * a.w.wny * a.w.wnx;
    unsigned* row_out = a.row_out ? a.row_out + (int64_t)q * a.w.wny : nullptr;
    cmp_acc acc;
    win::walk<V>(a.w, [&](int64_t r, int64_t x, int64_t left) {
        unsigned out = 0;
        if (left > 0) {
            T fa[V], fb[V];                                         // both sources' loads are issued before the first comparison
            load_cells<T, WIDE, ARMON_CMP_NT>(ours + r * a.w.pitch + x, left >= V, left, fa);
            load_cells<T, WIDE, ARMON_CMP_NT>(ref + r * a.w.wnx + x, left >= V, left, fb);
            const u64 g = a.g0 + (u64)r * a.NX + (u64)x;
#pragma unroll
            for (int c = 0; c < V; c++)
                if (c < left) out += compare_cell(fa[c], fb[c], g + (u64)c, a.rtol, a.atol, acc);
        }
        if (row_out && __ballot(out != 0) != 0) {                   // wave-uniform; rare
            out = red::wave_reduce<red::op_sum>(out);
            if (lane == 0) atomicAdd(row_out + r, out);
        }
    });
    u64* part = a.partials + ((int64_t)q * gridDim.x + blockIdx.x) * kWords;
    const int tid = (int)threadIdx.x;
    const u64 n_bits = red::block_reduce<red::op_sum, kWavesPerBlock>(acc.n_bits, lds, tid);
    const u64 n_out = red::block_reduce<red::op_sum, kWavesPerBlock>(acc.n_out, lds, tid);
    const u64 first_out = red::block_reduce<red::op_umin, kWavesPerBlock>(acc.first_out, lds, tid);
    const red::upair mabs = red::block_reduce<red::op_pair_max, kWavesPerBlock>(acc.abs_, lds_pair, tid);
    const red::upair mrel = red::block_reduce<red::op_pair_max, kWavesPerBlock>(acc.rel, lds_pair, tid);
    if (tid == 0) {
        part[0] = n_bits; part[1] = n_out; part[2] = first_out;
        part[3] = mabs.v; part[4] = mabs.at; part[5] = mrel.v; part[6] = mrel.at;
    }
}

// one workgroup per variable: diff[q] = merge(diff[q], its partials), n_cells += cells
__global__ void __launch_bounds__(kBlock)
k_diff_fold(const u64* __restrict__ partials, int n, u64 cells, armon_state_diff* __restrict__ diff)
{
    __shared__ u64 lds[kWavesPerBlock];
    __shared__ red::upair lds_pair[kWavesPerBlock];
    const int q = blockIdx.x, tid = (int)threadIdx.x;
    u64 n_bits = 0, n_out = 0, first_out = kNone;
    red::upair mabs{0, kNone}, mrel{0, kNone};
    for (int i = tid; i < n; i += kBlock) {
        const u64* p = partials + ((int64_t)q * n + i) * kWords;
        n_bits += p[0]; n_out += p[1];
        first_out = p[2] < first_out ? p[2] : first_out;
        mabs = red::op_pair_max::f(mabs, red::upair{p[3], p[4]});
        mrel = red::op_pair_max::f(mrel, red::upair{p[5], p[6]});
    }
    n_bits = red::block_reduce<red::op_sum, kWavesPerBlock>(n_bits, lds, tid);
    n_out = red::block_reduce<red::op_sum, kWavesPerBlock>(n_out, lds, tid);
    first_out = red::block_reduce<red::op_umin, kWavesPerBlock>(first_out, lds, tid);
    mabs = red::block_reduce<red::op_pair_max, kWavesPerBlock>(mabs, lds_pair, tid);
    mrel = red::block_reduce<red::op_pair_max, kWavesPerBlock>(mrel, lds_pair, tid);
    if (tid == 0) {
        armon_state_diff d = diff[q];
        d.n_cells += cells; d.n_bits += n_bits; d.n_out += n_out;
        d.first_out = first_out < d.first_out ? first_out : d.first_out;
        const red::upair A = red::op_pair_max::f(red::upair{d.max_abs, d.max_abs_at}, mabs);
        const red::upair R = red::op_pair_max::f(red::upair{d.max_rel, d.max_rel_at}, mrel);
        d.max_abs = A.v; d.max_abs_at = A.at; d.max_rel = R.v; d.max_rel_at = R.at;
        diff[q] = d;
    }
}

__global__ void k_diff_reset(int nvars, armon_state_diff* __restrict__ diff)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nvars) diff[q] = armon_state_diff{0, 0, 0, kNone, 0, kNone, 0, kNone};
}

template <typename T>
int state_compare_impl(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars, const T* const* vars,
                       int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first, int64_t global_nx,
                       const T* ref_dense_dev, double rtol, double atol, armon_state_diff* diff_dev, uint32_t* row_out_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nvars >= 1 && nvars <= kMaxVars, "nvars = %d: 1 to %d vectors", nvars, kMaxVars);
    ARMON_REQUIRE(vars && ref_dense_dev && diff_dev, "NULL argument");
    ARMON_REQUIRE(rtol >= 0 && atol >= 0, "invalid tolerance: rtol = %g, atol = %g", rtol, atol);     // (a NaN fails both)
    cmp_args<T> a;
    int rc = win::make_window<T>(row_length, nghost, nx, ny, col0, row0, wnx, wny, a.w);
    if (rc == ARMON_OK) rc = win::check_global_index(global_first, global_nx, wnx);
    if (rc != ARMON_OK) return rc;
    uintptr_t mis = (uintptr_t)ref_dense_dev;
    for (int q = 0; q < kMaxVars; q++) {
        a.vars[q] = q < nvars ? vars[q] : nullptr;
        ARMON_REQUIRE(q >= nvars || vars[q], "NULL array");
        mis |= (uintptr_t)a.vars[q];
    }
    a.ref = ref_dense_dev;
    a.row_out = row_out_dev;
    a.g0 = (uint64_t)global_first; a.NX = (uint64_t)global_nx;
    a.rtol = (T)rtol; a.atol = (T)atol;
    // rows of the dense side start wnx apart: it only has 16-B rows when wnx is a multiple of V
    const bool wide_ok = win::rows_are_16B(a.w, mis, wide<T>::n) && wnx % wide<T>::n == 0;
    // the 8 workgroups per CU are shared by the variables
    const int64_t max_blocks = (int64_t)ctx->n_cu * 8 / nvars;
    const int64_t blocks = win::walk_blocks(a.w, max_blocks < 1 ? 1 : max_blocks);
    rc = ensure_partials(ctx, (size_t)kWords * nvars * blocks);   // (doubles and 64-bit words have the same size)
    if (rc != ARMON_OK) return rc;
    a.partials = reinterpret_cast<u64*>(ctx->partials);
    const dim3 grid((unsigned)blocks, (unsigned)nvars), block(kBlock);
    if (wide_ok) hipLaunchKernelGGL((k_state_compare<T, true>), grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL((k_state_compare<T, false>), grid, block, 0, ctx->stream, a);
    rc = check_launch("state_compare");
    if (rc != ARMON_OK) return rc;
    hipLaunchKernelGGL(k_diff_fold, dim3((unsigned)nvars), block, 0, ctx->stream, a.partials, (int)blocks, (u64)(wnx * wny), diff_dev);
    return check_launch("diff_fold");
}

}  // namespace

extern "C" {

int armon_hip_state_diff_reset(armon_ctx* ctx, int nvars, armon_state_diff* diff_dev)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(nvars >= 1 && nvars <= kMaxVars && diff_dev, "state_diff_reset: nvars = %d (1 to %d), diff_dev = %p", nvars, kMaxVars,
                  (void*)diff_dev);
    hipLaunchKernelGGL(k_diff_reset, dim3(1), dim3(kWave), 0, ctx->stream, nvars, diff_dev);
    return check_launch("state_diff_reset");
}

int armon_hip_state_compare(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
                            const double* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
                            int64_t global_nx, const double* ref_dense_dev, double rtol, double atol, armon_state_diff* diff_dev,
                            uint32_t* row_out_dev)
{
    return state_compare_impl<double>(ctx, row_length, nghost, nx, ny, nvars, vars, col0, row0, wnx, wny, global_first, global_nx,
                                      ref_dense_dev, rtol, atol, diff_dev, row_out_dev);
}

int armon_hip_state_compare_f32(armon_ctx* ctx, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
                                const float* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
                                int64_t global_nx, const float* ref_dense_dev, double rtol, double atol, armon_state_diff* diff_dev,
                                uint32_t* row_out_dev)
{
    return state_compare_impl<float>(ctx, row_length, nghost, nx, ny, nvars, vars, col0, row0, wnx, wny, global_first, global_nx,
                                     ref_dense_dev, rtol, atol, diff_dev, row_out_dev);
}

}  // extern "C"
