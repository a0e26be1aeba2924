// lane_shift.hpp — a value of the neighbouring lane through a DPP wavefront shift (v_mov_b32 wave_shr:1 / wave_shl:1,
// two per double): no LDS, no barrier. Used by the spatial form of the fused X sweep (sweep_spatial.hpp) and by the
// staged kernels that evaluate a stencil along the contiguous axis (staged_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace armon {
namespace fused {

// value of the previous lane (cell i-1 for K = 1). Lane 0 has no source and reads 0 (bound_ctrl): it
// is a halo lane whose results are discarded, and not keeping its own value saves a register copy per shift.
// ROW = 0: the 64 lanes of the wave are one strip (wave_shr:1 / wave_shl:1); ROW = 1: four independent strips of 16
// lanes each (row_shr:1 / row_shl:1; lanes 0 and 15 of every row read 0) — the form of the narrow boundary strips.
template <int ROW = 0>
__device__ __forceinline__ double from_prev_lane(double x)
{
    constexpr int ctrl = ROW ? 0x111 : 0x138;                          // row_shr:1 : wave_shr:1
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, ctrl, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, ctrl, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int ROW = 0>
__device__ __forceinline__ float from_prev_lane(float x)
{
    constexpr int ctrl = ROW ? 0x111 : 0x138;
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, true));
}

// value of the next lane; lane 63 (lane 15 of a row) reads 0
template <int ROW = 0>
__device__ __forceinline__ double from_next_lane(double x)
{
    constexpr int ctrl = ROW ? 0x101 : 0x130;                          // row_shl:1 : wave_shl:1
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, ctrl, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, ctrl, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int ROW = 0>
__device__ __forceinline__ float from_next_lane(float x)
{
    constexpr int ctrl = ROW ? 0x101 : 0x130;
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, true));
}

// Per-lane strip of K consecutive cells with access to the cells just outside it.
template <int K, typename T>
struct Strip {
    T v[K];
    __device__ __forceinline__ T& operator[](int k) { return v[k]; }
    __device__ __forceinline__ T operator[](int k) const { return v[k]; }
};

template <int K, typename T>
struct Shifted {      // v[k-1] for k = 0..K-1 ("left") or v[k+1] ("right")
    T v[K];
    __device__ __forceinline__ T operator[](int k) const { return v[k]; }
};

template <int ROW, int K, typename T>
__device__ __forceinline__ Shifted<K, T> left_of(const Strip<K, T>& s)
{
    Shifted<K, T> r;
    r.v[0] = from_prev_lane<ROW>(s.v[K - 1]);
#pragma unroll
    for (int k = 1; k < K; k++) r.v[k] = s.v[k - 1];
    return r;
}

template <int ROW, int K, typename T>
__device__ __forceinline__ Shifted<K, T> right_of(const Strip<K, T>& s)
{
    Shifted<K, T> r;
    r.v[K - 1] = from_next_lane<ROW>(s.v[0]);
#pragma unroll
    for (int k = 0; k < K - 1; k++) r.v[k] = s.v[k + 1];
    return r;
}

}  // namespace fused
}  // namespace armon
