// reduce.hpp — wavefront shuffle + LDS tree reductions shared by the reduction and sweep kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "physics.hpp"

namespace armon {
namespace red {

constexpr int kWave = 64;
constexpr unsigned long long kNone = ~0ull;      // the all-ones word: no position, no key

struct op_min { template <typename T> __device__ static T id() { return T(INFINITY); } template <typename T> __device__ static T f(T a, T b) { return phys::mn(a, b); } };
// maximum of NON-NEGATIVE values, NaN sticks (phys::amax): only the dt/CFL reductions use it, and a NaN in one cell has to
// reach the host's validity check (ref src/solver_state.jl:123-124)
struct op_max { template <typename T> __device__ static T id() { return T(0.); } template <typename T> __device__ static T f(T a, T b) { return phys::amax(a, b); } };
struct op_sum { template <typename T> __device__ static T id() { return T(0.); } template <typename T> __device__ static T f(T a, T b) { return a + b; } };
// minimum of unsigned integers (positions; the all-ones word = none)
struct op_umin { template <typename T> __device__ static T id() { return ~T(0); } template <typename T> __device__ static T f(T a, T b) { return b < a ? b : a; } };
struct op_umax { template <typename T> __device__ static T id() { return T(0); } template <typename T> __device__ static T f(T a, T b) { return b > a ? b : a; } };
// the unsigned word whose order is the numerical order of the doubles (-0.0 below +0.0)
__device__ __forceinline__ unsigned long long order_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
// (value, position) pairs of unsigned 64-bit words: the larger value wins, on equal values the smaller position. Associative
// and commutative; the neutral element is (0, all ones), which is also what a value of 0 carries as its position.
struct upair { unsigned long long v, at; };
struct op_pair_max {
    template <typename T> __device__ static T id() { return T{0ull, ~0ull}; }
    template <typename T> __device__ static T f(T a, T b) { return (b.v > a.v || (b.v == a.v && b.at < a.at)) ? b : a; }
};

// (key, position) pairs: the smaller key wins, on equal keys the smaller position; neutral (all ones, all ones)
struct op_pair_min {
    template <typename T> __device__ static T id() { return T{~0ull, ~0ull}; }
    template <typename T> __device__ static T f(T a, T b) { return (b.v < a.v || (b.v == a.v && b.at < a.at)) ? b : a; }
};

template <typename T> __device__ __forceinline__ T shfl_down(T v, int off) { return __shfl_down(v, off, kWave); }
__device__ __forceinline__ upair shfl_down(upair p, int off) { return upair{__shfl_down(p.v, off, kWave), __shfl_down(p.at, off, kWave)}; }

template <typename OP, typename T>
__device__ __forceinline__ T wave_reduce(T v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = OP::f(v, shfl_down(v, off));
    return v;   // valid in lane 0
}

// Reduce across a workgroup of NWAVES waves; result valid in thread 0. `lds` holds NWAVES values.
template <typename OP, int NWAVES, typename T>
__device__ __forceinline__ T block_reduce(T v, T* lds, int tid)
{
    const int lane = tid & (kWave - 1), wave = tid / kWave;
    v = wave_reduce<OP>(v);
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    T r = OP::template id<T>();
    if (tid == 0) {
#pragma unroll
        for (int w = 0; w < NWAVES; w++) r = OP::f(r, lds[w]);
    }
    __syncthreads();
    return r;
}

}  // namespace red
}  // namespace armon
