// arith_probe.hip — test infrastructure, not part of the product library: each entry point applies ONE arithmetic primitive of
// the hot path elementwise to device arrays, so that tests/test_gpu_arith_primitives.py can drive it operand by operand.
// Built by armon.jl_amd/build.py into libarmon_arith_probe.so with the product's own flags (-ffp-contract=off included):
// what is tested is what the sweeps compile.
//
//   int arith_probe_<primitive>(const T* a, const T* b, T* out, size_t n)      out[i] = a[i] / b[i]   (quotients)
//   int arith_probe_<primitive>(const T* x, T* out, size_t n)                  out[i] = f(x[i])       (roots, reciprocals)
//
// All pointers are device memory of n elements. The float2v forms take n floats, n even, as n / 2 pairs. Every entry point
// synchronises the device before it launches and before it returns, and returns the HIP status (0 = success).
#include "../../armon.jl_amd/csrc/sweep_stages.hpp"

using namespace armon;
using fused::fast::float2v;

namespace {

constexpr int kBlock = 256;

template <class F, typename T>
__global__ void __launch_bounds__(kBlock) k_binary(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) out[i] = F::f(a[i], b[i]);
}

template <class F, typename T>
__global__ void __launch_bounds__(kBlock) k_unary(const T* __restrict__ x, T* __restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock) out[i] = F::f(x[i]);
}

// one lane, one float2v: elements 2 i and 2 i + 1
template <class F>
__global__ void __launch_bounds__(kBlock) k_pair(const float* __restrict__ x, float* __restrict__ out, size_t pairs)
{
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < pairs; i += (size_t)gridDim.x * kBlock) {
        const float2v r = F::f(float2v{x[2 * i], x[2 * i + 1]});
        out[2 * i] = r.x;
        out[2 * i + 1] = r.y;
    }
}

unsigned grid_of(size_t n)
{
    const size_t blocks = (n + kBlock - 1) / kBlock;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

template <class Launch> int run(Launch launch)
{
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    launch();
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

}  // namespace

#define PROBE_API extern "C" __attribute__((visibility("default")))

#define PROBE_BINARY(name, T, expr)                                                                                    \
    namespace { struct F_##name { static __device__ __forceinline__ T f(T a, T b) { return expr; } }; }               \
    PROBE_API int arith_probe_##name(const T* a, const T* b, T* out, size_t n)                                         \
    {                                                                                                                  \
        return run([&] { hipLaunchKernelGGL((k_binary<F_##name, T>), dim3(grid_of(n)), dim3(kBlock), 0, 0, a, b, out, n); }); \
    }

#define PROBE_UNARY(name, T, expr)                                                                                     \
    namespace { struct F_##name { static __device__ __forceinline__ T f(T x) { return expr; } }; }                    \
    PROBE_API int arith_probe_##name(const T* x, T* out, size_t n)                                                     \
    {                                                                                                                  \
        return run([&] { hipLaunchKernelGGL((k_unary<F_##name, T>), dim3(grid_of(n)), dim3(kBlock), 0, 0, x, out, n); }); \
    }

#define PROBE_PAIR(name, expr)                                                                                         \
    namespace { struct F_##name { static __device__ __forceinline__ float2v f(float2v x) { return expr; } }; }        \
    PROBE_API int arith_probe_##name(const float* x, float* out, size_t n)                                             \
    {                                                                                                                  \
        if (n % 2) return (int)hipErrorInvalidValue;                                                                   \
        return run([&] { hipLaunchKernelGGL((k_pair<F_##name>), dim3(grid_of(n / 2)), dim3(kBlock), 0, 0, x, out, n / 2); }); \
    }

// exact flavour (csrc/physics.hpp)
PROBE_BINARY(quo_f64, double, xct::Den<double>(b).quo(a))
PROBE_BINARY(quo_t_f64, double, xct::Den<double>(b).quo_t(a))
PROBE_BINARY(twice_quo_f64, double, xct::Den<double>(b).twice().quo(a))              // a / (2 b)
PROBE_BINARY(quo_f32, float, xct::Den<float>(b).quo(a))
PROBE_BINARY(quo_t_f32, float, xct::Den<float>(b).quo_t(a))
PROBE_BINARY(twice_quo_f32, float, xct::Den<float>(b).twice().quo(a))
PROBE_UNARY(xct_sqrt_f64, double, xct::sqrt_(x))

// tuned flavour (csrc/sweep_stages.hpp)
PROBE_UNARY(fast_rcp_f64, double, fused::fast::rcp(x))
PROBE_UNARY(fast_rcp1_f64, double, fused::fast::rcp1(x))
PROBE_UNARY(fast_sqrt_f64, double, fused::fast::sqrt_(x))
PROBE_UNARY(fast_rcp_f32, float, fused::fast::rcp(x))
PROBE_UNARY(fast_rcp1_f32, float, fused::fast::rcp1(x))
PROBE_UNARY(fast_sqrt_f32, float, fused::fast::sqrt_(x))
PROBE_PAIR(fast_rcp_f32x2, fused::fast::rcp(x))
PROBE_PAIR(fast_rcp1_f32x2, fused::fast::rcp1(x))
PROBE_PAIR(fast_sqrt_f32x2, fused::fast::sqrt_(x))
