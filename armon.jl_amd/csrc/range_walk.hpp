// range_walk.hpp — how a staged kernel walks an armon_range: one thread per cell of a row, rows strided over blockIdx.y
// (launch shape: range_grid of common.hpp). Shared by staged_kernels.hip and init_regions.hip.
#pragma once

#include "common.hpp"

namespace armon {

__device__ __forceinline__ int64_t row_base(const armon_range& r, int64_t j)
{
    return r.col_start + j * r.col_step + r.row_start;
}

// Threads are laid along a row of the range, shifted left so that every wave's row segment starts on a 64-B sector
// of the array (ranges start g or g-w cells into a row: without the shift each 512-B segment straddles one more sector;
// the fused sweeps gained 9-11 % from the same alignment). Grids are sized for row_len + 15 threads.
template <typename T> __device__ __forceinline__ int64_t row_thread(const armon_range& r)
{
    constexpr int64_t per_sector = 64 / sizeof(T);
    return (int64_t)blockIdx.x * blockDim.x + threadIdx.x - ((r.col_start + r.row_start) & (per_sector - 1));
}

#define ARMON_FOR_RANGE(r, i)                                                         \
    const int64_t k_ = row_thread<T>(r);                                               \
    if (k_ >= 0 && k_ < (r).row_len)                                                   \
        for (int64_t j_ = blockIdx.y, i = row_base((r), j_) + k_; j_ < (r).col_len;    \
             j_ += gridDim.y, i = row_base((r), j_) + k_)

}  // namespace armon
