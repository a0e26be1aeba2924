// window.hpp — the window walk of the in-situ kernels (coarsen, checkpoint, state_compare, profile, analytic, history,
// derive), stated once (DESIGN, "The window walk"). A window is the real cells [col0, col0 + wnx) x [row0, row0 + wny) of a
// block. Lanes run along x: a lane takes V = 16 B of columns of one row, as ONE 16-B access when every row of the window
// starts on a 16-B boundary in every vector (rows_are_16B) and the lane has all V columns, element accesses by the same
// lanes otherwise; columns past the window are never touched. A row is cut into spans of 64 lanes x V columns; the
// (row, span) items, span fastest, are dealt a wave at a time to a 1-D grid capped per CU (walk_blocks), under 64-bit item
// numbers: a window may have any number of rows. Sources are read once, with non-temporal loads.
#pragma once

#include "common.hpp"
#include "reduce.hpp"

namespace armon {
namespace win {

using red::kNone;
using red::kWave;
constexpr int kWavesPerBlock = kBlock / kWave;

template <typename T> struct wide;
template <> struct wide<double> { static constexpr int n = 2; typedef double type __attribute__((ext_vector_type(2))); };
template <> struct wide<float> { static constexpr int n = 4; typedef float type __attribute__((ext_vector_type(4))); };

__device__ __forceinline__ unsigned long long bits_of(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned long long bits_of(float v) { return (unsigned long long)__float_as_uint(v); }
__device__ __forceinline__ bool finite(double v) { return (bits_of(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
__device__ __forceinline__ bool finite(float v) { return (bits_of(v) & 0x7f800000ull) != 0x7f800000ull; }

// f[c] by selects: the array stays in registers under a loop that is not unrolled
template <int V, typename T>
__device__ __forceinline__ T pick(const T f[V], int c)
{
    T r = f[0];
#pragma unroll
    for (int i = 1; i < V; i++) r = c == i ? f[i] : r;
    return r;
}

// V cells of a row from `src`: one 16-B load when WIDE and the lane has all V of them, element loads otherwise (a cell the
// lane does not have is 0). NT: non-temporal, for a source that is read once.
template <typename T, bool WIDE, bool NT = true>
__device__ __forceinline__ void load_cells(const T* __restrict__ src, bool whole, int64_t left, T f[wide<T>::n])
{
    constexpr int V = wide<T>::n;
    typedef typename wide<T>::type VT;
    if (WIDE && whole) {
        const VT* q = reinterpret_cast<const VT*>(src);
        const VT w = NT ? __builtin_nontemporal_load(q) : *q;
#pragma unroll
        for (int c = 0; c < V; c++) f[c] = w[c];
    } else {
#pragma unroll
        for (int c = 0; c < V; c++) f[c] = c < left ? (NT ? __builtin_nontemporal_load(src + c) : src[c]) : T(0.);
    }
}

template <typename T, bool WIDE>
__device__ __forceinline__ void store_cells(T* __restrict__ dst, bool whole, int64_t left, const T f[wide<T>::n])
{
    constexpr int V = wide<T>::n;
    typedef typename wide<T>::type VT;
    if (WIDE && whole) {
        VT w;
#pragma unroll
        for (int c = 0; c < V; c++) w[c] = f[c];
        *reinterpret_cast<VT*>(dst) = w;
    } else {
#pragma unroll
        for (int c = 0; c < V; c++)
            if (c < left) dst[c] = f[c];
    }
}

struct window {
    int64_t pitch, first;           // row pitch of the vectors; index of the window's first cell in them
    int64_t wnx, wny, nspan;        // columns, rows; spans of 64 lanes x V columns per row
};

// the shared argument checks (none looks at the context), then the window
template <typename T>
inline int make_window(int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t col0, int64_t row0, int64_t wnx, int64_t wny,
                       window& w)
{
    ARMON_REQUIRE(nx >= 1 && ny >= 1 && nghost >= 0, "invalid block: nx = %lld, ny = %lld, nghost = %d", (long long)nx, (long long)ny, nghost);
    ARMON_REQUIRE(nx < (1ll << 31) && ny < (1ll << 31), "block too large: nx = %lld, ny = %lld", (long long)nx, (long long)ny);
    ARMON_REQUIRE(row_length >= nx + 2 * (int64_t)nghost, "the real cells leave the block: row_length = %lld < nx + 2 nghost = %lld",
                  (long long)row_length, (long long)(nx + 2 * (int64_t)nghost));
    ARMON_REQUIRE(col0 >= 0 && row0 >= 0 && wnx >= 1 && wny >= 1 && wnx <= nx - col0 && wny <= ny - row0,
                  "the window [%lld, %lld) x [%lld, %lld) leaves the real domain %lld x %lld", (long long)col0,
                  (long long)(col0 + wnx), (long long)row0, (long long)(row0 + wny), (long long)nx, (long long)ny);
    constexpr int V = wide<T>::n;
    w.pitch = row_length;
    w.first = ((int64_t)nghost + row0) * row_length + nghost + col0;
    w.wnx = wnx; w.wny = wny;
    w.nspan = (wnx + kWave * V - 1) / (kWave * V);
    return ARMON_OK;
}

// the global position of the window's first cell, as (column, row) ...
inline int check_global_cell(int64_t global_col0, int64_t global_row0)
{
    ARMON_REQUIRE(global_col0 >= 0 && global_row0 >= 0 && global_col0 < (1ll << 40) && global_row0 < (1ll << 40),
                  "invalid global position: (%lld, %lld)", (long long)global_col0, (long long)global_row0);
    return ARMON_OK;
}
// ... or as (index, global row length)
inline int check_global_index(int64_t global_first, int64_t global_nx, int64_t wnx)
{
    ARMON_REQUIRE(global_first >= 0 && global_nx >= wnx, "invalid global position: first = %lld, row length = %lld",
                  (long long)global_first, (long long)global_nx);
    return ARMON_OK;
}

// every row of the window starts on a 16-B boundary; mis = the vectors' base addresses or-ed together, V = wide<T>::n
inline bool rows_are_16B(const window& w, uintptr_t mis, int V) { return (mis & 15) == 0 && w.first % V == 0 && w.pitch % V == 0; }

// the grid of a walk: a wave per (row, span) item, at most max_blocks workgroups
inline int64_t walk_blocks(const window& w, int64_t max_blocks)
{
    const int64_t blocks = (w.wny * w.nspan + kWavesPerBlock - 1) / kWavesPerBlock;
    return blocks < max_blocks ? blocks : max_blocks;
}

// the lane's first column of span sp, and how many columns the window has from there on (<= 0: none)
struct lane_cols { int64_t x, left; };
template <int V>
__device__ __forceinline__ lane_cols lane_column(const window& w, int64_t sp, int lane)
{
    const int64_t x = (sp * kWave + lane) * V;
    return lane_cols{x, w.wnx - x};
}

// The walk: body(r, x, left) for the lane's V columns from x of row r, `left` of them inside the window. The body is called
// wave-uniformly (it may shuffle): a lane past the window's last column gets left <= 0 and has to touch nothing.
template <int V, typename F>
__device__ __forceinline__ void walk(const window& w, F&& body)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave, nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const int64_t units = w.wny * w.nspan;
    for (int64_t unit = wave; unit < units; unit += nwaves) {
        const int64_t sp = unit % w.nspan, r = unit / w.nspan;
        const lane_cols c = lane_column<V>(w, sp, lane);
        body(r, c.x, c.left);
    }
}

}  // namespace win
}  // namespace armon
