// periodic.hip — the ghosts of a periodic axis filled from the opposite border of the same block (the rule
// is stated word for word in include/armon_hip.h). The oracle's periodic_ghosts; the reference has no periodic domain.
//
// A copy kernel: no LDS, no arithmetic, plain loads and stores (the cells it reads and the ghosts it writes are what the
// sweep behind it reads next, so neither is marked non-temporal). One launch per call, all variables and both sides, on a
// 1-D grid under 64-bit item numbers (window.hpp's convention): a block of any number of rows is one launch.
//  * Y axis: the items are whole ghost rows, cut into spans of 64 lanes x V columns, span fastest. A lane takes V = 16 B of
//    one row as one access when every row starts on a 16-B boundary in every vector (win::rows_are_16B) and the lane has
//    all V columns, element accesses otherwise; columns past nx are never touched.
//  * X axis: a row has 2·layers ghost cells on two lines nx cells apart. Side and layer run fastest over the lanes, in the
//    order of the addresses (-layers .. -1, then nx .. nx + layers - 1), so a wave covers 64 / (2·layers) consecutive rows
//    and its stores fall on two runs of lines, one per side: 16 lines (fp64, layers = 4, pitch of whole lines) is what the
//    layout allows, against 64 for a lane per row.
#include "common.hpp"
#include "window.hpp"

using namespace armon;

namespace {

constexpr int kMaxVars = 8;

template <typename T>
struct wrap_args {
    T* v[kMaxVars];
    int64_t pitch, nx, ny;
    int nghost, layers, nvars;
};

// v[k] by selects: the pointer table stays in scalar registers
template <typename T>
__device__ __forceinline__ T* pick_var(const wrap_args<T>& a, int k)
{
    T* p = a.v[0];
#pragma unroll
    for (int i = 1; i < kMaxVars; i++) p = k == i ? a.v[i] : p;
    return p;
}

// item = (variable, side·layer, span), span fastest; a wave per item
template <typename T, bool WIDE>
__global__ void __launch_bounds__(kBlock)
k_periodic_y(wrap_args<T> a, int64_t nspan)
{
    constexpr int V = win::wide<T>::n;
    const int lane = threadIdx.x & (win::kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * win::kWavesPerBlock + threadIdx.x / win::kWave;
    const int64_t nwaves = (int64_t)gridDim.x * win::kWavesPerBlock;
    const int64_t rows = 2 * (int64_t)a.layers;
    const int64_t items = (int64_t)a.nvars * rows * nspan;
    for (int64_t item = wave; item < items; item += nwaves) {
        const int64_t sp = item % nspan, rest = item / nspan;
        const int s = (int)(rest % rows), k = (int)(rest / rows);
        // ghost row -1-l takes real row ny-1-l; ghost row ny+l takes real row l
        const int64_t l = s < a.layers ? s : s - a.layers;
        const int64_t dst_row = s < a.layers ? -1 - l : a.ny + l;
        const int64_t src_row = s < a.layers ? a.ny - 1 - l : l;
        const int64_t x = (sp * win::kWave + lane) * V, left = a.nx - x;
        if (left <= 0) continue;
        T* p = pick_var(a, k);
        const T* src = p + (src_row + a.nghost) * a.pitch + a.nghost + x;
        T* dst = p + (dst_row + a.nghost) * a.pitch + a.nghost + x;
        T f[V];
        win::load_cells<T, WIDE, false>(src, left >= V, left, f);
        win::store_cells<T, WIDE>(dst, left >= V, left, f);
    }
}

// item = (variable, row, side·layer), side·layer fastest; a lane per item
template <typename T>
__global__ void __launch_bounds__(kBlock)
k_periodic_x(wrap_args<T> a)
{
    const int64_t cells = 2 * (int64_t)a.layers;
    const int64_t items = (int64_t)a.nvars * a.ny * cells;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t item = (int64_t)blockIdx.x * kBlock + threadIdx.x; item < items; item += step) {
        const int s = (int)(item % cells);
        const int64_t rest = item / cells, y = rest % a.ny;
        const int k = (int)(rest / a.ny);
        // ghost -1-l takes real cell nx-1-l; ghost nx+l takes real cell l. Lanes in the order of the addresses.
        const int64_t l = s < a.layers ? a.layers - 1 - s : s - a.layers;
        const int64_t dst_col = s < a.layers ? -1 - l : a.nx + l;
        const int64_t src_col = s < a.layers ? a.nx - 1 - l : l;
        T* row = pick_var(a, k) + (y + a.nghost) * a.pitch + a.nghost;
        row[dst_col] = row[src_col];
    }
}

template <typename T>
int periodic_impl(armon_ctx* ctx, int axis, int64_t row_length, int nghost, int layers, int64_t nx, int64_t ny, int nvars,
                  T* const* vars)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(axis == 0 || axis == 1, "unknown axis %d: 0 (x) or 1 (y)", axis);
    ARMON_REQUIRE(nvars >= 1 && nvars <= kMaxVars, "nvars = %d is outside 1..%d", nvars, kMaxVars);
    ARMON_REQUIRE(vars != nullptr, "vars is NULL");
    for (int k = 0; k < nvars; k++) ARMON_REQUIRE(vars[k] != nullptr, "vars[%d] is NULL", k);
    ARMON_REQUIRE(nghost >= 1 && layers >= 1 && layers <= nghost, "layers = %d is outside 1..nghost = %d", layers, nghost);
    ARMON_REQUIRE(nx >= 1 && ny >= 1 && nx < (1ll << 31) && ny < (1ll << 31), "invalid block: nx = %lld, ny = %lld", (long long)nx,
                  (long long)ny);
    const int64_t n = axis == 0 ? nx : ny;
    ARMON_REQUIRE(n >= layers, "n = %lld real cells along the axis cannot fill layers = %d ghost layers", (long long)n, layers);
    ARMON_REQUIRE(row_length >= nx + 2 * (int64_t)nghost, "row_length = %lld < nx + 2 nghost = %lld", (long long)row_length,
                  (long long)(nx + 2 * (int64_t)nghost));
    wrap_args<T> a;
    uintptr_t mis = 0;
    for (int k = 0; k < kMaxVars; k++) {
        a.v[k] = vars[k < nvars ? k : 0];
        mis |= reinterpret_cast<uintptr_t>(a.v[k]);
    }
    a.pitch = row_length; a.nx = nx; a.ny = ny;
    a.nghost = nghost; a.layers = layers; a.nvars = nvars;
    const int64_t max_blocks = (int64_t)ctx->n_cu * 8;
    if (axis == 0) {
        const int64_t items = (int64_t)nvars * ny * 2 * layers;
        const int64_t blocks = (items + kBlock - 1) / kBlock;
        const unsigned grid = (unsigned)(blocks < max_blocks ? blocks : max_blocks);
        hipLaunchKernelGGL((k_periodic_x<T>), dim3(grid), dim3(kBlock), 0, ctx->stream, a);
        return check_launch("periodic_ghosts (x)");
    }
    win::window w;
    const int rc = win::make_window<T>(row_length, nghost, nx, ny, 0, 0, nx, ny, w);
    if (rc != ARMON_OK) return rc;
    const int64_t items = (int64_t)nvars * 2 * layers * w.nspan;
    const int64_t blocks = (items + win::kWavesPerBlock - 1) / win::kWavesPerBlock;
    const unsigned grid = (unsigned)(blocks < max_blocks ? blocks : max_blocks);
    if (win::rows_are_16B(w, mis, win::wide<T>::n))
        hipLaunchKernelGGL((k_periodic_y<T, true>), dim3(grid), dim3(kBlock), 0, ctx->stream, a, w.nspan);
    else
        hipLaunchKernelGGL((k_periodic_y<T, false>), dim3(grid), dim3(kBlock), 0, ctx->stream, a, w.nspan);
    return check_launch("periodic_ghosts (y)");
}

}  // namespace

extern "C" {

int armon_hip_periodic_ghosts(armon_ctx* ctx, int axis, int64_t row_length, int nghost, int layers, int64_t nx, int64_t ny,
                              int nvars, double* const* vars)
{
    return periodic_impl<double>(ctx, axis, row_length, nghost, layers, nx, ny, nvars, vars);
}

int armon_hip_periodic_ghosts_f32(armon_ctx* ctx, int axis, int64_t row_length, int nghost, int layers, int64_t nx, int64_t ny,
                                  int nvars, float* const* vars)
{
    return periodic_impl<float>(ctx, axis, row_length, nghost, layers, nx, ny, nvars, vars);
}

}  // extern "C"
