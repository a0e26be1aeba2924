// placement.hip — armon_hip_tune_placement / armon_hip_choose_placement (fp64 and fp32).
// ---- placement of the 8 streamed vectors -------------------------------------------------------
// The same sweeps run 10-20 % apart depending on where the 4 read and 4 written vectors sit in HBM relative to each
// other, and nothing visible from user space predicts it: time `tries` assignments of the 8 roles to the vectors of
// `pool` (the first one = pool[0..7] as given) with the caller's own X and Y sweeps, as in a cycle (cycle_f64 / cycle_f32 below) — X reads
// roles 0..3 and writes roles 4..7, Y reads 4..7 and writes 0..3 — and report the fastest.
#include "common.hpp"

#include <cstdint>
#include <utility>
#include <vector>

using namespace armon;

namespace {

template <typename real>
__global__ void __launch_bounds__(256) k_fill_uniform(real* __restrict__ p, size_t n, real value)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = value;
}

// What a draw is timed with: the X and the Y sweep of a cycle as the host will run them. fp64: a cycle that satisfies
// armon_hip_sweep_pair's preconditions on vectors that hold its intermediate runs through that call — other pitch of the
// rows between the sweeps, other load policy in the Y march, hence another access pattern to choose a placement for.
struct cycle_f64 {
    size_t bytes;
    int operator()(armon_ctx* ctx, const armon_sweep_desc* x, const armon_sweep_desc* y) const
    {
        const int64_t rows = x->ny + 2 * (int64_t)x->nghost;
        const bool pair = x->axis == ARMON_AXIS_X && y->axis == ARMON_AXIS_Y && x->nx == y->nx && x->ny == y->ny &&
                          x->nghost == y->nghost && x->nx > 0 && x->ny > 0 && x->nghost >= 0 && y->bc_low && y->bc_high &&
                          x->out_hi == 0 && y->out_hi == 0 && !x->p_out && !x->c_out && !x->dt_cfl_out && x->x_kernel == 0 &&
                          (uint64_t)bytes >= (uint64_t)(armon_hip_sweep_pair_pitch(x->nx, x->nghost) * rows) * sizeof(double);
        if (pair) return armon_hip_sweep_pair(ctx, x, y, bytes);
        const int rc = armon_hip_sweep(ctx, x);
        return rc == ARMON_OK ? armon_hip_sweep(ctx, y) : rc;
    }
};
struct cycle_f32 {
    int operator()(armon_ctx* ctx, const armon_sweep_desc_f32* x, const armon_sweep_desc_f32* y) const
    {
        const int rc = armon_hip_sweep_f32(ctx, x);
        return rc == ARMON_OK ? armon_hip_sweep_f32(ctx, y) : rc;
    }
};

// The search both entry points share. `prepare(idx)` readies the pool for the assignment idx[0..7] before it is timed,
// `stop(seen, best_ms)` ends the search early; both return ARMON_OK / false to go on. *tries_done = draws timed.
template <class DESC, class SWEEP, class PREPARE, class STOP>
int placement_search(armon_ctx* ctx, SWEEP sweep, const DESC* x_desc, const DESC* y_desc, void* const* pool, int n_pool,
                     int tries, int* best, double* times_ms, int* tries_done, PREPARE prepare, STOP stop)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define PLACEMENT_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail_hip(e_, #expr); } } while (0)
    PLACEMENT_TRY(hipEventCreate(&e0));
    PLACEMENT_TRY(hipEventCreate(&e1));
    std::vector<int> idx(n_pool);
    std::vector<double> seen;
    double best_ms = 1e300;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    int t = 0;
    for (; t < tries; t++) {
        for (int k = 0; k < n_pool; k++) idx[k] = k;
        if (t > 0)
            for (int k = 0; k < 8; k++) {                         // partial Fisher-Yates: 8 distinct vectors
                rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
                std::swap(idx[k], idx[k + (int)(rng % (uint64_t)(n_pool - k))]);
            }
        int rc = prepare(idx.data());
        if (rc != ARMON_OK) { cleanup(); return rc; }
        DESC dx = *x_desc, dy = *y_desc;
        using ptr_t = decltype(dx.rho_out);
        auto P = [&](int role) { return static_cast<ptr_t>(pool[idx[role]]); };
        dx.rho_in = P(0); dx.u_in = P(1); dx.v_in = P(2); dx.E_in = P(3);
        dx.rho_out = P(4); dx.u_out = P(5); dx.v_out = P(6); dx.E_out = P(7);
        dy.rho_in = P(4); dy.u_in = P(5); dy.v_in = P(6); dy.E_in = P(7);
        dy.rho_out = P(0); dy.u_out = P(1); dy.v_out = P(2); dy.E_out = P(3);
        double ms_min = 1e300;
        for (int rep = 0; rep < 3; rep++) {
            PLACEMENT_TRY(hipEventRecord(e0, ctx->stream));
            rc = sweep(ctx, &dx, &dy);
            if (rc != ARMON_OK) { cleanup(); return rc; }
            PLACEMENT_TRY(hipEventRecord(e1, ctx->stream));
            PLACEMENT_TRY(hipEventSynchronize(e1));
            float ms = 0.f;
            PLACEMENT_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < ms_min) ms_min = ms;
        }
        if (times_ms) times_ms[t] = ms_min;
        seen.push_back(ms_min);
        if (ms_min < best_ms) {
            best_ms = ms_min;
            for (int k = 0; k < 8; k++) best[k] = idx[k];
        }
        if (stop(seen, best_ms)) { t++; break; }
    }
#undef PLACEMENT_TRY
    if (tries_done) *tries_done = t;
    cleanup();
    return ARMON_OK;
}

// A pool whose first four vectors hold a LIVE state: it is parked in four more vectors while roles move around, copied
// into every candidate's input vectors, and left in pool[picks[0..3]].
template <class DESC, class SWEEP>
int tune_placement(armon_ctx* ctx, SWEEP sweep, const DESC* x_desc, const DESC* y_desc, void* const* pool, int n_pool,
                   size_t bytes, int tries, int* picks, double* times_ms)
{
    ARMON_REQUIRE(ctx && x_desc && y_desc && pool && picks, "NULL argument");
    ARMON_REQUIRE(n_pool >= 8 && tries >= 1 && bytes > 0, "need at least 8 vectors and 1 try (n_pool = %d, tries = %d)", n_pool, tries);
    for (int k = 0; k < n_pool; k++) ARMON_REQUIRE(pool[k], "pool[%d] is NULL", k);
    void* master[4] = {nullptr, nullptr, nullptr, nullptr};     // the state is parked here while roles move around
    bool parked = false;              // true once the state is safe in `master`: a failure puts it back in pool[0..3]
    auto cleanup = [&]() {
        if (parked) {
            for (int k = 0; k < 4; k++)
                (void)hipMemcpyAsync(pool[k], master[k], bytes, hipMemcpyDeviceToDevice, ctx->stream);
            (void)hipStreamSynchronize(ctx->stream);
        }
        for (void* m : master)
            if (m) (void)hipFree(m);
    };
#define TUNE_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { cleanup(); return fail_hip(e_, #expr); } } while (0)
    for (int k = 0; k < 4; k++) {
        TUNE_TRY(hipMalloc(&master[k], bytes));
        TUNE_TRY(hipMemcpyAsync(master[k], pool[k], bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    parked = true;
    // (`what`: the call as TUNE_TRY's #expr spelled it when these copies stood in the search loop — the messages callers have seen)
    auto copy_in = [&](const int* idx, const char* what) {
        for (int k = 0; k < 4; k++) {
            hipError_t e = hipMemcpyAsync(pool[idx[k]], master[k], bytes, hipMemcpyDeviceToDevice, ctx->stream);
            if (e != hipSuccess) return fail_hip(e, what);
        }
        return (int)ARMON_OK;
    };
    int best[8] = {};
    int rc = placement_search(ctx, sweep, x_desc, y_desc, pool, n_pool, tries, best, times_ms, nullptr,
                              [&](const int* idx) { return copy_in(idx, "hipMemcpyAsync(pool[idx[k]], master[k], bytes, hipMemcpyDeviceToDevice, ctx->stream)"); },
                              [](const std::vector<double>&, double) { return false; });
    if (rc == ARMON_OK) rc = copy_in(best, "hipMemcpyAsync(pool[best[k]], master[k], bytes, hipMemcpyDeviceToDevice, ctx->stream)");
    if (rc != ARMON_OK) { cleanup(); return rc; }
    TUNE_TRY(hipStreamSynchronize(ctx->stream));
#undef TUNE_TRY
    for (int k = 0; k < 8; k++) picks[k] = best[k];
    parked = false;                   // the state now lives in pool[picks[0..3]]
    cleanup();
    return ARMON_OK;
}

// Same choice for a pool that holds NO state worth keeping (a host calls it BEFORE init_test writes the initial
// condition): nothing is parked or restored, so the only transient memory is the caller's spare vectors. Each
// candidate's four input vectors are filled with a uniform state (the sweeps' instruction stream does not depend on the
// data) and timed like above; after 12 draws the search stops as soon as two of them lie within `tolerance` of the best
// one while a draw at least 7 % slower has been seen as well (the good placements form a plateau), after
// at most `tries` draws.
template <typename real, class DESC, class SWEEP>
int choose_placement(armon_ctx* ctx, SWEEP sweep, const DESC* x_desc, const DESC* y_desc, void* const* pool, int n_pool,
                     size_t bytes, int tries, double tolerance, int* picks, double* times_ms, int* tries_done)
{
    ARMON_REQUIRE(ctx && x_desc && y_desc && pool && picks, "NULL argument");
    ARMON_REQUIRE(n_pool >= 8 && tries >= 1 && bytes >= sizeof(real), "need at least 8 vectors and 1 try (n_pool = %d, tries = %d)", n_pool, tries);
    for (int k = 0; k < n_pool; k++) ARMON_REQUIRE(pool[k], "pool[%d] is NULL", k);
    const size_t n = bytes / sizeof(real);
    const real uniform[4] = {real(1), real(0), real(0), real(2.5)};          // rho, u, v, E: Sod's left state
    auto fill = [&](const int* idx) {
        for (int k = 0; k < 4; k++)
            hipLaunchKernelGGL(k_fill_uniform<real>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                               static_cast<real*>(pool[idx[k]]), n, uniform[k]);
        return (int)ARMON_OK;
    };
    // stop once the plateau of good placements has been hit twice — two draws within `tolerance` of the best —
    // AND a draw at least 7 % slower has been seen too, after 12 draws at least: the X+Y times come in three
    // levels (16384²: ≈5.65 / 6.17 / 6.45 ms) and two equal draws of the middle level must not end the search
    auto plateau = [&](const std::vector<double>& seen, double best_ms) {
        int near = 0;
        double worst = 0;
        for (double v : seen) {
            near += v <= best_ms * (1. + tolerance);
            worst = v > worst ? v : worst;
        }
        return tolerance > 0 && seen.size() >= 12 && near >= 2 && best_ms <= 0.93 * worst;
    };
    int best[8] = {};
    int rc = placement_search(ctx, sweep, x_desc, y_desc, pool, n_pool, tries, best, times_ms, tries_done, fill, plateau);
    if (rc != ARMON_OK) return rc;
    for (int k = 0; k < 8; k++) picks[k] = best[k];
    return ARMON_OK;
}

}  // namespace

extern "C" int armon_hip_tune_placement(armon_ctx* ctx, const armon_sweep_desc* x_desc, const armon_sweep_desc* y_desc,
                                        void* const* pool, int n_pool, size_t bytes, int tries, int* picks, double* times_ms)
{
    return tune_placement(ctx, cycle_f64{bytes}, x_desc, y_desc, pool, n_pool, bytes, tries, picks, times_ms);
}

extern "C" int armon_hip_tune_placement_f32(armon_ctx* ctx, const armon_sweep_desc_f32* x_desc, const armon_sweep_desc_f32* y_desc,
                                            void* const* pool, int n_pool, size_t bytes, int tries, int* picks, double* times_ms)
{
    return tune_placement(ctx, cycle_f32{}, x_desc, y_desc, pool, n_pool, bytes, tries, picks, times_ms);
}

extern "C" int armon_hip_choose_placement(armon_ctx* ctx, const armon_sweep_desc* x_desc, const armon_sweep_desc* y_desc,
                                          void* const* pool, int n_pool, size_t bytes, int tries, double tolerance, int* picks,
                                          double* times_ms, int* tries_done)
{
    return choose_placement<double>(ctx, cycle_f64{bytes}, x_desc, y_desc, pool, n_pool, bytes, tries, tolerance, picks, times_ms,
                                    tries_done);
}

extern "C" int armon_hip_choose_placement_f32(armon_ctx* ctx, const armon_sweep_desc_f32* x_desc, const armon_sweep_desc_f32* y_desc,
                                              void* const* pool, int n_pool, size_t bytes, int tries, double tolerance, int* picks,
                                              double* times_ms, int* tries_done)
{
    return choose_placement<float>(ctx, cycle_f32{}, x_desc, y_desc, pool, n_pool, bytes, tries, tolerance, picks,
                                   times_ms, tries_done);
}
