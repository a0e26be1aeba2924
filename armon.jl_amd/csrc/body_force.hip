// body_force.hip — a uniform acceleration (gx, gy) applied as one kick at the end of a cycle (the rule is
// stated word for word in include/armon_hip.h). No reference counterpart: the reference has no source terms.
//
// A streaming kernel: no LDS, no MFMA, lanes along x, the walk of every staged kernel (range_walk.hpp). One element per lane
// — a wave reads 512 B (fp64) or 256 B (fp32) of a row per plane, its first lane on a 64-B sector (row_thread's shift).
// Wider accesses were not taken: a real row starts nghost cells into a row of nx + 2 nghost, so whether a 16-B access is
// aligned depends on the parity of both, row by row when the pitch is odd; the sector-aligned one-element form is the one
// the staged kernels and init_regions.hip use and needs no edge handling. Rows are strided over gridDim.y, so every
// wave has several independent rows in flight.
//
// Templated on which components are non-zero: a plane whose component is zero is neither read nor written (its pointer may
// be NULL), so gy alone moves v and E only.
#include <cmath>

#include "common.hpp"
#include "range_walk.hpp"

using namespace armon;

namespace {

// One IEEE operation per operation written (the library is built with -ffp-contract=off).
template <typename T, bool GX, bool GY>
__global__ void __launch_bounds__(kBlock)
k_body_force(armon_range r, T dt, T gx, T gy, T* __restrict__ u, T* __restrict__ v, T* __restrict__ E)
{
    const T hx = T(0.5) * dt * gx;              // uniform: scalar registers
    const T hy = T(0.5) * dt * gy;
    ARMON_FOR_RANGE(r, i) {
        T work;
        if (GX && GY) {
            const T u0 = u[i], v0 = v[i];
            work = gx * (u0 + hx) + gy * (v0 + hy);
            u[i] = u0 + dt * gx;
            v[i] = v0 + dt * gy;
        } else if (GX) {
            const T u0 = u[i];
            work = gx * (u0 + hx);
            u[i] = u0 + dt * gx;
        } else {
            const T v0 = v[i];
            work = gy * (v0 + hy);
            v[i] = v0 + dt * gy;
        }
        E[i] = E[i] + dt * work;
    }
}

template <typename T>
int body_force_impl(armon_ctx* ctx, armon_range r, T dt, T gx, T gy, T* u, T* v, T* E)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(range_ok(r), "invalid range (col %lld:%lld:%lld row %lld+%lld)", (long long)r.col_start,
                  (long long)r.col_step, (long long)r.col_len, (long long)r.row_start, (long long)r.row_len);
    ARMON_REQUIRE(std::isfinite(dt), "dt is a NaN or an infinity");
    ARMON_REQUIRE(std::isfinite(gx), "gx is a NaN or an infinity");
    ARMON_REQUIRE(std::isfinite(gy), "gy is a NaN or an infinity");
    const bool x = gx != T(0), y = gy != T(0);
    if (!x && !y) return ARMON_OK;              // no force: nothing is launched, no plane is looked at
    ARMON_REQUIRE(E != nullptr, "E is NULL");
    ARMON_REQUIRE(!x || u != nullptr, "u is NULL with gx != 0");
    ARMON_REQUIRE(!y || v != nullptr, "v is NULL with gy != 0");
    if (range_empty(r)) return ARMON_OK;
    dim3 grid, block;
    range_grid(r, 1, grid, block);
    if (x && y)
        hipLaunchKernelGGL((k_body_force<T, true, true>), grid, block, 0, ctx->stream, r, dt, gx, gy, u, v, E);
    else if (x)
        hipLaunchKernelGGL((k_body_force<T, true, false>), grid, block, 0, ctx->stream, r, dt, gx, gy, u, v, E);
    else
        hipLaunchKernelGGL((k_body_force<T, false, true>), grid, block, 0, ctx->stream, r, dt, gx, gy, u, v, E);
    return check_launch("body_force");
}

}  // namespace

extern "C" {

int armon_hip_body_force(armon_ctx* ctx, armon_range real, double dt, double gx, double gy, double* u, double* v, double* E)
{
    return body_force_impl<double>(ctx, real, dt, gx, gy, u, v, E);
}

int armon_hip_body_force_f32(armon_ctx* ctx, armon_range real, float dt, float gx, float gy, float* u, float* v, float* E)
{
    return body_force_impl<float>(ctx, real, dt, gx, gy, u, v, E);
}

}  // extern "C"
