// diffuse.hip — one explicit step of physical diffusion: shear viscosity, conduction of the internal energy and a diffusivity
// per scalar plane (the rule is stated word for word in include/armon_hip.h). No reference counterpart.
//
// A nine-point stencil as a streaming kernel: no LDS, no MFMA, no barrier. Lanes along x, one column per lane; a wave owns a
// strip of kCols = 62 columns (its lanes 0 and 63 hold the columns just outside, whose results are discarded) and marches down
// a run of kRun rows. The x-neighbours of a value come from the DPP shifts of lane_shift.hpp; rows j and j+1 of the inputs (and
// u, v of row j-1) stay in registers, row j+2 is in flight, and the fluxes of the high y-face of row j are carried into row j+1 as its low ones. The
// flux of an x-face is evaluated by the lane on its left and handed to the lane on its right, so a face has ONE value. Every
// input element is therefore loaded once per strip and run: 64/62 of the columns and (kRun + 2)/kRun of the rows, from HBM
// once to first order (the halo rows of a run are the neighbouring runs' own rows: L2 hits when they run close in time).
//
// Cells outside the domain are never read as ghosts: the index of a neighbour outside [0, n) is wrapped or mirrored onto a
// real cell, column by column (per lane, once) and row by row (per wave, uniform), with the side's factor on u and v.
//
// Templated on STATE (nu or chi non-zero: u, v, E read and written) and on the number NS of diffusing planes; without STATE
// the planes and rho alone are touched.
#include <cmath>

#include "common.hpp"
#include "lane_shift.hpp"

using namespace armon;
using armon::fused::from_next_lane;
using armon::fused::from_prev_lane;

namespace {

constexpr int kCols = 62;        // columns a wave writes: 64 lanes less the two halo lanes
constexpr int kRun = 64;         // rows a wave marches down; it re-reads one row above and one below
constexpr int kWaves = kBlock / 64;

template <typename T>
struct DiffuseArgs {
    int64_t nx, ny, pitch;
    int nghost;
    int per_x, per_y;
    T fu_xl, fu_xh, fv_xl, fv_xh;              // factors of u and v across the low and high x sides, when they are not periodic
    T fu_yl, fu_yh, fv_yl, fv_yh;              // and across the y sides (single members, picked by selects: an array indexed
                                               // by the side would send the whole argument block through scratch memory)
    T dt, idx, idy, nu, chi, D[ARMON_MAX_SCALARS];
    const T *rho, *u, *v, *E;
    T *rho_out, *u_out, *v_out, *E_out;
    const T* phi[ARMON_MAX_SCALARS];
    T* phi_out[ARMON_MAX_SCALARS];
};

// index i in [-1, n] → the real cell that stands for it and which side it left through (0: none, 1: low, 2: high)
__device__ __forceinline__ int64_t map_index(int64_t i, int64_t n, int periodic, int& side)
{
    side = 0;
    if (i >= 0 && i < n) return i;
    if (periodic) return i < 0 ? n - 1 : 0;
    side = i < 0 ? 1 : 2;
    return i < 0 ? -1 - i : 2 * n - 1 - i;
}

// One row of a lane's column: what a step reads of it. u and v carry the factors of the sides the cell lies beyond.
template <typename T, bool STATE, int NS>
struct Row {
    T rho, u, v, e, E;
    T phi[NS > 0 ? NS : 1];
};

// The same row as it lies in memory: loaded one iteration ahead of its use, so that a wave has two rows in flight.
template <typename T, int NS>
struct Raw {
    T rho, u, v, E;
    T phi[NS > 0 ? NS : 1];
};

template <typename T, bool STATE, int NS>
__device__ __forceinline__ Raw<T, NS> load_raw(const DiffuseArgs<T>& a, int64_t j, int64_t col_off)
{
    Raw<T, NS> r{};
    int side;
    const int64_t jm = map_index(j, a.ny, a.per_y, side);
    const int64_t at = (jm + a.nghost) * a.pitch + col_off;
    r.rho = a.rho[at];
    if (STATE) {
        r.u = a.u[at];
        r.v = a.v[at];
        r.E = a.E[at];
    }
#pragma unroll
    for (int k = 0; k < NS; k++) r.phi[k] = a.phi[k][at];
    return r;
}

// row j from its loaded values: the factors of the sides it lies beyond, and e
template <typename T, bool STATE, int NS>
__device__ __forceinline__ Row<T, STATE, NS> finish_row(const DiffuseArgs<T>& a, const Raw<T, NS>& m, int64_t j, T fu_col, T fv_col)
{
    Row<T, STATE, NS> r{};
    int side;
    map_index(j, a.ny, a.per_y, side);
    r.rho = m.rho;
    if (STATE) {
        const T fu = side == 1 ? a.fu_yl : side == 2 ? a.fu_yh : T(1);
        const T fv = side == 1 ? a.fv_yl : side == 2 ? a.fv_yh : T(1);
        r.u = (m.u * fu_col) * fu;
        r.v = (m.v * fv_col) * fv;
        r.E = m.E;
        r.e = m.E - T(0.5) * (r.u * r.u + r.v * r.v);
    }
#pragma unroll
    for (int k = 0; k < NS; k++) r.phi[k] = m.phi[k];
    return r;
}

template <typename T, bool STATE, int NS>
__device__ __forceinline__ Row<T, STATE, NS> load_row(const DiffuseArgs<T>& a, int64_t j, int64_t col_off, T fu_col, T fv_col)
{
    return finish_row<T, STATE, NS>(a, load_raw<T, STATE, NS>(a, j, col_off), j, fu_col, fv_col);
}

// the fluxes of a face, in the order u, v, E, phi_k
template <typename T, int NS>
struct Flux {
    T u, v, E;
    T phi[NS > 0 ? NS : 1];
};

// x-face between this lane's cell L and the next lane's R, both in row j; du, dv: a[j+1] - a[j-1] of this lane's column
template <typename T, bool STATE, int NS>
__device__ __forceinline__ Flux<T, NS> x_face(const DiffuseArgs<T>& a, const Row<T, STATE, NS>& L, T du, T dv)
{
    Flux<T, NS> f{};
    const T rf = T(0.5) * (L.rho + from_next_lane(L.rho));
    if (STATE) {
        const T q4y = T(0.25) * a.idy, c43 = T(4) / T(3), c23 = T(2) / T(3);
        const T uR = from_next_lane(L.u), vR = from_next_lane(L.v), eR = from_next_lane(L.e);
        const T mu = a.nu * rf;
        const T ux = (uR - L.u) * a.idx;
        const T vx = (vR - L.v) * a.idx;
        const T uy = (du + from_next_lane(du)) * q4y;
        const T vy = (dv + from_next_lane(dv)) * q4y;
        const T txx = mu * (c43 * ux - c23 * vy);
        const T txy = mu * (uy + vx);
        const T uf = T(0.5) * (L.u + uR);
        const T vf = T(0.5) * (L.v + vR);
        const T q = (a.chi * rf) * ((eR - L.e) * a.idx);
        f.u = txx;
        f.v = txy;
        f.E = (uf * txx + vf * txy) + q;
    }
#pragma unroll
    for (int k = 0; k < NS; k++) f.phi[k] = (a.D[k] * rf) * ((from_next_lane(L.phi[k]) - L.phi[k]) * a.idx);
    return f;
}

// y-face between L (row j) and R (row j+1) of this lane's column; dLu .. dRv: a[i+1] - a[i-1] in either row
template <typename T, bool STATE, int NS>
__device__ __forceinline__ Flux<T, NS> y_face(const DiffuseArgs<T>& a, const Row<T, STATE, NS>& L, const Row<T, STATE, NS>& R,
                                              T dLu, T dLv, T dRu, T dRv)
{
    Flux<T, NS> g{};
    const T rf = T(0.5) * (L.rho + R.rho);
    if (STATE) {
        const T q4x = T(0.25) * a.idx, c43 = T(4) / T(3), c23 = T(2) / T(3);
        const T mu = a.nu * rf;
        const T uy = (R.u - L.u) * a.idy;
        const T vy = (R.v - L.v) * a.idy;
        const T ux = (dLu + dRu) * q4x;
        const T vx = (dLv + dRv) * q4x;
        const T tyy = mu * (c43 * vy - c23 * ux);
        const T txy = mu * (uy + vx);
        const T uf = T(0.5) * (L.u + R.u);
        const T vf = T(0.5) * (L.v + R.v);
        const T q = (a.chi * rf) * ((R.e - L.e) * a.idy);
        g.u = txy;
        g.v = tyy;
        g.E = (uf * txy + vf * tyy) + q;
    }
#pragma unroll
    for (int k = 0; k < NS; k++) g.phi[k] = (a.D[k] * rf) * ((R.phi[k] - L.phi[k]) * a.idy);
    return g;
}

template <typename T, bool STATE, int NS>
__global__ void __launch_bounds__(kBlock)
k_diffuse(const DiffuseArgs<T> a)
{
    const int lane = threadIdx.x & 63;
    const int64_t strip = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int64_t c0 = strip * kCols;
    if (c0 >= a.nx) return;                                    // a whole wave: no lane of it takes part in a shift
    // the lane's column, and the real column that stands for it (lanes past the first column outside hold that column again)
    int64_t c = c0 - 1 + lane;
    if (c > a.nx) c = a.nx;
    int side;
    const int64_t cm = map_index(c, a.nx, a.per_x, side);
    const T fu_col = side == 1 ? a.fu_xl : side == 2 ? a.fu_xh : T(1);
    const T fv_col = side == 1 ? a.fv_xl : side == 2 ? a.fv_xh : T(1);
    const int64_t col_off = a.nghost + cm;
    const bool writes = lane >= 1 && lane <= kCols && c < a.nx;

    const int64_t j0 = (int64_t)blockIdx.y * kRun;
    const int64_t j1 = j0 + kRun < a.ny ? j0 + kRun : a.ny;

    using R = Row<T, STATE, NS>;
    R below = load_row<T, STATE, NS>(a, j0 - 1, col_off, fu_col, fv_col);
    R here = load_row<T, STATE, NS>(a, j0, col_off, fu_col, fv_col);
    Raw<T, NS> ahead = load_raw<T, STATE, NS>(a, j0 + 1, col_off);          // (j0 + 1 <= ny: a row map_index knows)
    T dxu_b = T(0), dxv_b = T(0), dxu_h = T(0), dxv_h = T(0);  // a[i+1] - a[i-1] of rows j-1 and j
    if (STATE) {
        dxu_b = from_next_lane(below.u) - from_prev_lane(below.u);
        dxv_b = from_next_lane(below.v) - from_prev_lane(below.v);
        dxu_h = from_next_lane(here.u) - from_prev_lane(here.u);
        dxv_h = from_next_lane(here.v) - from_prev_lane(here.v);
    }
    Flux<T, NS> g_lo = y_face<T, STATE, NS>(a, below, here, dxu_b, dxv_b, dxu_h, dxv_h);
    T u_below = below.u, v_below = below.v;

    for (int64_t j = j0; j < j1; j++) {
        const R above = finish_row<T, STATE, NS>(a, ahead, j + 1, fu_col, fv_col);
        // row j + 2 for the next iteration, asked for before this one's arithmetic (the run's last iteration asks for row
        // j1 again, a row of the block or the one just outside, and does not use it)
        ahead = load_raw<T, STATE, NS>(a, j + 2 <= j1 ? j + 2 : j1, col_off);
        T dxu_a = T(0), dxv_a = T(0), du = T(0), dv = T(0);
        if (STATE) {
            dxu_a = from_next_lane(above.u) - from_prev_lane(above.u);
            dxv_a = from_next_lane(above.v) - from_prev_lane(above.v);
            du = above.u - u_below;
            dv = above.v - v_below;
        }
        const Flux<T, NS> g_hi = y_face<T, STATE, NS>(a, here, above, dxu_h, dxv_h, dxu_a, dxv_a);
        const Flux<T, NS> f_hi = x_face<T, STATE, NS>(a, here, du, dv);
        Flux<T, NS> f_lo{};
        if (STATE) {
            f_lo.u = from_prev_lane(f_hi.u);
            f_lo.v = from_prev_lane(f_hi.v);
            f_lo.E = from_prev_lane(f_hi.E);
        }
#pragma unroll
        for (int k = 0; k < NS; k++) f_lo.phi[k] = from_prev_lane(f_hi.phi[k]);

        const T kk = a.dt / here.rho;
        if (writes) {
            const int64_t at = (j + a.nghost) * a.pitch + col_off;
            if (a.rho_out) a.rho_out[at] = here.rho;
            if (STATE) {
                // the cell's own u and v: a writing lane's column lies inside the block, so its column factors are +1 and its
                // row is real
                a.u_out[at] = here.u + kk * ((f_hi.u - f_lo.u) * a.idx + (g_hi.u - g_lo.u) * a.idy);
                a.v_out[at] = here.v + kk * ((f_hi.v - f_lo.v) * a.idx + (g_hi.v - g_lo.v) * a.idy);
                a.E_out[at] = here.E + kk * ((f_hi.E - f_lo.E) * a.idx + (g_hi.E - g_lo.E) * a.idy);
            }
#pragma unroll
            for (int k = 0; k < NS; k++)
                a.phi_out[k][at] = here.phi[k] + kk * ((f_hi.phi[k] - f_lo.phi[k]) * a.idx + (g_hi.phi[k] - g_lo.phi[k]) * a.idy);
        }
        u_below = here.u;
        v_below = here.v;
        here = above;
        dxu_h = dxu_a;
        dxv_h = dxv_a;
        g_lo = g_hi;
    }
}

template <typename T, bool STATE>
void launch_ns(int ns, dim3 grid, hipStream_t s, const DiffuseArgs<T>& a)
{
    switch (ns) {
    case 0:                                     // (the state alone; without it nothing diffuses and nothing is launched)
        if constexpr (STATE) hipLaunchKernelGGL((k_diffuse<T, true, 0>), grid, dim3(kBlock), 0, s, a);
        break;
    case 1: hipLaunchKernelGGL((k_diffuse<T, STATE, 1>), grid, dim3(kBlock), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_diffuse<T, STATE, 2>), grid, dim3(kBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_diffuse<T, STATE, 3>), grid, dim3(kBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((k_diffuse<T, STATE, 4>), grid, dim3(kBlock), 0, s, a); break;
    }
}

template <typename T, typename Desc>
int diffuse_impl(armon_ctx* ctx, const Desc* d)
{
    ARMON_REQUIRE(ctx != nullptr, "ctx is NULL");
    ARMON_REQUIRE(d != nullptr, "the descriptor is NULL");
    ARMON_REQUIRE(d->ns >= 0 && d->ns <= ARMON_MAX_SCALARS, "ns = %d is outside 0..%d", d->ns, ARMON_MAX_SCALARS);
    ARMON_REQUIRE(std::isfinite(d->dt) && d->dt >= 0, "dt = %g is negative or not finite", d->dt);
    ARMON_REQUIRE(std::isfinite(d->nu) && d->nu >= 0, "nu = %g is negative or not finite", d->nu);
    ARMON_REQUIRE(std::isfinite(d->chi) && d->chi >= 0, "chi = %g is negative or not finite", d->chi);
    DiffuseArgs<T> a{};
    a.dt = T(d->dt), a.nu = T(d->nu), a.chi = T(d->chi);
    ARMON_REQUIRE(std::isfinite(a.dt) && std::isfinite(a.nu) && std::isfinite(a.chi), "dt, nu or chi is not finite in the data type");
    bool any = a.nu != T(0) || a.chi != T(0);
    for (int k = 0; k < d->ns; k++) {
        ARMON_REQUIRE(std::isfinite(d->D[k]) && d->D[k] >= 0, "D[%d] = %g is negative or not finite", k, d->D[k]);
        a.D[k] = T(d->D[k]);
        ARMON_REQUIRE(std::isfinite(a.D[k]), "D[%d] is not finite in the data type", k);
        any = any || a.D[k] != T(0);
    }
    if (!any) return ARMON_OK;                  // nothing diffuses: nothing is launched, no plane is looked at
    const bool state = a.nu != T(0) || a.chi != T(0);
    ARMON_REQUIRE(d->nx >= 1 && d->ny >= 1, "empty block: nx = %lld, ny = %lld", (long long)d->nx, (long long)d->ny);
    ARMON_REQUIRE(d->nghost >= 0 && d->nghost <= 1024, "nghost = %d is outside 0..1024", d->nghost);
    const int64_t n_runs = (d->ny + kRun - 1) / kRun, n_strips = (d->nx + kCols - 1) / kCols;
    const int64_t n_blocks = (n_strips + kWaves - 1) / kWaves;
    ARMON_REQUIRE(n_runs <= 65535 && n_blocks <= 0x7fffffff && d->nx <= (int64_t)1 << 40,
                  "oversized block: nx = %lld, ny = %lld (at most %d rows)", (long long)d->nx, (long long)d->ny, 65535 * kRun);
    ARMON_REQUIRE(std::isfinite(d->dx) && d->dx > 0, "dx = %g is not finite and positive", d->dx);
    ARMON_REQUIRE(std::isfinite(d->dy) && d->dy > 0, "dy = %g is not finite and positive", d->dy);
    a.idx = T(1) / T(d->dx), a.idy = T(1) / T(d->dy);
    ARMON_REQUIRE(std::isfinite(a.idx) && std::isfinite(a.idy), "1/dx or 1/dy is not finite in the data type");
    for (int axis = 0; axis < 2; axis++) {
        const int lo = 2 * axis, hi = lo + 1;
        ARMON_REQUIRE(!d->periodic[lo] == !d->periodic[hi], "periodic flag on one side of the %s axis only (%d, %d)",
                      axis ? "y" : "x", d->periodic[lo], d->periodic[hi]);
        if (d->periodic[lo]) continue;
        for (int s = lo; s <= hi; s++) {
            ARMON_REQUIRE(d->u_factor[s] == 1 || d->u_factor[s] == -1, "u_factor[%d] = %g is not +1 or -1", s, d->u_factor[s]);
            ARMON_REQUIRE(d->v_factor[s] == 1 || d->v_factor[s] == -1, "v_factor[%d] = %g is not +1 or -1", s, d->v_factor[s]);
        }
    }
    // arrays: what the step reads, what it writes, and that no output is an input or another output
    const void* in[4 + ARMON_MAX_SCALARS];
    const void* out[4 + ARMON_MAX_SCALARS];
    int n_in = 0, n_out = 0;
    ARMON_REQUIRE(d->rho != nullptr, "rho is NULL");
    in[n_in++] = d->rho;
    if (d->rho_out) out[n_out++] = d->rho_out;
    if (state) {
        ARMON_REQUIRE(d->u != nullptr, "u is NULL");
        ARMON_REQUIRE(d->v != nullptr, "v is NULL");
        ARMON_REQUIRE(d->E != nullptr, "E is NULL");
        ARMON_REQUIRE(d->u_out != nullptr, "u_out is NULL");
        ARMON_REQUIRE(d->v_out != nullptr, "v_out is NULL");
        ARMON_REQUIRE(d->E_out != nullptr, "E_out is NULL");
        in[n_in++] = d->u, in[n_in++] = d->v, in[n_in++] = d->E;
        out[n_out++] = d->u_out, out[n_out++] = d->v_out, out[n_out++] = d->E_out;
    }
    for (int k = 0; k < d->ns; k++) {
        ARMON_REQUIRE(d->phi[k] != nullptr, "phi[%d] is NULL", k);
        ARMON_REQUIRE(d->phi_out[k] != nullptr, "phi_out[%d] is NULL", k);
        in[n_in++] = d->phi[k];
        out[n_out++] = d->phi_out[k];
    }
    for (int i = 0; i < n_out; i++) {
        for (int k = 0; k < n_in; k++) ARMON_REQUIRE(out[i] != in[k], "output array %d is an input array (aliasing)", i);
        for (int k = 0; k < i; k++) ARMON_REQUIRE(out[i] != out[k], "output arrays %d and %d are the same (aliasing)", k, i);
    }

    a.nx = d->nx, a.ny = d->ny, a.nghost = d->nghost, a.pitch = d->nx + 2 * (int64_t)d->nghost;
    a.per_x = d->periodic[ARMON_SIDE_LEFT] != 0, a.per_y = d->periodic[ARMON_SIDE_BOTTOM] != 0;
    a.fu_xl = T(d->u_factor[ARMON_SIDE_LEFT]), a.fu_xh = T(d->u_factor[ARMON_SIDE_RIGHT]);
    a.fv_xl = T(d->v_factor[ARMON_SIDE_LEFT]), a.fv_xh = T(d->v_factor[ARMON_SIDE_RIGHT]);
    a.fu_yl = T(d->u_factor[ARMON_SIDE_BOTTOM]), a.fu_yh = T(d->u_factor[ARMON_SIDE_TOP]);
    a.fv_yl = T(d->v_factor[ARMON_SIDE_BOTTOM]), a.fv_yh = T(d->v_factor[ARMON_SIDE_TOP]);
    a.rho = d->rho, a.rho_out = d->rho_out;
    if (state) {
        a.u = d->u, a.v = d->v, a.E = d->E;
        a.u_out = d->u_out, a.v_out = d->v_out, a.E_out = d->E_out;
    }
    for (int k = 0; k < d->ns; k++) a.phi[k] = d->phi[k], a.phi_out[k] = d->phi_out[k];

    const dim3 grid((unsigned)n_blocks, (unsigned)n_runs, 1);
    if (state)
        launch_ns<T, true>(d->ns, grid, ctx->stream, a);
    else
        launch_ns<T, false>(d->ns, grid, ctx->stream, a);
    return check_launch("diffuse");
}

}  // namespace

extern "C" {

int armon_hip_diffuse(armon_ctx* ctx, const armon_diffuse_desc* d) { return diffuse_impl<double>(ctx, d); }

int armon_hip_diffuse_f32(armon_ctx* ctx, const armon_diffuse_desc_f32* d) { return diffuse_impl<float>(ctx, d); }

}  // extern "C"
