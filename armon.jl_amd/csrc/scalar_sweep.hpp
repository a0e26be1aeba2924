// scalar_sweep.hpp — armon_hip_sweep_scalars: passive scalars φ_k carried through one directional sweep.
//
// A passive scalar is "one more transverse velocity that does not enter the EOS": the Lagrangian phase leaves it alone, it
// is remapped as ρ·φ and divided by the new ρ. The fused sweeps are out of place, so after armon_hip_sweep the pre-sweep
// state is still there: this launch reads it again (ρ, u, v, E: 32 B per fp64 cell), redoes the state's EOS → solve → GAD →
// Lagrange → remap of ρ ONCE, and carries all ns planes through it (16 B per plane and cell). Neither direction states the
// sweep's arithmetic again: both run the state through the forms of armon_hip_sweep with outputs that are not stored (what
// only feeds u', v', E', p and c is dead code here and the compiler drops it) and add the planes' own remap.
//  * X sweep (k_scalar_x): lanes along x, neighbours by the DPP shifts of lane_shift.hpp — SpatialSweep<..., NS>
//    (sweep_spatial.hpp), which remaps the planes one after the other behind the state's projection. Tuned flavour: the very
//    stage functions (sweep_stages.hpp, fast::) with ρ_lag·φ in the slot of ρ·ut; exact flavour: the quotients of run_exact's
//    t_vrho / o_v lines.
//  * Y sweep (k_scalar_y): lanes along x, a register march in y. The state runs through Pipe / PipeFast as they are;
//    ScalarMarch reads the pipeline's rings after each step and keeps the rings of the planes next to them, with the
//    arithmetic the pipeline applies to its ut.
// The host side shares the descriptor checks, the common fill of sweep_args and the ladder with armon_hip_sweep
// (sweep_device.hpp: check_sweep_desc, base_sweep_args, with_flavour).
// Not a stand-alone header: scalar_sweep.hip (real = double) and scalar_sweep_f32.hip (real = float) include it.
#pragma once
#include "sweep_device.hpp"

namespace {

[[maybe_unused]] constexpr auto kNoFoldHere = &fold_dt_launch;     // (sweep_device.hpp's dt/CFL fold: nothing is tracked here)

// The planes' transport rule of this translation unit: scalar_sweep*.hip leave it at the remap of ρ·φ,
// scalar_sweep_bounded*.hip (armon_hip_sweep_scalars_bounded) choose φ per unit mass. Everything else — the checks, the
// launch geometry, the state's part of the kernels — is the same text.
#ifndef ARMON_SCALARS_TRANSPORT
#define ARMON_SCALARS_TRANSPORT 0
#endif
constexpr int kTransport = ARMON_SCALARS_TRANSPORT;
static_assert(kTransport == fused::kTransportRemap || kTransport == fused::kTransportBounded, "transport rule");

template <int NS>
struct scalar_planes {
    const real* in[NS];
    real* out[NS];
};

// ---- march form: the planes' rings next to those of Pipe / PipeFast ---------------------------------------------------
// step<PH8>() is called right after pipe.advance<Y_AXIS, PH8>() and reads what that step left in the pipeline's rings: the
// Lagrangian cells l[], the final fluxes, the sums of lengths, the advection fluxes of ρ. pc[n][slot]: φ_n of the cell in slot
// `slot` of the pipeline's cell ring (the caller's prefetch lands there). Returns φ_n of the cell the step emits.
// TRANSPORT: kTransportRemap — the above; kTransportBounded — φ per unit mass: rings of φ (not of q), of its
// plain minmod slopes σ and of the fluxes A = a_ρ·φ*, with the pipeline's own mass fluxes a[..][0] and Lagrangian cells.
template <class PIPE, int NS, int TRANSPORT = fused::kTransportRemap>
struct ScalarMarch {
    using T = typename PIPE::real;
    static constexpr int S = PIPE::S, W = PIPE::W, LAG = PIPE::LAG;
    T lphi[NS][4];        // exact, and bounded: φ of the Lagrangian cells cu, cu-1, cu-2, cu-3 (the pipeline's Upd::ut)
    T q[NS][4];           // remap: ρ_lag·φ of those cells
    T d[NS][4];           // remap, tuned: q(this) - q(previous cell) (the pipeline's Upd::d_ut)
    T s[NS][2];           // limited slopes of cells cu-1 / cu-2 (remap: of q; bounded: σ of φ)
    T a[NS][2];           // advection fluxes at interfaces na / na-1

    __device__ __forceinline__ ScalarMarch()
    {
#pragma unroll
        for (int n = 0; n < NS; n++) {
#pragma unroll
            for (int k = 0; k < 4; k++) lphi[n][k] = q[n][k] = d[n][k] = T(0.);
            s[n][0] = s[n][1] = a[n][0] = a[n][1] = T(0.);
        }
    }

    template <int PH8>
    __device__ __forceinline__ void step(const PIPE& p, const T (&pc)[NS][8], T (&out)[NS])
    {
        if constexpr (TRANSPORT == fused::kTransportBounded) step_bounded<PH8>(p, pc, out);
        else step_remap<PH8>(p, pc, out);
    }

    // φ per unit mass. Interface na is the low side of cell cu-1 (W = 1; donor cu-2 when it moves up, else cu-1) or of cell
    // cu (donor cu-1, else cu); the step emits the cell below it, whose neighbours are the ring's slots on either side.
    template <int PH8>
    __device__ __forceinline__ void step_bounded(const PIPE& p, const T (&pc)[NS][8], T (&out)[NS])
    {
        constexpr int PH = PH8 & 3;
        constexpr int R0 = PH & 3, R1 = (PH - 1) & 3, R2 = (PH - 2) & 3, R3 = (PH - 3) & 3;
        constexpr int P0 = PH & 1, P1 = P0 ^ 1;
        constexpr int CC = (S == 1) ? ((PH8 - 2) & 7) : ((PH8 - 1) & 7);     // the cell the step updated (cu)
        constexpr int LO = (W == 1) ? R2 : R1, LB = (W == 1) ? R3 : R2, LA = (W == 1) ? R1 : R0;   // emitted, below, above
        const auto& l1 = p.l[R1];
        const auto& l2 = p.l[R2];
        const auto& lo = p.l[LO];
        const T a_rho = p.a[P0][0];
#pragma unroll
        for (int n = 0; n < NS; n++) lphi[n][R0] = pc[n][CC];
        if constexpr (PIPE::kExact) {
            using Den = xct::Den<T>;
            if (W == 1) {
                const bool up = p.dt * p.fus[R2] > 0;
                const T nu = Den(up ? l2.dxl.b * l2.rho : l1.dxl.b * l1.rho).quo_t(phys::abs_(a_rho));
                const T h = T(0.5) * (1 - nu);
#pragma unroll
                for (int n = 0; n < NS; n++) {
                    s[n][P0] = phys::slope_minmod(lphi[n][R2], lphi[n][R1], lphi[n][R0], T(1.), T(1.));
                    a[n][P0] = a_rho * (up ? lphi[n][R2] + s[n][P1] * h : lphi[n][R1] - s[n][P0] * h);
                }
            } else {
                const bool up = p.dt * p.fus[R1] > 0;
#pragma unroll
                for (int n = 0; n < NS; n++) a[n][P0] = a_rho * (up ? lphi[n][R1] : lphi[n][R0]);
            }
            const T m = lo.dxl.b * lo.rho;
            const Den d_rho(p.d_dx.quo(m - (a_rho - p.a[P1][0])));
#pragma unroll
            for (int n = 0; n < NS; n++) {
                const T t_q = p.d_dx.quo_t(m * lphi[n][LO] - (a[n][P0] - a[n][P1]));
                const T v = d_rho.quo_t(t_q);
                const T f_lo = phys::mn(phys::mn(lphi[n][LB], lphi[n][LO]), lphi[n][LA]);
                const T f_hi = phys::mx(phys::mx(lphi[n][LB], lphi[n][LO]), lphi[n][LA]);
                out[n] = v < f_lo ? f_lo : (v > f_hi ? f_hi : v);
            }
        } else {
            namespace fast = fused::fast;
            if (W == 1) {
                const auto up = p.dtu[R2] > T(0.);
                const T h = fast::leaving_weight(a_rho, fast::inv_mass(fast::sel(up, l2.dxl * l2.rho, l1.dxl * l1.rho)));
#pragma unroll
                for (int n = 0; n < NS; n++) {
                    s[n][P0] = fast::minmod(lphi[n][R0] - lphi[n][R1], lphi[n][R1] - lphi[n][R2]);
                    a[n][P0] = fast::carry2(a_rho, h, fast::sel(up, s[n][P1], -s[n][P0]), fast::sel(up, lphi[n][R2], lphi[n][R1]));
                }
            } else {
                const auto up = p.dtu[R1] > T(0.);
#pragma unroll
                for (int n = 0; n < NS; n++) a[n][P0] = fast::carry1(a_rho, fast::sel(up, lphi[n][R1], lphi[n][R0]));
            }
            const T irho = fast::rcp(fast::fma_(lo.dxl, lo.rho, p.a[P1][0] - a_rho));     // 1 / T_ρ, as fast::project forms it
            const T m = lo.dxl * lo.rho;
#pragma unroll
            for (int n = 0; n < NS; n++)
                out[n] = fast::settle(m, irho, lphi[n][LO], a[n][P1], a[n][P0], lphi[n][LB], lphi[n][LA]);
        }
    }

    template <int PH8>
    __device__ __forceinline__ void step_remap(const PIPE& p, const T (&pc)[NS][8], T (&out)[NS])
    {
        constexpr int PH = PH8 & 3;
        constexpr int R0 = PH & 3, R1 = (PH - 1) & 3, R2 = (PH - 2) & 3, R3 = (PH - 3) & 3;
        constexpr int P0 = PH & 1, P1 = P0 ^ 1;
        constexpr int CC = (S == 1) ? ((PH8 - 2) & 7) : ((PH8 - 1) & 7);     // the cell the step updated (cu)
        constexpr int LO = (W == 1) ? R2 : R1;                               // the cell it emits
        const auto& l0 = p.l[R0];
        const auto& l1 = p.l[R1];
        const auto& l2 = p.l[R2];
        const auto& lo = p.l[LO];
        if constexpr (PIPE::kExact) {
            using Den = xct::Den<T>;
#pragma unroll
            for (int n = 0; n < NS; n++) {
                lphi[n][R0] = pc[n][CC];
                q[n][R0] = l0.rho * lphi[n][R0];
            }
            if (W == 1) {
                const T r_m = p.dsum[P1].quo(2 * l1.dxl.b);
                const T r_p = p.dsum[P0].quo(2 * l1.dxl.b);
                const T disp = p.dt * p.fus[R2];
                const bool up = disp > 0;
                const T Dxe = up ? -(p.dx - p.dt * p.fus[R3]) : (p.dx + p.dt * p.fus[R1]);
                const T lf = (up ? l2 : l1).dxl.twice().quo(Dxe);
#pragma unroll
                for (int n = 0; n < NS; n++) {
                    s[n][P0] = phys::slope_minmod(q[n][R2], q[n][R1], q[n][R0], r_m, r_p);
                    a[n][P0] = disp * ((up ? q[n][R2] : q[n][R1]) - (up ? s[n][P1] : s[n][P0]) * lf);
                }
            } else {
                const T disp = p.dt * p.fus[R1];
#pragma unroll
                for (int n = 0; n < NS; n++) a[n][P0] = disp * ((disp > 0) ? q[n][R1] : q[n][R0]);
            }
            const T dX = lo.dxl.b;
            const T t_rho = p.d_dx.quo(dX * lo.rho - (p.a[P0][0] - p.a[P1][0]));
            const Den d_rho(t_rho);
#pragma unroll
            for (int n = 0; n < NS; n++) {
                const T t_q = p.d_dx.quo_t(dX * lo.rho * lphi[n][LO] - (a[n][P0] - a[n][P1]));
                out[n] = d_rho.quo_t(t_q);
            }
        } else {
            namespace fast = fused::fast;
#pragma unroll
            for (int n = 0; n < NS; n++) {
                q[n][R0] = l0.rho * pc[n][CC];              // fast::lagrange: q_ut = ρ_lag·ut
                d[n][R0] = q[n][R0] - q[n][R1];
            }
            if (W == 1) {
                const T r_p = fast::slope_ratio(l1.dxl, p.isum[P0]), r_m = fast::slope_ratio(l1.dxl, p.isum[P1]);
                const T disp = p.dtu[R2];
                const auto up = disp > T(0.);
                const T Dxe = fast::sel(up, fast::extent_up(p.dtu[R3], p.dx), fast::extent_dn(p.dx, p.dtu[R1]));
                const T lf = fast::donor_reach(Dxe, fast::sel(up, l2.hinv, l1.hinv));
#pragma unroll
                for (int n = 0; n < NS; n++) {
                    s[n][P0] = fast::slope(r_p, d[n][R0], r_m, d[n][R1]);
                    a[n][P0] = fast::advect2(disp, lf, -fast::sel(up, s[n][P1], s[n][P0]), fast::sel(up, q[n][R2], q[n][R1]));
                }
            } else {
                const T disp = p.dtu[R1];
                const auto up = disp > T(0.);
#pragma unroll
                for (int n = 0; n < NS; n++) a[n][P0] = fast::advect1(disp, fast::sel(up, q[n][R1], q[n][R0]));
            }
#pragma unroll
            for (int n = 0; n < NS; n++) {
                const T qq[4] = {lo.rho, q[n][LO], q[n][LO], q[n][LO]};
                const T al[4] = {p.a[P1][0], a[n][P1], a[n][P1], a[n][P1]}, ah[4] = {p.a[P0][0], a[n][P0], a[n][P0], a[n][P0]};
                T o_rho, o_u, o_E;
                fast::project(p.inv_dx, lo.dxl, qq, al, ah, o_rho, o_u, out[n], o_E);
            }
        }
    }
};

// ---- X kernel ---------------------------------------------------------------------------------------------------------
// blockDim = (64, kSXRows): one wave per row and strip of 128 cells (two per lane), of which it produces the inner 120; strip
// origins sit on the 64-B sectors of the ghosted row as in k_sweep_x_dpp. grid = (strips, row groups, row-group overflow).
constexpr int kSXRows = 4;

template <int SCHEME, int LIM, int PROJ, int EOS, bool EXACT, int NS>
__global__ void __launch_bounds__(64 * kSXRows)
k_scalar_x(sweep_args a, scalar_planes<NS> ph, int vec)
{
    constexpr int K = 2, HALO = 4, WIDTH = 64 * K, STRIDE = WIDTH - 2 * HALO;
    using SW = fused::SpatialSweep<SCHEME, LIM, PROJ, EOS, EXACT, K, real, 0, NS, kTransport>;
    using St = fused::Strip<K, real>;
    static_assert(SW::LAG <= HALO, "strip halo");
    const int lane = threadIdx.x;
    const int64_t row = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * kSXRows + threadIdx.y;   // wave-uniform
    const int64_t w0 = a.x_first + (int64_t)blockIdx.x * STRIDE;                                  // first cell the strip produces
    if (row >= a.ny || w0 >= a.o_hi) return;
    const int64_t row_off = (row + a.g) * a.row_len + a.g;
    const real* in[4] = {a.rho_in + row_off, a.ua_in + row_off, a.ut_in + row_off, a.E_in + row_off};
    const int64_t cb = w0 - HALO;
    const int64_t j0 = cb + (int64_t)lane * K;
    St st[4], phi[NS], o_phi[NS];
    if (vec && cb >= 0 && cb + WIDTH <= a.nx) {                // uniform: no ghost, no clamping
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const vec2 v = ld2(in[q] + j0);
            st[q].v[0] = v.x;
            st[q].v[1] = v.y;
        }
#pragma unroll
        for (int n = 0; n < NS; n++) {
            const vec2 v = ld2(ph.in[n] + row_off + j0);
            phi[n].v[0] = v.x;
            phi[n].v[1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; k++) {
            // clamp into the block (ghosts included), then mirror physical boundaries: φ with factor +1
            int64_t j = j0 + k;
            j = j < -(int64_t)a.g ? -(int64_t)a.g : (j > a.nx + a.g - 1 ? a.nx + a.g - 1 : j);
            real fa, ft;
            const int64_t src = bc_source(a, a.nx, j, fa, ft);
            st[0].v[k] = in[0][src];
            st[1].v[k] = in[1][src] * fa;
            st[2].v[k] = in[2][src] * ft;
            st[3].v[k] = in[3][src];
#pragma unroll
            for (int n = 0; n < NS; n++) phi[n].v[k] = (ph.in[n] + row_off)[src];
        }
    }
    const SW sw{a.dt, a.dx, a.gamma, a.inv_dx, a.dt_dx};
    St unused[6];                                              // ρ', ua', ut', E', p, c: never stored
    sw.run(st[0], st[1], st[2], st[3], unused[0], unused[1], unused[2], unused[3], unused[4], unused[5], phi, o_phi);
    const int64_t hi = (w0 + STRIDE < a.o_hi) ? w0 + STRIDE : a.o_hi;
    const int64_t lo = w0 > a.o_lo ? w0 : a.o_lo;
    if (vec && j0 >= lo && j0 + 1 < hi) {
#pragma unroll
        for (int n = 0; n < NS; n++) st2(ph.out[n] + row_off + j0, o_phi[n].v[0], o_phi[n].v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int64_t j = j0 + k;
            if (j >= lo && j < hi) {
#pragma unroll
                for (int n = 0; n < NS; n++) (ph.out[n] + row_off)[j] = o_phi[n].v[k];
            }
        }
    }
}

// ---- Y kernel ---------------------------------------------------------------------------------------------------------
// k_sweep_y's march (one column per lane, runs of a.seg rows per workgroup, rows prefetched PF steps ahead into the cell
// ring) with the planes' rows prefetched next to the state's; it stores the planes only.
constexpr int kSYBlock = 256;
constexpr int kSYPf = 4;

template <class PIPE, int NS>
__global__ void __launch_bounds__(kSYBlock)
k_scalar_y(sweep_args a, scalar_planes<NS> ph)
{
    constexpr int LAG = PIPE::LAG, PF = kSYPf;
    const int nx = (int)a.nx, ny = (int)a.ny, g = a.g;
    const int xr = (int)(blockIdx.x * kSYBlock + threadIdx.x) - a.xshift;
    const bool active = xr >= 0 && xr < nx;
    const int x = active ? xr : (xr < 0 ? 0 : nx - 1);          // idle lanes shadow an edge column and never store
    const int o_hi = (int)a.o_hi;
    const int o0 = (int)a.o_lo + (int)blockIdx.y * a.seg;
    const int o1 = (o0 + a.seg < o_hi) ? o0 + a.seg : o_hi;
    const int jb = o0 - LAG, je = o1 + LAG;
    if ((int)(blockIdx.x * kSYBlock + (threadIdx.x & ~63u)) - a.xshift >= nx) return;   // a wave with no column at all

    // descriptors based at the first row this run touches: every row offset is a small non-negative 32-bit number
    const unsigned colb = (unsigned)(x + g) * (unsigned)sizeof(real);
    const unsigned pitchb = (unsigned)a.row_len * (unsigned)sizeof(real);
    const int64_t in_base = (int64_t)(jb + g) * a.row_len, out_base = (int64_t)(o0 + g) * a.row_len;
    const rsrc_t r_rho = make_rsrc(a.rho_in + in_base), r_ua = make_rsrc(a.ua_in + in_base);
    const rsrc_t r_ut = make_rsrc(a.ut_in + in_base), r_E = make_rsrc(a.E_in + in_base);
    rsrc_t r_phi[NS], w_phi[NS];
#pragma unroll
    for (int n = 0; n < NS; n++) {
        r_phi[n] = make_rsrc(ph.in[n] + in_base);
        w_phi[n] = make_rsrc(ph.out[n] + out_base);
    }

    PIPE pipe(a.dt, a.dx, a.gamma, a.inv_dx, a.dt_dx);
    ScalarMarch<PIPE, NS, kTransport> march;
    real pc[NS][8];
#pragma unroll
    for (int n = 0; n < NS; n++)
#pragma unroll
        for (int k = 0; k < 8; k++) pc[n][k] = real(0);

    int lj = jb;                     // next row to load and its offset from the run's first row
    unsigned lo_off = 0;
    unsigned so_off = (unsigned)(jb - LAG - o0) * pitchb;     // row j - LAG relative to row o0 (wraps until valid)

    auto load = [&](auto slot, auto checked) {
        constexpr int K = decltype(slot)::value & 7;
        constexpr bool CHECKED = decltype(checked)::value;
        auto& dst = pipe.c[K];
        if (CHECKED) {
            const bool m_lo = lj < 0 && a.bc_low, m_hi = lj >= ny && a.bc_high;     // uniform, rare
            const int src = m_lo ? -1 - lj : (m_hi ? 2 * ny - 1 - lj : lj);
            const unsigned off = (unsigned)(src - jb) * pitchb;
            const real fa = m_lo ? a.fa_low : (m_hi ? a.fa_high : real(1));
            const real ft = m_lo ? a.ft_low : (m_hi ? a.ft_high : real(1));
            dst.rho = buf_load<real>(r_rho, colb, off);
            dst.ua = buf_load<real>(r_ua, colb, off) * fa;
            dst.ut = buf_load<real>(r_ut, colb, off) * ft;
            dst.E = buf_load<real>(r_E, colb, off);
#pragma unroll
            for (int n = 0; n < NS; n++) pc[n][K] = buf_load<real>(r_phi[n], colb, off);     // mirrored with factor +1
            if (lj + 1 < je) {       // stay on the last row once the run is exhausted (padding steps)
                lj++;
                lo_off += pitchb;
            }
        } else {
            dst.rho = buf_load<real>(r_rho, colb, lo_off);
            dst.ua = buf_load<real>(r_ua, colb, lo_off);
            dst.ut = buf_load<real>(r_ut, colb, lo_off);
            dst.E = buf_load<real>(r_E, colb, lo_off);
#pragma unroll
            for (int n = 0; n < NS; n++) pc[n][K] = buf_load<real>(r_phi[n], colb, lo_off);
            lj++;
            lo_off += pitchb;
        }
    };
    using std::integral_constant;
    auto step = [&](auto ph8, auto checked, int j) {
        constexpr int PH8 = decltype(ph8)::value;
        constexpr bool CHECKED = decltype(checked)::value;
        load(integral_constant<int, PH8 + PF>{}, checked);   // row j + PF → slot (j + PF) mod 8
        real p, c, c_lag, out[NS];
        pipe.template advance<true, PH8>(p, c, c_lag);
        march.template step<PH8>(pipe, pc, out);
        const int o = j - LAG;
        if ((!CHECKED || (o >= o0 && o < o1)) && active) {
#pragma unroll
            for (int n = 0; n < NS; n++) buf_store(w_phi[n], colb, so_off, out[n]);
        }
        so_off += pitchb;
    };
    auto run = [&](auto checked, int t0, int t1) {           // steps [t0, t1), both multiples of 8
        for (int t = t0; t < t1; t += 8)
            static_for(std::make_integer_sequence<int, 8>{}, [&](auto ph8) { step(ph8, checked, jb + t + decltype(ph8)::value); });
    };

    const int T = je - jb;                                   // steps of the run
    const int T8 = (T + 7) & ~7;                             // … padded to the unroll
    const int P = (2 * LAG + 7) & ~7;                        // after P steps every step emits a valid cell
    // last step (exclusive) whose prefetch needs neither mirroring nor clamping and whose store is valid
    const int plain_end = (a.bc_high && ny < je ? ny : je) - jb - PF;
    int M = (T < plain_end ? T : plain_end) & ~7;
    if (M < P) M = P;
    static_for(std::make_integer_sequence<int, PF>{}, [&](auto k) { load(k, std::true_type{}); });
    run(std::true_type{}, 0, P < T8 ? P : T8);
    run(std::false_type{}, P, M);
    run(std::true_type{}, M, T8);
}

// ---- launch -----------------------------------------------------------------------------------------------------------
// Rows per run of the Y march: at least two rounds of workgroups on the device, runs of at least 32 rows (a run re-reads
// 2·LAG halo rows).
int scalar_y_seg(int n_cu, int64_t nx, int64_t ny)
{
    const int64_t cols = (nx + 16 + kSYBlock - 1) / kSYBlock;
    const int64_t slots = (int64_t)n_cu * 2;                 // workgroups of 4 waves, two waves per SIMD
    const int64_t nruns = (2 * slots + cols - 1) / cols;
    int64_t seg = (ny + nruns - 1) / nruns;
    if (seg < 32) seg = 32;
    if (seg > ny) seg = ny;
    return (int)seg;
}

template <class FL, int NS>
int scalar_launch(armon_ctx* ctx, const sweep_args& a, int axis, const real* const* phi_in, real* const* phi_out, bool vec)
{
    scalar_planes<NS> ph;
    for (int n = 0; n < NS; n++) {
        ph.in[n] = phi_in[n];
        ph.out[n] = phi_out[n];
    }
    if (axis == ARMON_AXIS_Y) {
        const dim3 grid((unsigned)((a.nx + a.xshift + kSYBlock - 1) / kSYBlock), (unsigned)((a.o_hi - a.o_lo + a.seg - 1) / a.seg));
        hipLaunchKernelGGL((k_scalar_y<typename FL::PIPE, NS>), grid, dim3(kSYBlock), 0, ctx->stream, a, ph);
        return check_launch("scalar_y");
    }
    const int64_t groups = (a.ny + kSXRows - 1) / kSXRows;
    const unsigned gy = (unsigned)(groups < 32768 ? groups : 32768);
    const dim3 grid((unsigned)((a.o_hi - a.x_first + 119) / 120), gy, (unsigned)((groups + gy - 1) / gy));
    hipLaunchKernelGGL((k_scalar_x<FL::SCHEME, FL::LIM, FL::PROJ, FL::EOS, FL::EXACT, NS>), grid, dim3(64, kSXRows), 0, ctx->stream, a, ph,
                       vec ? 1 : 0);
    return check_launch("scalar_x");
}

}  // namespace

extern "C" int ARMON_SCALARS_FN(armon_ctx* ctx, const ARMON_SWEEP_DESC* d, int ns, const real* const* phi_in, real* const* phi_out)
{
    ARMON_REQUIRE(ctx && d, "NULL argument");
    ARMON_REQUIRE(ns >= 1 && ns <= ARMON_MAX_SCALARS, "ns = %d: a launch carries 1 to %d scalar planes", ns, ARMON_MAX_SCALARS);
    ARMON_REQUIRE(phi_in && phi_out, "phi_in / phi_out: NULL array of planes");
    int lag;
    if (const int bad = check_sweep_desc(d, &lag); bad != ARMON_OK) return bad;
    const bool X = d->axis == ARMON_AXIS_X;
    const int64_t n_axis = X ? d->nx : d->ny;
    ARMON_REQUIRE(d->rho_in && d->u_in && d->v_in && d->E_in, "NULL state array (rho_in, u_in, v_in, E_in: the pre-sweep state)");
    // ---- what only the scalar sweep refuses -------------------------------------------------------------------------
    ARMON_REQUIRE(d->x_kernel == 0, "x_kernel = %d: the scalar sweep has one X form", d->x_kernel);
    ARMON_REQUIRE(!d->dt_state, "dt_state: the scalar sweep is host-driven (no device-resident time step)");
    ARMON_REQUIRE(d->out_hi == 0 || (d->out_lo == 0 && d->out_hi == n_axis),
                  "out_lo / out_hi = [%lld, %lld): the scalar sweep runs whole blocks", (long long)d->out_lo, (long long)d->out_hi);
    const void* state[8] = {d->rho_in, d->u_in, d->v_in, d->E_in, d->rho_out, d->u_out, d->v_out, d->E_out};
    for (int k = 0; k < ns; k++) {
        ARMON_REQUIRE(phi_in[k], "phi_in[%d] is NULL", k);
        ARMON_REQUIRE(phi_out[k], "phi_out[%d] is NULL", k);
        for (int j = 0; j < ns; j++) {
            ARMON_REQUIRE(phi_out[k] != phi_in[j], "phi_out[%d] aliases phi_in[%d] (the sweep is out of place)", k, j);
            ARMON_REQUIRE(j == k || phi_out[k] != phi_out[j], "phi_out[%d] aliases phi_out[%d]", k, j);
        }
        for (int j = 0; j < 8; j++)
            ARMON_REQUIRE((const void*)phi_out[k] != state[j], "phi_out[%d] aliases a state array of the descriptor", k);
    }

    const int64_t pitch = d->nx + 2 * (int64_t)d->nghost;
    sweep_args a = base_sweep_args(d, pitch, pitch);
    a.o_hi = n_axis;
    a.seg = X ? 512 : scalar_y_seg(ctx->n_cu, d->nx, d->ny);
    ARMON_REQUIRE(X || a.row_len * (int64_t)sizeof(real) * (a.seg + 2 * lag + 16) < (1ll << 32),
                  "block too wide for 32-bit row offsets (%lld cells per row, runs of %d rows)", (long long)d->nx, a.seg);
    a.xshift = X ? 0 : d->nghost % 16;
    a.x_first = X ? -(int64_t)(d->nghost % 8) : 0;
    // 16-B accesses of the X sweep: every lane pair on an even cell of an even-pitched row, in arrays that start on 16 B
    uintptr_t bases = (uintptr_t)d->rho_in | (uintptr_t)d->u_in | (uintptr_t)d->v_in | (uintptr_t)d->E_in;
    for (int k = 0; k < ns; k++) bases |= (uintptr_t)phi_in[k] | (uintptr_t)phi_out[k];
    const bool vec = X && a.row_len % 2 == 0 && bases % (2 * sizeof(real)) == 0;

    return with_flavour(d, [&](auto fl) {
        using FL = decltype(fl);
        switch (ns) {
        case 1: return scalar_launch<FL, 1>(ctx, a, d->axis, phi_in, phi_out, vec);
        case 2: return scalar_launch<FL, 2>(ctx, a, d->axis, phi_in, phi_out, vec);
        case 3: return scalar_launch<FL, 3>(ctx, a, d->axis, phi_in, phi_out, vec);
        default: return scalar_launch<FL, 4>(ctx, a, d->axis, phi_in, phi_out, vec);
        }
    });
}
