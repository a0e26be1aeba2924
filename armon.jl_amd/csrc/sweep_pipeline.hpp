// sweep_pipeline.hpp — the fused directional sweep as a register-resident software pipeline (the "march" form).
//
// One lane marches along the sweep axis, one cell per step, and keeps in registers everything the
// reference passes between its five per-sweep kernels through memory (p, c, uˢ, pˢ, work_1..4 —
// ref src/solver.jl:300-316): EOS → first-order interface solve → GAD limited flux → Lagrangian cell
// update → advection (with minmod slopes) → Euler projection. Each step consumes the state of cell j
// and emits the post-sweep state of cell j - LAG, LAG = 2 + [GAD] + [euler_2nd] = 2..4, i.e. exactly
// the dependency cone i-LAG..i+LAG of the reference. Every interface solve, flux,
// update, slope and advection is computed ONCE (the staged GAD kernel solves each interface three
// times, ref src/riemann_schemes.jl:63-80).
//
// History lives in rings indexed by the step's phase, a template parameter: callers unroll the march,
// every ring index is a compile-time constant and no register is ever moved to "shift" the history.
// The cell ring has 8 slots and doubles as the landing zone of the caller's prefetch: the state of
// cell j is loaded straight into slot j mod 8 (up to 4 steps ahead) and stays there while the cell is
// the "current", "previous" and "second previous" cell of the pipeline. A slot is only reloaded after
// its last use, so no live value is ever copied (a reload overlapping a live value would force the
// compiler to copy registers at the loop back-edge, and those copies wait for the loads in flight).
// The other rings have 4 slots (2 for slopes / advection fluxes), indexed by the phase mod 4.
//
// Two arithmetic flavours with the same interface:
//  * Pipe      — EXACT: the same IEEE operations in the same order as the staged kernels and the reference formulas
//                (bit-identical results; needs -ffp-contract=off). States its arithmetic itself, and so does the exact
//                spatial form: both are pinned to the oracle's bits cell by cell by the tests, and as stage functions
//                their guarded quotients (a branch each) are rescheduled by the compiler at a cost in registers.
//  * PipeFast  — tuned (sweep_stages.hpp, fast::). Holds no formula: a step fetches the operands of each stage from the
//                ring slots of the steps that produced them, calls the stage and puts the results into this step's
//                slots. What is the march's own is what it keeps: the differences of consecutive cells (d_*) and the
//                reciprocal of the sum of two adjacent lengths (isum).
#pragma once

#include "sweep_stages.hpp"

namespace armon {
namespace fused {

template <typename T> struct Out4 { T rho, ua, ut, E; };

template <int SCHEME_, int LIM_, int PROJ_, int EOS_>
struct PipeTraits {
    static constexpr int SCHEME = SCHEME_, LIM = LIM_, PROJ = PROJ_, EOS = EOS_;
    static constexpr int S = (SCHEME == ARMON_SCHEME_GAD) ? 1 : 0;
    static constexpr int W = (PROJ == ARMON_PROJECTION_EULER_2ND) ? 1 : 0;
    static constexpr int LAG = S + W + 2;
};

// ======================================================================================================
// EXACT pipeline
// ======================================================================================================
template <int SCHEME, int LIM, int PROJ, int EOS, typename T = double>
struct Pipe : PipeTraits<SCHEME, LIM, PROJ, EOS> {
    using real = T;
    using TR = PipeTraits<SCHEME, LIM, PROJ, EOS>;
    static constexpr int S = TR::S, W = TR::W, LAG = TR::LAG;
    static constexpr bool kExact = true;

    using Den = xct::Den<T>;
    struct Cell { T rho, ua, ut, E, p, rc; };                 // pre-sweep state + EOS
    struct Upd { T rho, ua, ut, E, q_ua, q_ut, q_E; Den dxl; };   // Lagrangian (post cell_update) state; dxl prepared as a denominator

    T dt, dx, gamma;
    Den d_dx;                   // the uniform denominator dx
    Den dsum[2];                // (dxl[cu-1] + dxl[cu]) of this / the previous step: r₊ of one cell, r₋ of the next
    Cell c[8];                  // ring of 8: cells j+4 .. j (prefetched), j-1, j-2
    T gus[4], gps[4];      // ring: first-order solutions at interfaces j, j-1, j-2
    T fus[4], fps[4];      // ring: final fluxes at interfaces nf .. nf-3
    Upd l[4];                   // ring: updated cells cu, cu-1, cu-2   (cu = nf - 1)
    T s[2][4];             // minmod slopes of cells cu-1 / cu-2
    T a[2][4];             // advection fluxes at interfaces na / na-1
    T csr[4];              // ring: sound speed of cells j .. j-3 (dt/CFL tracking only)

    // (the two quotients the tuned pipeline takes from its caller are not used here: the exact flavour prepares denominators)
    __device__ __forceinline__ Pipe(T dt_, T dx_, T gamma_, T /*inv_dx*/, T /*dt_dx*/) : Pipe(dt_, dx_, gamma_) {}
    __device__ __forceinline__ Pipe(T dt_, T dx_, T gamma_) : dt(dt_), dx(dx_), gamma(gamma_), d_dx(dx_)
    {
        dsum[0] = dsum[1] = Den(dx_ + dx_);
        // Neutral, finite start values: the first 2*LAG outputs are discarded by the caller.
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = Cell{T(1.), T(0.), T(0.), T(1.), T(1.), T(1.)};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            gus[k] = T(0.); gps[k] = T(1.); fus[k] = T(0.); fps[k] = T(1.); csr[k] = T(1.);
            l[k] = Upd{T(1.), T(0.), T(0.), T(1.), T(0.), T(0.), T(1.), d_dx};
            s[0][k] = s[1][k] = T(0.);
            a[0][k] = a[1][k] = T(0.);
        }
    }

    // Feed cell j (pre-sweep state; Y_AXIS: ua is v and ut is u) and get the post-sweep state of cell
    // j - LAG. PH8 = step index mod 8. p_j, c_j: EOS of cell j, for optional materialisation.
    // c_lag: the (pre-sweep) sound speed of the emitted cell j - LAG, for the fused dt/CFL reduction.
    template <bool Y_AXIS, int PH8>
    __device__ __forceinline__ Out4<T> push(T rho, T ua, T ut, T E, T& p_j, T& c_j, T& c_lag)
    {
        Cell& n = c[PH8 & 7];
        n.rho = rho; n.ua = ua; n.ut = ut; n.E = E;
        return advance<Y_AXIS, PH8>(p_j, c_j, c_lag);
    }

    // Same, with (ρ, ua, ut, E) of cell j already stored in c[PH8 & 7] by the caller's prefetch.
    template <bool Y_AXIS, int PH8>
    __device__ __forceinline__ Out4<T> advance(T& p_j, T& c_j, T& c_lag)
    {
        constexpr int PH = PH8 & 3;
        constexpr int R0 = PH & 3, R1 = (PH - 1) & 3, R2 = (PH - 2) & 3, R3 = (PH - 3) & 3;
        constexpr int P0 = PH & 1, P1 = P0 ^ 1;
        c_lag = csr[(PH - LAG) & 3];      // LAG = 4: this very slot, read before it is overwritten below
        Cell& c0 = c[PH8 & 7];
        const Cell& c1 = c[(PH8 - 1) & 7];
        const Cell& c2 = c[(PH8 - 2) & 7];

        // ---- EOS (ref src/kernels.jl:4-55): e = E - 0.5*(u² + v²) with u, v in the reference's order
        T p, cs;
        {
            const T u = Y_AXIS ? c0.ut : c0.ua, v = Y_AXIS ? c0.ua : c0.ut;
            if (EOS == ARMON_EOS_BIZARRIUM) {
                T g_unused;
                phys::bizarrium<false>(c0.rho, c0.E, u, v, p, cs, g_unused);
            } else {
                phys::perfect_gas(gamma, c0.rho, c0.E, u, v, p, cs);
            }
        }
        p_j = p;
        c_j = cs;
        csr[R0] = cs;
        c0.p = p;
        c0.rc = c0.rho * cs;

        // ---- first-order acoustic solve at interface j (ref src/riemann_schemes.jl:21-30): one denominator
        {
            const T rc_l = c1.rc, rc_r = c0.rc;
            const Den d(rc_l + rc_r);
            gus[R0] = d.quo_t(rc_l * c1.ua + rc_r * c0.ua + (c1.p - c0.p));
            gps[R0] = d.quo(rc_r * c1.p + rc_l * c0.p + rc_l * rc_r * (c1.ua - c0.ua));
        }

        // ---- final flux at interface nf = j - S
        if (S == 1) {
            // acoustic_GAD! at interface i = j-1: cells i-s = c2, i = c1 (ref src/riemann_schemes.jl:84-104)
            const T gus0 = gus[R0], gps0 = gps[R0], gus1 = gus[R1], gps1 = gps[R1], gus2 = gus[R2], gps2 = gps[R2];
            const T r_um = phys::limiter<LIM>(Den(gus1 - c2.ua + T(1e-6)).quo_t(gus0 - c1.ua));
            const T r_pm = phys::limiter<LIM>(Den(gps1 - c2.p + T(1e-6)).quo(gps0 - c1.p));
            const T r_up = phys::limiter<LIM>(Den(c1.ua - gus1 + T(1e-6)).quo_t(c2.ua - gus2));
            const T r_pp = phys::limiter<LIM>(Den(c1.p - gps1 + T(1e-6)).quo(c2.p - gps2));
            const T dm_l = c2.rho * dx;
            const T dm_r = c1.rho * dx;
            const T Dm = (dm_l + dm_r) / 2;
            const T theta = T(0.5) * (1 - (c2.rc + c1.rc) / 2 * Den(Dm).quo(dt));
            fus[R0] = gus1 + theta * (r_up * (c1.ua - gus1) - r_um * (gus1 - c2.ua));
            fps[R0] = gps1 + theta * (r_pp * (c1.p - gps1) - r_pm * (gps1 - c2.p));
        } else {
            fus[R0] = gus[R0];
            fps[R0] = gps[R0];
        }
        const T fus0 = fus[R0], fps0 = fps[R0], fus1 = fus[R1], fps1 = fps[R1], fus2 = fus[R2], fus3 = fus[R3];

        // ---- Lagrangian update of cell cu = nf - 1 (ref src/kernels.jl:58-68)
        {
            const Cell& cc = (S == 1) ? c2 : c1;
            Upd& n = l[R0];
            const T dm = cc.rho * dx;
            n.dxl = Den(dx + dt * (fus0 - fus1));
            n.rho = n.dxl.quo(dm);
            const T dt_dm = Den(dm).quo(dt);
            n.ua = cc.ua + dt_dm * (fps1 - fps0);
            n.ut = cc.ut;
            n.E = cc.E + dt_dm * (fps1 * fus1 - fps0 * fus0);
            n.q_ua = n.rho * n.ua;
            n.q_ut = n.rho * n.ut;
            n.q_E = n.rho * n.E;
        }
        const Upd& l0 = l[R0];
        const Upd& l1 = l[R1];
        const Upd& l2 = l[R2];

        // ---- advection flux at interface na (→ a[P0]; a[P1] holds interface na-1), projection of na-1
        if (W == 1) {
            // slopes of cell cu-1 (ref src/projection_schemes.jl:105-116 evaluated per donor cell);
            // s[P1] still holds the slopes of cell cu-2 from the previous step.
            // r₋ = 2Δx/(Δx + Δx₋), r₊ = 2Δx/(Δx + Δx₊): this cell's Δx + Δx₊ is the next cell's Δx₋ + Δx (same bits:
            // IEEE addition commutes), so each sum is prepared once, by the step that first needs it
            dsum[P0] = Den(l1.dxl.b + l0.dxl.b);
            const T r_m = dsum[P1].quo(2 * l1.dxl.b);
            const T r_p = dsum[P0].quo(2 * l1.dxl.b);
            // reference order of the conserved quantities: ρ, ρu, ρv, ρE
            s[P0][0] = phys::slope_minmod(l2.rho, l1.rho, l0.rho, r_m, r_p);
            s[P0][Y_AXIS ? 2 : 1] = phys::slope_minmod(l2.q_ua, l1.q_ua, l0.q_ua, r_m, r_p);
            s[P0][Y_AXIS ? 1 : 2] = phys::slope_minmod(l2.q_ut, l1.q_ut, l0.q_ut, r_m, r_p);
            s[P0][3] = phys::slope_minmod(l2.q_E, l1.q_E, l0.q_E, r_m, r_p);
            // interface is = cu-1 (ref :92-124): upwind donor cell and its slopes
            const T disp = dt * fus2;
            const bool up = disp > 0;
            const Upd& d = up ? l2 : l1;
            const T Dxe = up ? -(dx - dt * fus3) : (dx + dt * fus1);
            const T lf = d.dxl.twice().quo(Dxe);
            const T q1 = Y_AXIS ? d.q_ut : d.q_ua, q2 = Y_AXIS ? d.q_ua : d.q_ut;
            a[P0][0] = disp * (d.rho - (up ? s[P1][0] : s[P0][0]) * lf);
            a[P0][1] = disp * (q1 - (up ? s[P1][1] : s[P0][1]) * lf);
            a[P0][2] = disp * (q2 - (up ? s[P1][2] : s[P0][2]) * lf);
            a[P0][3] = disp * (d.q_E - (up ? s[P1][3] : s[P0][3]) * lf);
            return project<Y_AXIS, P0>(l2);
        } else {
            // advection_first_order! at interface is = cu (ref src/projection_schemes.jl:62-78)
            const T disp = dt * fus1;
            const Upd& d = (disp > 0) ? l1 : l0;
            const T q1 = Y_AXIS ? d.q_ut : d.q_ua, q2 = Y_AXIS ? d.q_ua : d.q_ut;
            a[P0][0] = disp * d.rho;
            a[P0][1] = disp * q1;
            a[P0][2] = disp * q2;
            a[P0][3] = disp * d.q_E;
            return project<Y_AXIS, P0>(l1);
        }
    }

    // euler_projection! of cell o with A_o = a[P1], A_{o+1} = a[P0] (ref src/projection_schemes.jl:23-41)
    template <bool Y_AXIS, int P0>
    __device__ __forceinline__ Out4<T> project(const Upd& lo) const
    {
        constexpr int P1 = P0 ^ 1;
        const T dX = lo.dxl.b;
        const T u = Y_AXIS ? lo.ut : lo.ua, v = Y_AXIS ? lo.ua : lo.ut;   // reference's (u, v)
        const T t_rho  = d_dx.quo(dX * lo.rho        - (a[P0][0] - a[P1][0]));
        const T t_urho = d_dx.quo_t(dX * lo.rho * u    - (a[P0][1] - a[P1][1]));
        const T t_vrho = d_dx.quo_t(dX * lo.rho * v    - (a[P0][2] - a[P1][2]));
        const T t_Erho = d_dx.quo(dX * lo.rho * lo.E - (a[P0][3] - a[P1][3]));
        Out4<T> o;
        o.rho = t_rho;
        const Den d_rho(t_rho);
        const T un = d_rho.quo_t(t_urho), vn = d_rho.quo_t(t_vrho);
        o.ua = Y_AXIS ? vn : un;
        o.ut = Y_AXIS ? un : vn;
        o.E = d_rho.quo(t_Erho);
        return o;
    }
};

// ======================================================================================================
// tuned pipeline
// ======================================================================================================
template <int SCHEME, int LIM, int PROJ, int EOS, typename T = double>
struct PipeFast : PipeTraits<SCHEME, LIM, PROJ, EOS> {
    using real = T;
    using TR = PipeTraits<SCHEME, LIM, PROJ, EOS>;
    static constexpr int S = TR::S, W = TR::W, LAG = TR::LAG;
    static constexpr bool kExact = false;

    struct Cell { T rho, ua, ut, E, p, rc; };
    // Lagrangian state (fast::Lag) + d_* = q(this) - q(previous cell), kept for the next step's slopes
    struct Upd : fast::Lag<T> { T d_rho, d_ua, d_ut, d_E; };

    using Sc = typename fast::scalar_of<T>::type;     // uniform parameters
    Sc dt, dx, gamma, inv_dx, dt_dx, gm1, ggm1;
    Cell c[8];
    T gus[4], gps[4], src[4];          // first-order solutions + (rc_l + rc_r) of the interface
    T fps[4], dtu[4], pu[4];           // final flux: pˢ, dt·uˢ, pˢ·uˢ at interfaces nf .. nf-3
    Upd l[4];
    T isum[2];                         // 1 / (dxl[cu] + dxl[cu-1]) of this / the previous step
    T s[2][4];
    T a[2][4];
    T csr[4];

    __device__ __forceinline__ PipeFast(Sc dt_, Sc dx_, Sc gamma_) : PipeFast(dt_, dx_, gamma_, Sc(1.) / dx_, dt_ / dx_) {}
    // inv_dx_ = 1 / dx, dt_dx_ = dt / dx as IEEE quotients in the run's precision (the host forms them once per launch)
    __device__ __forceinline__ PipeFast(Sc dt_, Sc dx_, Sc gamma_, Sc inv_dx_, Sc dt_dx_) : dt(dt_), dx(dx_), gamma(gamma_)
    {
        inv_dx = inv_dx_;
        dt_dx = dt_dx_;
        gm1 = gamma_ - Sc(1.);
        ggm1 = gamma_ * (gamma_ - Sc(1.));
#pragma unroll
        for (int k = 0; k < 8; k++) c[k] = Cell{T(1.), T(0.), T(0.), T(1.), T(1.), T(1.)};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            gus[k] = T(0.); gps[k] = T(1.); src[k] = T(2.);
            fps[k] = T(1.); dtu[k] = T(0.); pu[k] = T(0.); csr[k] = T(1.);
            l[k] = Upd{{T(1.), T(0.), T(0.), T(1.), T(dx_), T(Sc(0.5) / dx_)}, T(0.), T(0.), T(0.), T(0.)};
            s[0][k] = s[1][k] = T(0.);
            a[0][k] = a[1][k] = T(0.);
        }
        isum[0] = isum[1] = T(Sc(0.5) / dx_);
    }

    template <bool Y_AXIS, int PH8>
    __device__ __forceinline__ Out4<T> push(T rho, T ua, T ut, T E, T& p_j, T& c_j, T& c_lag)
    {
        Cell& n = c[PH8 & 7];
        n.rho = rho; n.ua = ua; n.ut = ut; n.E = E;
        return advance<Y_AXIS, PH8>(p_j, c_j, c_lag);
    }

    template <bool Y_AXIS, int PH8>
    __device__ __forceinline__ Out4<T> advance(T& p_j, T& c_j, T& c_lag)
    {
        constexpr int PH = PH8 & 3;
        constexpr int R0 = PH & 3, R1 = (PH - 1) & 3, R2 = (PH - 2) & 3, R3 = (PH - 3) & 3;
        constexpr int P0 = PH & 1, P1 = P0 ^ 1;
        c_lag = csr[(PH - LAG) & 3];
        Cell& c0 = c[PH8 & 7];
        const Cell& c1 = c[(PH8 - 1) & 7];
        const Cell& c2 = c[(PH8 - 2) & 7];

        // ---- EOS of cell j
        T p, cs;
        fast::eos<EOS>(gm1, ggm1, c0.rho, c0.ua, c0.ut, c0.E, p, cs, c0.rc);
        p_j = p;
        c_j = cs;
        csr[R0] = cs;
        c0.p = p;

        // ---- first-order solve at interface j = c1 | c0
        fast::solve(c1.rc, c1.ua, c1.p, c0.rc, c0.ua, c0.p, gus[R0], gps[R0], src[R0]);

        // ---- final flux at interface nf = j - S; GAD: interface j-1 = c2 | c1, first-order solutions j-2, j-1, j
        T fus0;
        if (S == 1) {
            fast::gad<LIM>(dt_dx, c2.rho, c2.ua, c2.p, c1.rho, c1.ua, c1.p, src[R1],
                           gus[R2], gps[R2], gus[R1], gps[R1], gus[R0], gps[R0], fus0, fps[R0]);
        } else {
            fus0 = gus[R0];
            fps[R0] = gps[R0];
        }
        fast::flux_products(dt, fus0, fps[R0], dtu[R0], pu[R0]);

        // ---- Lagrangian update of cell cu = nf - 1, between interfaces nf-1 and nf; its differences to cell cu-1
        const Cell& cc = (S == 1) ? c2 : c1;
        Upd& n = l[R0];
        const Upd& prev = l[R1];
        static_cast<fast::Lag<T>&>(n) = fast::lagrange(dx, dt_dx, cc.rho, cc.ua, cc.ut, cc.E, fps[R1], dtu[R1], pu[R1],
                                                       fps[R0], dtu[R0], pu[R0]);
        n.d_rho = n.rho - prev.rho;
        n.d_ua = n.q_ua - prev.q_ua;
        n.d_ut = n.q_ut - prev.q_ut;
        n.d_E = n.q_E - prev.q_E;
        const Upd& l0 = l[R0];
        const Upd& l1 = l[R1];
        const Upd& l2 = l[R2];

        if (W == 1) {
            // slopes of cell cu-1 (stored in the reference's order ρ, ρu, ρv, ρE); of the two sums of lengths the second
            // is last step's first
            isum[P0] = fast::inv_pair_length(l1.dxl, l0.dxl);
            const T r_p = fast::slope_ratio(l1.dxl, isum[P0]), r_m = fast::slope_ratio(l1.dxl, isum[P1]);
            s[P0][0] = fast::slope(r_p, l0.d_rho, r_m, l1.d_rho);
            s[P0][Y_AXIS ? 2 : 1] = fast::slope(r_p, l0.d_ua, r_m, l1.d_ua);
            s[P0][Y_AXIS ? 1 : 2] = fast::slope(r_p, l0.d_ut, r_m, l1.d_ut);
            s[P0][3] = fast::slope(r_p, l0.d_E, r_m, l1.d_E);
            // interface cu-1, between interfaces cu-2 and cu; donor cell: cu-2 when it moves up, else cu-1 (per component)
            const T disp = dtu[R2];
            const auto up = disp > T(0.);
            const T Dxe = fast::sel(up, fast::extent_up(dtu[R3], dx), fast::extent_dn(dx, dtu[R1]));
            const T lf = fast::donor_reach(Dxe, fast::sel(up, l2.hinv, l1.hinv));
            const T d_q1 = Y_AXIS ? fast::sel(up, l2.q_ut, l1.q_ut) : fast::sel(up, l2.q_ua, l1.q_ua);
            const T d_q2 = Y_AXIS ? fast::sel(up, l2.q_ua, l1.q_ua) : fast::sel(up, l2.q_ut, l1.q_ut);
            a[P0][0] = fast::advect2(disp, lf, -fast::sel(up, s[P1][0], s[P0][0]), fast::sel(up, l2.rho, l1.rho));
            a[P0][1] = fast::advect2(disp, lf, -fast::sel(up, s[P1][1], s[P0][1]), d_q1);
            a[P0][2] = fast::advect2(disp, lf, -fast::sel(up, s[P1][2], s[P0][2]), d_q2);
            a[P0][3] = fast::advect2(disp, lf, -fast::sel(up, s[P1][3], s[P0][3]), fast::sel(up, l2.q_E, l1.q_E));
            return project<Y_AXIS, P0>(l2);
        } else {
            // interface cu; donor cell: cu-1 when it moves up, else cu
            const T disp = dtu[R1];
            const auto up = disp > T(0.);
            const T d_q1 = Y_AXIS ? fast::sel(up, l1.q_ut, l0.q_ut) : fast::sel(up, l1.q_ua, l0.q_ua);
            const T d_q2 = Y_AXIS ? fast::sel(up, l1.q_ua, l0.q_ua) : fast::sel(up, l1.q_ut, l0.q_ut);
            a[P0][0] = fast::advect1(disp, fast::sel(up, l1.rho, l0.rho));
            a[P0][1] = fast::advect1(disp, d_q1);
            a[P0][2] = fast::advect1(disp, d_q2);
            a[P0][3] = fast::advect1(disp, fast::sel(up, l1.q_E, l0.q_E));
            return project<Y_AXIS, P0>(l1);
        }
    }

    // projection of cell o with A_o = a[P1], A_{o+1} = a[P0]
    template <bool Y_AXIS, int P0>
    __device__ __forceinline__ Out4<T> project(const Upd& lo) const
    {
        Out4<T> o;
        const T q[4] = {lo.rho, Y_AXIS ? lo.q_ut : lo.q_ua, Y_AXIS ? lo.q_ua : lo.q_ut, lo.q_E};   // reference's order
        T un, vn;
        fast::project(inv_dx, lo.dxl, q, a[P0 ^ 1], a[P0], o.rho, un, vn, o.E);
        o.ua = Y_AXIS ? vn : un;
        o.ut = Y_AXIS ? un : vn;
        return o;
    }
};

}  // namespace fused
}  // namespace armon
