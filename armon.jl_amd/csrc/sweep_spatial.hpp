// sweep_spatial.hpp — the fused X sweep with lanes laid ALONG the sweep axis (the "spatial" form).
//
// For an X sweep the stencil runs along the contiguous axis, so a wave owns a strip of 64·K consecutive
// cells of one row (K cells per lane) and every stage of the sweep is evaluated "in place": a lane
// computes the EOS of its own cells, the interface solve on the low side of each of its cells, the
// limited flux there, the Lagrangian update of its cells, their slopes, the advection flux on their
// low side and finally their projection. What the reference hands from one kernel to the next through
// memory, and what the marching pipeline (sweep_pipeline.hpp) keeps in a lane's registers across steps,
// is here fetched from the neighbouring lane with DPP wavefront shifts (lane_shift.hpp): no LDS, no barrier,
// fully coalesced loads and stores, and ~1/3 of the registers of the marching form, so 4+ waves per SIMD
// hide the fp64 and memory latencies.
// Cost: the first and last HALO cells of a strip are recomputed by the neighbouring strip.
//
// Tuned flavour: run_fast holds no formula. It fetches the operands of each stage from its own cells and through
// left_of / right_of, calls the stage (sweep_stages.hpp, fast:: — the very functions PipeFast calls) and stores the
// results into Strips; it takes differences and the reciprocal of the right-hand sum of lengths from the neighbouring
// lane where the march keeps them from the previous step, and evaluates only the chosen donor's operands.
// Exact flavour: run_exact states its arithmetic itself, like Pipe (sweep_pipeline.hpp says why).
//
// Passive scalars (NS > 0; scalar_sweep.hpp's k_scalar_x): the sweep carries NS planes φ_n behind the state,
// as ScalarMarch carries them beside Pipe in Y. A plane is "one more ut": q = ρ_lag·φ takes the slope, the advection flux and
// the projection of ρ·ut, with the operations of that line. Everything about the planes stands in `if constexpr (NS > 0)`;
// with NS = 0 no line of the sweep depends on them. The planes are remapped ONE AFTER THE OTHER, behind the state's
// projection, from what they share with ρ (slope ratios, donor reach and — exact flavour — the displacement, kept in Strips
// under NS > 0 only; the tuned displacement dtu and the fluxes of ρ are there anyway): remapping them inside the state's own
// loops keeps every plane's q, slope and flux alive next to the state's four, which cost a prototype's fp64 ns = 4 kernels
// 40-50 VGPRs and two to three waves per SIMD (profiles/scalar_unify_resources.txt).
//
// TRANSPORT (NS > 0 only) chooses the planes' rule. kTransportRemap: the one above. kTransportBounded: φ per
// unit mass — the flux of a plane is the state's own mass flux a0 times the mean of the donor's limited profile of φ over the
// mass that leaves it, φ* = φ_d ± σ_d·½(1 − ν), σ a plain minmod of φ's two differences, ν = |a0| / m_d, m = Δx_lag·ρ_lag; then
// φ' = (m φ − ΔA) / dx / ρ', clamped to the smallest and largest of φ at i−1, i, i+1. It shares the mass, the weight ½(1 − ν) of
// every interface and (exact flavour) the displacement with ρ, and none of the slope ratios or the donor reach.
#pragma once

#include "lane_shift.hpp"
#include "sweep_pipeline.hpp"

namespace armon {
namespace fused {

// One X sweep of the K cells held by each lane. In: pre-sweep (ρ, u, v, E). Out: post-sweep state, valid
// for the cells at least LAG cells away from both ends of the wave's strip; p/c: EOS of the cells.
// NS > 0: also the planes phi[0..NS) → o_phi[0..NS), valid for the same cells.
constexpr int kTransportRemap = 0, kTransportBounded = 1;

template <int SCHEME, int LIM, int PROJ, int EOS, bool EXACT, int K, typename T = double, int ROW = 0, int NS = 0,
          int TRANSPORT = kTransportRemap>
struct SpatialSweep {
    static constexpr bool REMAP = NS > 0 && TRANSPORT == kTransportRemap, BOUNDED = NS > 0 && TRANSPORT == kTransportBounded;
    using TR = PipeTraits<SCHEME, LIM, PROJ, EOS>;
    static constexpr int S = TR::S, W = TR::W, LAG = TR::LAG;
    using S_ = Strip<K, T>;
    using Sh = Shifted<K, T>;
    // neighbour access of this sweep's strip shape (the whole wave, or rows of 16 lanes)
    static __device__ __forceinline__ Sh left_of(const S_& s) { return fused::left_of<ROW, K, T>(s); }
    static __device__ __forceinline__ Sh right_of(const S_& s) { return fused::right_of<ROW, K, T>(s); }

    T dt, dx, gamma;
    // 1 / dx and dt / dx, formed by the caller (the host, in the run's precision; armon_hip_sweep): a wave lives for one
    // strip, and the two IEEE divisions (two v_rcp_f64 at 4x the issue cost of an FMA + their expansions, ~40 FMA slots of
    // a strip's ~600) were per-wave work. Tuned arithmetic only; the exact flavour prepares its own denominators.
    T inv_dx, dt_dx;

    __device__ __forceinline__ void run(const S_& rho, const S_& u, const S_& v, const S_& E,
                                        S_& o_rho, S_& o_u, S_& o_v, S_& o_E, S_& p, S_& cs,
                                        const S_* phi = nullptr, S_* o_phi = nullptr) const
    {
        if (EXACT) run_exact(rho, u, v, E, o_rho, o_u, o_v, o_E, p, cs, phi, o_phi);
        else run_fast(rho, u, v, E, o_rho, o_u, o_v, o_E, p, cs, phi, o_phi);
    }

    // ---------------------------------------------------------------------------------------------
    __device__ __forceinline__ void run_exact(const S_& rho, const S_& ua, const S_& ut, const S_& E,
                                              S_& o_rho, S_& o_u, S_& o_v, S_& o_E, S_& p, S_& cs,
                                              const S_* phi = nullptr, S_* o_phi = nullptr) const
    {
        using Den = xct::Den<T>;       // correctly rounded quotients, shared denominators (sweep_pipeline.hpp)
        const Den d_dx(dx);
        S_ rc;
#pragma unroll
        for (int k = 0; k < K; k++) {
            if (EOS == ARMON_EOS_BIZARRIUM) {
                T g_unused;
                phys::bizarrium<false>(rho[k], E[k], ua[k], ut[k], p.v[k], cs.v[k], g_unused);
            } else {
                phys::perfect_gas(gamma, rho[k], E[k], ua[k], ut[k], p.v[k], cs.v[k]);
            }
            rc.v[k] = rho[k] * cs[k];
        }
        // first-order solve on the low side of each cell (ref src/riemann_schemes.jl:21-30)
        const Sh rcL = left_of(rc), uL = left_of(ua), pL = left_of(p);
        S_ gus, gps;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const T rc_l = rcL[k], rc_r = rc[k];
            const Den d(rc_l + rc_r);
            gus.v[k] = d.quo_t(rc_l * uL[k] + rc_r * ua[k] + (pL[k] - p[k]));
            gps.v[k] = d.quo(rc_r * pL[k] + rc_l * p[k] + rc_l * rc_r * (uL[k] - ua[k]));
        }
        S_ fus, fps;
        if (S == 1) {
            // acoustic_GAD! (ref src/riemann_schemes.jl:84-104): cells i-s = left, i = own
            const Sh rhoL = left_of(rho);
            const Sh gusL = left_of(gus), gpsL = left_of(gps), gusR = right_of(gus), gpsR = right_of(gps);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T r_um = phys::limiter<LIM>(Den(gus[k] - uL[k] + T(1e-6)).quo_t(gusR[k] - ua[k]));
                const T r_pm = phys::limiter<LIM>(Den(gps[k] - pL[k] + T(1e-6)).quo(gpsR[k] - p[k]));
                const T r_up = phys::limiter<LIM>(Den(ua[k] - gus[k] + T(1e-6)).quo_t(uL[k] - gusL[k]));
                const T r_pp = phys::limiter<LIM>(Den(p[k] - gps[k] + T(1e-6)).quo(pL[k] - gpsL[k]));
                const T dm_l = rhoL[k] * dx;
                const T dm_r = rho[k] * dx;
                const T Dm = (dm_l + dm_r) / 2;
                const T theta = T(0.5) * (1 - (rcL[k] + rc[k]) / 2 * Den(Dm).quo(dt));
                fus.v[k] = gus[k] + theta * (r_up * (ua[k] - gus[k]) - r_um * (gus[k] - uL[k]));
                fps.v[k] = gps[k] + theta * (r_pp * (p[k] - gps[k]) - r_pm * (gps[k] - pL[k]));
            }
        } else {
            fus = gus;
            fps = gps;
        }
        // Lagrangian update (ref src/kernels.jl:58-68)
        const Sh fusR = right_of(fus), fpsR = right_of(fps);
        S_ l_rho, l_ua, l_E, dxl, q_ua, q_ut, q_E;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const T dm = rho[k] * dx;
            dxl.v[k] = dx + dt * (fusR[k] - fus[k]);
            l_rho.v[k] = Den(dxl[k]).quo(dm);
            const T dt_dm = Den(dm).quo(dt);
            l_ua.v[k] = ua[k] + dt_dm * (fps[k] - fpsR[k]);
            l_E.v[k] = E[k] + dt_dm * (fps[k] * fus[k] - fpsR[k] * fusR[k]);
            q_ua.v[k] = l_rho[k] * l_ua[k];
            q_ut.v[k] = l_rho[k] * ut[k];
            q_E.v[k] = l_rho[k] * l_E[k];
        }
        // advection flux on the low side of each cell
        S_ a0, a1, a2, a3;    // ρ, ρu, ρv, ρE
        [[maybe_unused]] S_ k_rm, k_rp, k_disp, k_lf;     // NS > 0: what the planes share with ρ (bounded: the displacement only)
        const Sh rL = left_of(l_rho), quL = left_of(q_ua), qvL = left_of(q_ut), qEL = left_of(q_E);
        if (W == 1) {
            const Sh rR = right_of(l_rho), quR = right_of(q_ua), qvR = right_of(q_ut), qER = right_of(q_E);
            const Sh dxlL = left_of(dxl), dxlR = right_of(dxl);
            S_ s0, s1, s2, s3;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T r_m = Den(dxl[k] + dxlL[k]).quo(2 * dxl[k]);
                const T r_p = Den(dxl[k] + dxlR[k]).quo(2 * dxl[k]);
                s0.v[k] = phys::slope_minmod(rL[k], l_rho[k], rR[k], r_m, r_p);
                s1.v[k] = phys::slope_minmod(quL[k], q_ua[k], quR[k], r_m, r_p);
                s2.v[k] = phys::slope_minmod(qvL[k], q_ut[k], qvR[k], r_m, r_p);
                s3.v[k] = phys::slope_minmod(qEL[k], q_E[k], qER[k], r_m, r_p);
                if constexpr (REMAP) {
                    k_rm.v[k] = r_m;
                    k_rp.v[k] = r_p;
                }
            }
            const Sh s0L = left_of(s0), s1L = left_of(s1), s2L = left_of(s2), s3L = left_of(s3);
            const Sh fusL = left_of(fus);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T disp = dt * fus[k];
                const bool up = disp > 0;
                const T Dxe = up ? -(dx - dt * fusL[k]) : (dx + dt * fusR[k]);
                const T lf = Den(2 * (up ? dxlL[k] : dxl[k])).quo(Dxe);
                a0.v[k] = disp * ((up ? rL[k] : l_rho[k]) - (up ? s0L[k] : s0[k]) * lf);
                a1.v[k] = disp * ((up ? quL[k] : q_ua[k]) - (up ? s1L[k] : s1[k]) * lf);
                a2.v[k] = disp * ((up ? qvL[k] : q_ut[k]) - (up ? s2L[k] : s2[k]) * lf);
                a3.v[k] = disp * ((up ? qEL[k] : q_E[k]) - (up ? s3L[k] : s3[k]) * lf);
                if constexpr (NS > 0) k_disp.v[k] = disp;
                if constexpr (REMAP) k_lf.v[k] = lf;
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T disp = dt * fus[k];
                const bool up = disp > 0;
                a0.v[k] = disp * (up ? rL[k] : l_rho[k]);
                a1.v[k] = disp * (up ? quL[k] : q_ua[k]);
                a2.v[k] = disp * (up ? qvL[k] : q_ut[k]);
                a3.v[k] = disp * (up ? qEL[k] : q_E[k]);
                if constexpr (NS > 0) k_disp.v[k] = disp;
            }
        }
        // projection (ref src/projection_schemes.jl:23-41)
        const Sh a0R = right_of(a0), a1R = right_of(a1), a2R = right_of(a2), a3R = right_of(a3);
#pragma unroll
        for (int k = 0; k < K; k++) {
            const T dX = dxl[k];
            const T t_rho  = d_dx.quo(dX * l_rho[k]           - (a0R[k] - a0[k]));
            const T t_urho = d_dx.quo_t(dX * l_rho[k] * l_ua[k] - (a1R[k] - a1[k]));
            const T t_vrho = d_dx.quo_t(dX * l_rho[k] * ut[k]   - (a2R[k] - a2[k]));
            const T t_Erho = d_dx.quo(dX * l_rho[k] * l_E[k]  - (a3R[k] - a3[k]));
            const Den d_rho(t_rho);
            o_rho.v[k] = t_rho;
            o_u.v[k] = d_rho.quo_t(t_urho);
            o_v.v[k] = d_rho.quo_t(t_vrho);
            o_E.v[k] = d_rho.quo(t_Erho);
        }
        // the planes, one after the other: the t_vrho / o_v lines with φ for ut
        if constexpr (REMAP) {
#pragma unroll
            for (int n = 0; n < NS; n++) {
                S_ q, a;
#pragma unroll
                for (int k = 0; k < K; k++) q.v[k] = l_rho[k] * phi[n][k];
                const Sh qL = left_of(q);
                if (W == 1) {
                    const Sh qR = right_of(q);
                    S_ s;
#pragma unroll
                    for (int k = 0; k < K; k++) s.v[k] = phys::slope_minmod(qL[k], q[k], qR[k], k_rm[k], k_rp[k]);
                    const Sh sL = left_of(s);
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const bool up = k_disp[k] > 0;
                        a.v[k] = k_disp[k] * ((up ? qL[k] : q[k]) - (up ? sL[k] : s[k]) * k_lf[k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < K; k++) a.v[k] = k_disp[k] * (k_disp[k] > 0 ? qL[k] : q[k]);
                }
                const Sh aR = right_of(a);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const T t_q = d_dx.quo_t(dxl[k] * l_rho[k] * phi[n][k] - (aR[k] - a[k]));
                    o_phi[n].v[k] = Den(o_rho[k]).quo_t(t_q);
                }
            }
        }
        // the planes per unit mass (§4.17), one after the other: the mass and the weight ½(1 − ν) of every interface once
        if constexpr (BOUNDED) {
            S_ m, h;
#pragma unroll
            for (int k = 0; k < K; k++) m.v[k] = dxl[k] * l_rho[k];
            if (W == 1) {
                const Sh mL = left_of(m);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const T nu = Den(k_disp[k] > 0 ? mL[k] : m[k]).quo_t(phys::abs_(a0[k]));
                    h.v[k] = T(0.5) * (1 - nu);
                }
            }
#pragma unroll
            for (int n = 0; n < NS; n++) {
                const Sh fL = left_of(phi[n]), fR = right_of(phi[n]);
                S_ a;
                if (W == 1) {
                    S_ s;
#pragma unroll
                    for (int k = 0; k < K; k++) s.v[k] = phys::slope_minmod(fL[k], phi[n][k], fR[k], T(1.), T(1.));
                    const Sh sL = left_of(s);
#pragma unroll
                    for (int k = 0; k < K; k++)
                        a.v[k] = a0[k] * (k_disp[k] > 0 ? fL[k] + sL[k] * h[k] : phi[n][k] - s[k] * h[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < K; k++) a.v[k] = a0[k] * (k_disp[k] > 0 ? fL[k] : phi[n][k]);
                }
                const Sh aR = right_of(a);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const T t_q = d_dx.quo_t(m[k] * phi[n][k] - (aR[k] - a[k]));
                    const T lo = phys::mn(phys::mn(fL[k], phi[n][k]), fR[k]), hi = phys::mx(phys::mx(fL[k], phi[n][k]), fR[k]);
                    const T v = Den(o_rho[k]).quo_t(t_q);
                    o_phi[n].v[k] = v < lo ? lo : (v > hi ? hi : v);              // (by comparisons: a NaN stays one)
                }
            }
        }
    }

    // ---------------------------------------------------------------------------------------------
    __device__ __forceinline__ void run_fast(const S_& rho, const S_& ua, const S_& ut, const S_& E,
                                             S_& o_rho, S_& o_u, S_& o_v, S_& o_E, S_& p, S_& cs,
                                             const S_* phi = nullptr, S_* o_phi = nullptr) const
    {
        const T gm1 = gamma - T(1.), ggm1 = gamma * (gamma - T(1.));
        S_ rc;
#pragma unroll
        for (int k = 0; k < K; k++) fast::eos<EOS>(gm1, ggm1, rho[k], ua[k], ut[k], E[k], p.v[k], cs.v[k], rc.v[k]);
        const Sh rcL = left_of(rc), uL = left_of(ua), pL = left_of(p);
        S_ gus, gps, src;
#pragma unroll
        for (int k = 0; k < K; k++) fast::solve(rcL[k], uL[k], pL[k], rc[k], ua[k], p[k], gus.v[k], gps.v[k], src.v[k]);
        S_ fus, fps;
        if (S == 1) {
            const Sh rhoL = left_of(rho);
            const Sh gusL = left_of(gus), gpsL = left_of(gps), gusR = right_of(gus), gpsR = right_of(gps);
#pragma unroll
            for (int k = 0; k < K; k++)
                fast::gad<LIM>(dt_dx, rhoL[k], uL[k], pL[k], rho[k], ua[k], p[k], src[k],
                               gusL[k], gpsL[k], gus[k], gps[k], gusR[k], gpsR[k], fus.v[k], fps.v[k]);
        } else {
            fus = gus;
            fps = gps;
        }
        S_ dtu, pu;
#pragma unroll
        for (int k = 0; k < K; k++) fast::flux_products(dt, fus[k], fps[k], dtu.v[k], pu.v[k]);
        const Sh dtuR = right_of(dtu), fpsR = right_of(fps), puR = right_of(pu);
        S_ l_rho, dxl, hinv, q_ua, q_ut, q_E;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const fast::Lag<T> n = fast::lagrange(dx, dt_dx, rho[k], ua[k], ut[k], E[k], fps[k], dtu[k], pu[k],
                                                  fpsR[k], dtuR[k], puR[k]);
            dxl.v[k] = n.dxl;
            hinv.v[k] = n.hinv;
            l_rho.v[k] = n.rho;
            q_ua.v[k] = n.q_ua;
            q_ut.v[k] = n.q_ut;
            q_E.v[k] = n.q_E;
        }
        S_ a0, a1, a2, a3;
        [[maybe_unused]] S_ k_rm, k_rp, k_lf;     // NS > 0, remap: what the planes share with ρ
        const Sh rL = left_of(l_rho), quL = left_of(q_ua), qvL = left_of(q_ut), qEL = left_of(q_E);
        if (W == 1) {
            const Sh rR = right_of(l_rho), quR = right_of(q_ua), qvR = right_of(q_ut), qER = right_of(q_E);
            // a cell's Δx + Δx₊ is its right neighbour's Δx₋ + Δx (the same bits: IEEE addition commutes), so every cell
            // inverts ONE sum and takes the other reciprocal from its neighbour (one shift instead of a second
            // v_rcp_f64, which issues at a quarter of an FMA's rate)
            const Sh dxlL = left_of(dxl);
            S_ isum;
#pragma unroll
            for (int k = 0; k < K; k++) isum.v[k] = fast::inv_pair_length(dxl[k], dxlL[k]);
            const Sh isumR = right_of(isum);
            S_ s0, s1, s2, s3;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T r_m = fast::slope_ratio(dxl[k], isum[k]), r_p = fast::slope_ratio(dxl[k], isumR[k]);
                s0.v[k] = fast::slope(r_p, rR[k], l_rho[k], r_m, rL[k]);
                s1.v[k] = fast::slope(r_p, quR[k], q_ua[k], r_m, quL[k]);
                s2.v[k] = fast::slope(r_p, qvR[k], q_ut[k], r_m, qvL[k]);
                s3.v[k] = fast::slope(r_p, qER[k], q_E[k], r_m, qEL[k]);
                if constexpr (REMAP) {
                    k_rm.v[k] = r_m;
                    k_rp.v[k] = r_p;
                }
            }
            const Sh s0L = left_of(s0), s1L = left_of(s1), s2L = left_of(s2), s3L = left_of(s3);
            const Sh dtuL = left_of(dtu), hinvL = left_of(hinv);
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T disp = dtu[k];
                const bool up = disp > 0;                 // donor: the cell on the left when the interface moves up
                const T Dxe = up ? fast::extent_up(dtuL[k], dx) : fast::extent_dn(dx, dtuR[k]);
                const T lf = fast::donor_reach(Dxe, up ? hinvL[k] : hinv[k]);
                a0.v[k] = fast::advect2(disp, lf, -(up ? s0L[k] : s0[k]), up ? rL[k] : l_rho[k]);
                a1.v[k] = fast::advect2(disp, lf, -(up ? s1L[k] : s1[k]), up ? quL[k] : q_ua[k]);
                a2.v[k] = fast::advect2(disp, lf, -(up ? s2L[k] : s2[k]), up ? qvL[k] : q_ut[k]);
                a3.v[k] = fast::advect2(disp, lf, -(up ? s3L[k] : s3[k]), up ? qEL[k] : q_E[k]);
                if constexpr (REMAP) k_lf.v[k] = lf;
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const T disp = dtu[k];
                const bool up = disp > 0;
                a0.v[k] = fast::advect1(disp, up ? rL[k] : l_rho[k]);
                a1.v[k] = fast::advect1(disp, up ? quL[k] : q_ua[k]);
                a2.v[k] = fast::advect1(disp, up ? qvL[k] : q_ut[k]);
                a3.v[k] = fast::advect1(disp, up ? qEL[k] : q_E[k]);
            }
        }
        const Sh a0R = right_of(a0), a1R = right_of(a1), a2R = right_of(a2), a3R = right_of(a3);
#pragma unroll
        for (int k = 0; k < K; k++) {
            const T q[4] = {l_rho[k], q_ua[k], q_ut[k], q_E[k]};
            const T a[4] = {a0[k], a1[k], a2[k], a3[k]}, aR[4] = {a0R[k], a1R[k], a2R[k], a3R[k]};
            fast::project(inv_dx, dxl[k], q, a, aR, o_rho.v[k], o_u.v[k], o_v.v[k], o_E.v[k]);
        }
        // the planes, one after the other: the stages of ρ·ut with q = ρ_lag·φ (fast::lagrange's q_ut) in its slot
        if constexpr (REMAP) {
#pragma unroll
            for (int n = 0; n < NS; n++) {
                S_ q, a;
#pragma unroll
                for (int k = 0; k < K; k++) q.v[k] = l_rho[k] * phi[n][k];
                const Sh qL = left_of(q);
                if (W == 1) {
                    const Sh qR = right_of(q);
                    S_ s;
#pragma unroll
                    for (int k = 0; k < K; k++) s.v[k] = fast::slope(k_rp[k], qR[k], q[k], k_rm[k], qL[k]);
                    const Sh sL = left_of(s);
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const bool up = dtu[k] > 0;
                        a.v[k] = fast::advect2(dtu[k], k_lf[k], -(up ? sL[k] : s[k]), up ? qL[k] : q[k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < K; k++) a.v[k] = fast::advect1(dtu[k], dtu[k] > 0 ? qL[k] : q[k]);
                }
                const Sh aR = right_of(a);
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const T qq[4] = {l_rho[k], q[k], q[k], q[k]};            // the other two slots are not used
                    const T al[4] = {a0[k], a[k], a[k], a[k]}, ah[4] = {a0R[k], aR[k], aR[k], aR[k]};
                    T t_rho, t_u, t_E;
                    fast::project(inv_dx, dxl[k], qq, al, ah, t_rho, t_u, o_phi[n].v[k], t_E);
                }
            }
        }
        // the planes per unit mass (§4.17), one after the other: the stages of sweep_stages.hpp's bounded transport
        if constexpr (BOUNDED) {
            S_ m, h, irho;
#pragma unroll
            for (int k = 0; k < K; k++) {
                m.v[k] = dxl[k] * l_rho[k];
                irho.v[k] = fast::rcp(fast::fma_(dxl[k], l_rho[k], a0[k] - a0R[k]));     // 1 / T_ρ, as fast::project forms it
            }
            if (W == 1) {
                S_ im;
#pragma unroll
                for (int k = 0; k < K; k++) im.v[k] = fast::inv_mass(m[k]);
                const Sh imL = left_of(im);
#pragma unroll
                for (int k = 0; k < K; k++) h.v[k] = fast::leaving_weight(a0[k], dtu[k] > 0 ? imL[k] : im[k]);
            }
#pragma unroll
            for (int n = 0; n < NS; n++) {
                const Sh fL = left_of(phi[n]), fR = right_of(phi[n]);
                S_ a;
                if (W == 1) {
                    S_ s;
#pragma unroll
                    for (int k = 0; k < K; k++) s.v[k] = fast::minmod(fR[k] - phi[n][k], phi[n][k] - fL[k]);
                    const Sh sL = left_of(s);
#pragma unroll
                    for (int k = 0; k < K; k++) {
                        const bool up = dtu[k] > 0;
                        a.v[k] = fast::carry2(a0[k], h[k], up ? sL[k] : -s[k], up ? fL[k] : phi[n][k]);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < K; k++) a.v[k] = fast::carry1(a0[k], dtu[k] > 0 ? fL[k] : phi[n][k]);
                }
                const Sh aR = right_of(a);
#pragma unroll
                for (int k = 0; k < K; k++)
                    o_phi[n].v[k] = fast::settle(m[k], irho[k], phi[n][k], a[k], aR[k], fL[k], fR[k]);
            }
        }
    }
};

}  // namespace fused
}  // namespace armon
