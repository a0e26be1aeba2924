// sweep_stages.hpp — the tuned arithmetic of the fused directional sweep, one function per stage, and its primitives.
//
// A sweep runs seven stages per cell: EOS → first-order interface solve → GAD limited flux → Lagrangian cell update →
// limited slopes → advection flux → Euler projection (ref src/solver.jl:300-316). For the tuned flavour (shared 1-ulp
// reciprocals instead of IEEE divisions, explicit FMAs, algebraically equivalent regrouping; agrees with the exact
// flavour to rounding) each stage is stated here ONCE, as a function from values to values: no ring, no lane shift, no
// index. The two forms of the sweep — the march (PipeFast, sweep_pipeline.hpp: operands from the ring slots of earlier
// steps) and the spatial form (SpatialSweep::run_fast, sweep_spatial.hpp: operands from the neighbouring lanes) — only
// fetch operands, call the stage and put the results away, so they are the same function of the state. Generic in the
// working type (double, float, or float2v: two fp32 cells per lane). What a form prepares in its own way for measured
// reasons — a reciprocal or a difference it keeps from the previous step or takes from the next lane, the choice of the
// upwind donor's operands — is an argument of the stage. The exact flavour is not here: Pipe and run_exact state it.
#pragma once

#include "physics.hpp"

namespace armon {
namespace fused {

namespace fast {

// 1/x to ≈1 ulp: v_rcp_f64 (2^-24) + two Newton steps. No scaling/fixup: operands here are O(1) state.
__device__ __forceinline__ double rcp(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, e, r);
}
__device__ __forceinline__ float rcp(float x) { return __builtin_amdgcn_rcpf(x); }     // v_rcp_f32: 1 ulp

// 1/x to ≈2e-15 (one Newton step): for the reciprocals that only feed second-order correction terms
// (limited GAD ratios, θ, slope ratios), where a relative error of 1e-15 is far below their truncation error.
__device__ __forceinline__ double rcp1(double x)
{
    const double r = __builtin_amdgcn_rcp(x);
    return __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
}
__device__ __forceinline__ float rcp1(float x) { return __builtin_amdgcn_rcpf(x); }

// sqrt(x) to ≈1-2 ulp: v_rsq_f64 + two coupled Newton (Goldschmidt) steps; sqrt(0) = 0.
__device__ __forceinline__ double sqrt_(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    r = __builtin_fma(-g, h, 0.5);
    g = __builtin_fma(g, r, g);
    return (x == 0.) ? 0. : g;
}
__device__ __forceinline__ float sqrt_(float x) { return __builtin_amdgcn_sqrtf(x); }      // v_sqrt_f32: 1 ulp, no denormal scaling (operands are O(1) energies)

// Two fp32 cells per lane as ONE 64-bit value (the tuned fp32 Y march, k_sweep_y with two columns per lane): elementwise arithmetic on this type is
// v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 — one instruction for both cells — where two scalar pipelines side by side
// left the pairing to the compiler's SLP pass (which found about half of it and paid for the rest in v_mov shuffles).
// Same IEEE operations per component, hence the same bits as the scalar pipeline.
typedef float float2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2v rcp(float2v x) { return float2v{__builtin_amdgcn_rcpf(x.x), __builtin_amdgcn_rcpf(x.y)}; }
__device__ __forceinline__ float2v rcp1(float2v x) { return rcp(x); }
__device__ __forceinline__ float2v sqrt_(float2v x) { return float2v{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)}; }
__device__ __forceinline__ float2v fma_(float2v a, float2v b, float2v c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ float2v max_(float2v a, float2v b) { return float2v{__builtin_fmaxf(a.x, b.x), __builtin_fmaxf(a.y, b.y)}; }
__device__ __forceinline__ float2v min_(float2v a, float2v b) { return float2v{__builtin_fminf(a.x, b.x), __builtin_fminf(a.y, b.y)}; }
// component-wise choice; `m` is the result of a comparison (bool for a scalar, an integer vector for float2v)
template <class M, class T> __device__ __forceinline__ T sel(M m, T a, T b) { return m ? a : b; }
// the scalar type behind a working type: uniform parameters (dt, dx, γ …) stay scalars (SGPRs) next to vector state
template <typename T> struct scalar_of { using type = T; };
template <> struct scalar_of<float2v> { using type = float; };

__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double max_(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float max_(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double min_(double a, double b) { return __builtin_fmin(a, b); }
__device__ __forceinline__ float min_(float a, float b) { return __builtin_fminf(a, b); }

template <int LIM, typename T>
__device__ __forceinline__ T limiter(T r)
{
    if (LIM == ARMON_LIMITER_MINMOD) return max_(T(0.), min_(T(1.), r));
    if (LIM == ARMON_LIMITER_SUPERBEE) return max_(max_(T(0.), min_(T(2.) * r, T(1.))), min_(r, T(2.)));
    return T(1.);
}

// minmod(a, b) = sign·min(|a|,|b|) when a·b > 0, else 0  (== slope_minmod of ref projection_schemes.jl:15-20)
// = the median of (a, b, 0).
template <typename T>
__device__ __forceinline__ T minmod(T a, T b)
{
    return max_(min_(a, b), min_(max_(a, b), T(0.)));
}

// ref src/kernels.jl:16-55 with the four divisions by (1 - s·x) and the two by ρ shared, the polynomials in Horner
// form and every multiply-add an explicit FMA (the library is built with -ffp-contract=off: a plain a*b + c costs two
// instructions): 62 VALU instructions instead of 94.
template <typename T>
__device__ __forceinline__ void bizarrium(T rho, T ua, T ut, T E, T& p, T& cs)
{
    constexpr double rho0 = 10000., K0 = 1e+11, Cv0 = 1000., T0 = 300., eps0 = 0., G0 = 1.5, s_ = 1.5;
    constexpr double q = -42080895. / 14941154., rr = 727668333. / 149411540., a1 = s_ / 3. - 2.;
    const T inv_rho = rcp(rho);
    const T x = fma_(rho, T(1. / rho0), T(-1.));
    const T G = fma_(T(-G0 * rho0), inv_rho, T(G0));                         // G0 (1 - ρ0/ρ)
    const T x2 = x * x;
    const T opx = T(1.) + x, opx2 = opx * opx, opx3 = opx2 * opx;
    const T inv_d = rcp(fma_(T(-s_), x, T(1.)));
    const T f0 = fma_(fma_(fma_(T(rr), x, T(q)), x, T(a1)), x, T(1.)) * inv_d;                  // (1 + a1 x + q x² + r x³)/(1 - s x)
    const T f1 = fma_(T(s_), f0, fma_(fma_(T(3. * rr), x, T(2. * q)), x, T(a1))) * inv_d;       // (a1 + 2q x + 3r x² + s f0)/(1 - s x)
    const T f2 = fma_(T(2. * s_), f1, fma_(T(6. * rr), x, T(2. * q))) * inv_d;                  // (2q + 6r x + 2s f1)/(1 - s x)
    // ε_k0 = ε0 - Cv0 T0 (1 + G) + ½ (K0/ρ0) x² f0
    const T epsk0 = fma_(T(0.5 * K0 / rho0) * x2, f0, fma_(T(-Cv0 * T0), G, T(eps0 - Cv0 * T0)));
    // p_k0 = -Cv0 T0 G0 ρ0 + ½ K0 x (1+x)² (2 f0 + x f1)
    const T pk0 = fma_(T(0.5 * K0) * x * opx2, fma_(x, f1, T(2.) * f0), T(-Cv0 * T0 * G0 * rho0));
    // p_k0' = -½ K0 (1+x)³ ρ0 (2 (1+3x) f0 + 2x (2+3x) f1 + x² (1+x) f2)
    const T inner = fma_(fma_(T(6.), x, T(2.)), f0, fma_(x * fma_(T(6.), x, T(4.)), f1, x2 * opx * f2));
    const T pk0prime = T(-0.5 * K0 * rho0) * opx3 * inner;
    const T e = fma_(T(-0.5), fma_(ua, ua, ut * ut), E);
    const T w = T(G0 * rho0) * (e - epsk0);                                  // = p - p_k0
    p = pk0 + w;
    cs = sqrt_(fma_(T(G0 * rho0), w, -pk0prime)) * inv_rho;
}

// ---- the tuned stages. T: working type; Sc: its scalar (uniform parameters) ------------------------------------------

// EOS of one cell. Perfect gas: p = (γ-1)ρe, c = sqrt(γp/ρ) = sqrt(γ(γ-1)e), no division; gm1 = γ-1, ggm1 = γ(γ-1)
template <int EOS, typename T, typename Sc>
__device__ __forceinline__ void eos(Sc gm1, Sc ggm1, T rho, T ua, T ut, T E, T& p, T& cs, T& rc)
{
    if (EOS == ARMON_EOS_BIZARRIUM) {
        bizarrium(rho, ua, ut, E, p, cs);
    } else {
        const T e = fma_(T(-0.5), fma_(ua, ua, ut * ut), E);
        p = gm1 * rho * e;
        cs = sqrt_(ggm1 * e);
    }
    rc = rho * cs;
}

// first-order acoustic solve of the interface between cells l | r: one shared reciprocal; sum = rc_l + rc_r (→ gad)
template <typename T>
__device__ __forceinline__ void solve(T rc_l, T u_l, T p_l, T rc_r, T u_r, T p_r, T& us, T& ps, T& sum)
{
    sum = rc_l + rc_r;
    const T inv = rcp(sum);
    us = fma_(rc_l, u_l, fma_(rc_r, u_r, p_l - p_r)) * inv;
    ps = fma_(rc_r, p_l, fma_(rc_l, p_r, rc_l * rc_r * (u_l - u_r))) * inv;
}

// GAD limited flux of the interface l | r from its first-order solution (us_0, ps_0, sum) and those of the interfaces
// on its left (us_l, ps_l) and right (us_r, ps_r)
template <int LIM, typename T, typename Sc>
__device__ __forceinline__ void gad(Sc dt_dx, T rho_l, T u_l, T p_l, T rho_r, T u_r, T p_r, T sum,
                                    T us_l, T ps_l, T us_0, T ps_0, T us_r, T ps_r, T& us, T& ps)
{
    const T Au = us_0 - u_l, Bu = u_r - us_0;     // (uˢ_i - u[i-s]), (u[i] - uˢ_i)
    const T Ap = ps_0 - p_l, Bp = p_r - ps_0;
    const T r_um = limiter<LIM>((us_r - u_r) * rcp1(Au + T(1e-6)));
    const T r_pm = limiter<LIM>((ps_r - p_r) * rcp1(Ap + T(1e-6)));
    const T r_up = limiter<LIM>((u_l - us_l) * rcp1(Bu + T(1e-6)));
    const T r_pp = limiter<LIM>((p_l - ps_l) * rcp1(Bp + T(1e-6)));
    // θ = ½(1 - (rc_l+rc_r)/2 · dt/Dm), Dm = dx(ρ_l+ρ_r)/2  →  ½ - ½·(rc_l+rc_r)·(dt/dx)/(ρ_l+ρ_r)
    const T theta = fma_(T(-0.5) * sum * dt_dx, rcp1(rho_l + rho_r), T(0.5));
    us = fma_(theta, fma_(r_up, Bu, -r_um * Au), us_0);
    ps = fma_(theta, fma_(r_pp, Bp, -r_pm * Ap), ps_0);
}

// what the later stages take of a final flux: dt·uˢ and pˢ·uˢ
template <typename T, typename Sc>
__device__ __forceinline__ void flux_products(Sc dt, T us, T ps, T& dtu, T& pu)
{
    dtu = dt * us;
    pu = ps * us;
}

// Lagrangian state of a cell: q_* = ρ·(ua, ut, E); hinv = 0.5/dxl
template <typename T> struct Lag { T rho, q_ua, q_ut, q_E, dxl, hinv; };

// Lagrangian update of one cell from the fluxes on its low and high side; dt_dx = dt/dx
template <typename T, typename Sc>
__device__ __forceinline__ Lag<T> lagrange(Sc dx, Sc dt_dx, T rho, T ua, T ut, T E,
                                           T ps_lo, T dtu_lo, T pu_lo, T ps_hi, T dtu_hi, T pu_hi)
{
    Lag<T> n;
    const T dtdm = dt_dx * rcp(rho);                // dt / (ρ dx)
    const T dxl = (dx + dtu_hi) - dtu_lo;
    const T inv_dxl = rcp(dxl);
    n.dxl = dxl;
    n.hinv = T(0.5) * inv_dxl;
    n.rho = rho * dx * inv_dxl;
    const T ua_n = fma_(dtdm, ps_lo - ps_hi, ua);
    const T E_n = fma_(dtdm, pu_lo - pu_hi, E);
    n.q_ua = n.rho * ua_n;
    n.q_ut = n.rho * ut;
    n.q_E = n.rho * E_n;
    return n;
}

// 1 / (Δx + Δx') of two adjacent cells: the slope ratios of both share it
template <typename T> __device__ __forceinline__ T inv_pair_length(T dxl_a, T dxl_b) { return rcp1(dxl_a + dxl_b); }

// a slope ratio of a cell, r₊ = 2Δx/(Δx+Δx₊) or r₋ = 2Δx/(Δx+Δx₋), from the prepared reciprocal of the sum
template <typename T> __device__ __forceinline__ T slope_ratio(T dxl, T isum) { return T(2.) * dxl * isum; }

// limited slope of one quantity from its differences to the right (d_p) and left (d_m) neighbour
template <typename T> __device__ __forceinline__ T slope(T r_p, T d_p, T r_m, T d_m) { return minmod(r_p * d_p, r_m * d_m); }
// the same from the three values, for a form that does not keep the differences (each taken next to its product)
template <typename T> __device__ __forceinline__ T slope(T r_p, T r, T c, T r_m, T l) { return minmod(r_p * (r - c), r_m * (c - l)); }

// Advection flux of an interface that moves by disp = dt·uˢ. The donor is the cell on the upwind side (up = disp > 0: the
// cell on the left); choosing the donor's operands is fetching, and is the form's. Second order: the donor's slope acts
// over lf = Dxe · hinv, with hinv = 0.5/dxl of the donor and Dxe its signed extent: extent_up from dt·uˢ of the interface
// on the left of this one, extent_dn from that on the right (the spatial form evaluates the chosen one only)
template <typename T, typename Sc> __device__ __forceinline__ T extent_up(T dtu_l, Sc dx) { return dtu_l - dx; }
template <typename T, typename Sc> __device__ __forceinline__ T extent_dn(Sc dx, T dtu_r) { return dx + dtu_r; }
template <typename T> __device__ __forceinline__ T donor_reach(T Dxe, T hinv) { return Dxe * hinv; }
// one quantity q of the donor with ms = minus its limited slope (negated where it is fetched); first order: q alone
template <typename T> __device__ __forceinline__ T advect2(T disp, T lf, T ms, T q) { return disp * fma_(ms, lf, q); }
template <typename T> __device__ __forceinline__ T advect1(T disp, T q) { return disp * q; }

// Euler projection of one cell (q = ρ, ρu, ρv, ρE after the Lagrangian update) from the advection fluxes on its low
// and high side: (dX·q - ΔA)/dx, then u = ρu/ρ …: the 1/dx cancels in the three ratios
template <typename T, typename Sc>
__device__ __forceinline__ void project(Sc inv_dx, T dX, const T (&q)[4], const T (&a_lo)[4], const T (&a_hi)[4],
                                        T& o_rho, T& o_u, T& o_v, T& o_E)
{
    const T T_rho = fma_(dX, q[0], a_lo[0] - a_hi[0]);
    const T T_u = fma_(dX, q[1], a_lo[1] - a_hi[1]);
    const T T_v = fma_(dX, q[2], a_lo[2] - a_hi[2]);
    const T T_E = fma_(dX, q[3], a_lo[3] - a_hi[3]);
    const T inv = rcp(T_rho);
    o_rho = T_rho * inv_dx;
    o_u = T_u * inv;
    o_v = T_v * inv;
    o_E = T_E * inv;
}

// ---- bounded transport of a passive scalar φ (per unit mass) -------------------------------------------
// m = Δx_lag·ρ_lag is the mass of a Lagrangian cell, a the state's mass flux of an interface (advect1 / advect2 of ρ).
// 1/m to one Newton step: it only feeds ν, the weight of the second-order term
template <typename T> __device__ __forceinline__ T inv_mass(T m) { return rcp1(m); }
// ½(1 − ν), ν = |a|/m_d: where in the donor's profile the mean of the mass that leaves it sits, in units of its slope
template <typename T> __device__ __forceinline__ T leaving_weight(T a, T im_d) { return fma_(T(-0.5), max_(a, -a) * im_d, T(0.5)); }
// flux of φ: a·φ*, φ* = φ_d + ss·h with ss the donor's limited slope signed towards the interface; first order: a·φ_d
template <typename T> __device__ __forceinline__ T carry2(T a, T h, T ss, T phi_d) { return a * fma_(ss, h, phi_d); }
template <typename T> __device__ __forceinline__ T carry1(T a, T phi_d) { return a * phi_d; }
// φ' = (m φ + A_lo − A_hi) / T_ρ (irho = 1/T_ρ: the 1/dx cancels as in project), kept within φ of the cell and its neighbours
template <typename T>
__device__ __forceinline__ T settle(T m, T irho, T phi, T A_lo, T A_hi, T phi_l, T phi_r)
{
    const T v = fma_(m, phi, A_lo - A_hi) * irho;
    const T lo = min_(min_(phi_l, phi), phi_r), hi = max_(max_(phi_l, phi), phi_r);
    return sel(v < lo, lo, sel(v > hi, hi, v));                // (by comparisons: a NaN stays one)
}

}  // namespace fast

}  // namespace fused
}  // namespace armon
