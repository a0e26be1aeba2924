// sweep_x_kernel.hpp — the spatial X sweep of the fused sweep (k_sweep_x_dpp). Not a stand-alone header (see fused_sweep.hpp).
#pragma once
#include "sweep_device.hpp"

namespace {

// ---- X sweep, spatial form (lanes along x, DPP neighbour exchange) -------------------------------------
// blockDim = (64, kXSRows): one wave per row, kXSRows consecutive rows per workgroup. Each wave walks
// NITER strips of 64*K cells along its row; a strip yields 64*K - 2*HALO new cells.
#ifndef ARMON_XS_ROWS
#define ARMON_XS_ROWS 4          // rows (= waves) per workgroup of the X sweep (tuning macro)
#endif
constexpr int kXSRows = ARMON_XS_ROWS;
// ARMON_X_PRIO > 0: a new wave runs its prologue and issues its strip's loads at that priority (s_setprio), ahead of the
// arithmetic of the older waves of its SIMD, and drops to 0 for its own arithmetic: with four waves per SIMD and ~600 vector
// instructions per strip, a newcomer otherwise waits its turn behind three compute phases before anything of its own is in
// flight. Bizarrium (the longest compute phase) 2.91 -> 2.82 ms at 16384², the copy's rate; perfect gas, already at that
// rate, unchanged (profiles/r04_ab_x_prologue.txt).
#ifndef ARMON_X_PRIO
#define ARMON_X_PRIO 3
#endif
// One strip per wave (SINGLE): load, sweep, store, exit — no second register set for a prefetched strip, 104-119 VGPRs, 4
// waves per SIMD; the other waves of the SIMD hide the load. Rounds 1-2 ran TWO strips per wave with the second one's 32
// input registers prefetched during the first (166-184 VGPRs, 2-3 waves per SIMD): A/B in one process
// (profiles/r03_ab_x_single_strip.txt) tuned 2.875 -> 2.817 ms, tuned with dt tracking 3.240 -> 2.923 (2 -> 4 waves), exact
// 3.444 -> 3.083, exact with tracking 3.818 -> 3.435, a 4096 x 8192 tile 0.415 -> 0.367. The multi-strip form stays in
// the A/B build only (-DARMON_ALT_KERNELS, knob ARMON_XS_NITER > 1).
constexpr int kXSNiter = 1;
// ROW = 1 (with K = 1): the NARROW form for the LAG-wide boundary strips of a tile (partial sweeps of <= 8 cells along x,
// which follow the halo exchange): a wave holds FOUR rows of 16 lanes instead of one row of 64 or 128 cells, neighbours by
// row_shr / row_shl shifts. A 4-cell strip then costs 16 loaded cells per row instead of 128 (a strip of a 4096-cell-wide
// tile: 3 % of the whole sweep -> 0.4 %). Same arithmetic per cell, hence the same bits.
template <int SCHEME, int LIM, int PROJ, int EOS, bool EXACT, int K, bool TRACK, bool SINGLE, int ROW = 0>
__device__ __forceinline__ void sweep_x_dpp_body(const sweep_args& a, int niter)
{
    using SW = fused::SpatialSweep<SCHEME, LIM, PROJ, EOS, EXACT, K, real, ROW>;
    using St = fused::Strip<K, real>;
    constexpr int LAG = SW::LAG;
    static_assert(ROW == 0 || K == 1, "the narrow form holds one cell per lane");
    // K = 2: 4 cells whatever the scheme (LAG <= 4), so that STRIDE = 120 cells = 15 whole 64-B sectors and every
    // strip's stores stay sector-aligned (Godunov + euler, LAG 2: -5.6 % time against HALO = 2, STRIDE = 124)
    constexpr int HALO = (K == 1) ? LAG : 4;
    static_assert(LAG <= 4, "strip halo");
    constexpr int WIDTH = ROW ? 16 : 64 * K;
    constexpr int STRIDE = WIDTH - 2 * HALO;
    constexpr int RW = ROW ? 4 : 1;                           // rows per wave

    const int lane = ROW ? (threadIdx.x & 15) : threadIdx.x;  // position in the strip
    // XCD-aware placement of the workgroups: consecutive workgroup ids go round-robin to the 8 XCDs (each with its own
    // L2), so with the plain mapping two strips that are neighbours along x — they share their 4-cell halos — always
    // sit on different XCDs and both fetch the shared sectors from HBM. Within every group of 8 rows of workgroups,
    // XCD k (ids ≡ k mod 8) gets the whole row k: neighbouring strips then follow each other on the same L2.
    unsigned vbx = blockIdx.x, vby = blockIdx.y;
    if (a.xcd_remap) {
        const unsigned G = (unsigned)a.gx, chunk = vby & ~7u;
        if (chunk + 8 <= (unsigned)a.gy) {                     // whole groups only: the last rows keep the plain mapping
            const unsigned local = (vby - chunk) * G + vbx;    // 0 .. 8G-1 in dispatch order
            vby = chunk + (local & 7u);
            vbx = local >> 3;
        }
    }
    // Which strip and row a wave takes. a.x_wg_along_x: the kXSRows waves of a workgroup take kXSRows CONSECUTIVE STRIPS of
    // ONE row (the 128-B lines two neighbouring strips share — a strip's loads start 32 B before its sector-aligned stores —
    // are then fetched once per workgroup, from its CU's L1, instead of by two workgroups on two XCDs); otherwise one strip
    // of kXSRows consecutive rows (the narrow form, blocks of more than 65535 rows, the A/B forms).
    const bool along_x = SINGLE && ROW == 0 && a.x_wg_along_x;
    const int64_t strip0 = along_x ? (int64_t)vbx * kXSRows + threadIdx.y : (int64_t)vbx * niter;
    const int64_t row_r = along_x ? (int64_t)vby
                                  : ((int64_t)vby * kXSRows + threadIdx.y) * RW + (ROW ? (threadIdx.x >> 4) : 0);
    const bool row_ok = row_r < a.ny;                         // whole wave (ROW: a row of 16 lanes)
    const int64_t row = row_ok ? row_r : a.ny - 1;
    // the row in the arrays the sweep reads and in those it writes: one pitch for a plain sweep, two for the pair's X sweep,
    // whose output is the intermediate of whole lines per row (armon_hip_sweep_pair)
    const int64_t row_in = (row + a.g) * a.row_len + a.g;
    const int64_t row_off = (row + a.g) * a.out_len + a.g;
    const real* in[4] = {a.rho_in + row_in, a.ua_in + row_in, a.ut_in + row_in, a.E_in + row_in};
    real* out[4] = {a.rho_out + row_off, a.ua_out + row_off, a.ut_out + row_off, a.E_out + row_off};
    // 16-B accesses need every lane pair on an even cell of an even-pitched row; strip origins are multiples of 8 cells
    // from the row start (x_first), so an odd o_lo (partial sweeps with LAG = 3) only masks half of one pair
    bool vec_ok = (K == 2) && (a.out_len % 2 == 0) && ((a.x_first + a.g) % 2 == 0);         // uniform: the stores
    bool vec_in = (K == 2) && (a.row_len % 2 == 0) && ((a.x_first + a.g) % 2 == 0);         // uniform: the loads
    // When the row pitch is not a multiple of a sector (8 doubles, 16 floats) the rows start at different places of their 64-B sectors and no single
    // origin aligns them all (fp64 at 16388 cells per row: X 1.05x the copy, profiles/r03_row_pitch.txt): the origin is then
    // taken row by row, less than a sector below o_lo, where that row's stores start on a sector (arrays start on one). Every
    // lane pair then sits on 16 B (fp32: 8 B) whatever the parity of the pitch.
    int64_t x_first = a.x_first;
    if (ROW == 0 && a.x_row_align) {
        // (a wave's row is uniform, which the compiler cannot know: without readfirstlane every strip index below becomes
        // 64-bit vector arithmetic — +3 % on the VALU-bound exact flavour)
        x_first = a.o_lo - __builtin_amdgcn_readfirstlane((int)(row_off + a.o_lo) & (64 / (int)sizeof(real) - 1));
        vec_ok = (K == 2);
        // (the stores decide the origin; with one pitch the loads sit on the same 16 B)
        vec_in = (K == 2) && __builtin_amdgcn_readfirstlane((int)(row_in + x_first) & 1) == 0;
    }

    SW sw{a.dt, a.dx, a.gamma, a.inv_dx, a.dt_dx};
    cfl_track cfl;
    // Strip origins are aligned so that a strip's stores start on a 64-B sector of the ghosted row (for the
    // usual STRIDE = 120 = 15 sectors); the first strip of a row is then a short one (stores masked below o_lo).
    const int64_t w_first = x_first + strip0 * STRIDE;
    // Strips are real-buffered in registers: the loads of strip it+1 are issued before strip it is
    // computed (the loop is unrolled by the two buffers, so no loaded register is ever copied).
    St buf[2][4];
    auto load_strip = [&](auto slot, int it) {
        constexpr int B = decltype(slot)::value;
        St& rho = buf[B][0];
        St& ua = buf[B][1];
        St& ut = buf[B][2];
        St& E = buf[B][3];
        const int64_t cb = w_first + (int64_t)it * STRIDE - HALO;     // first cell of the strip
        const int64_t j0 = cb + (int64_t)lane * K;                    // this lane's first cell
        const bool interior = cb >= 0 && cb + WIDTH <= a.nx;          // uniform: no ghost, no clamping
        if (interior && (K == 1 || vec_in)) {
            if (K == 2) {
                constexpr bool NT = x_nt_loads(EOS, EXACT);
                const vec2 r = ld2<NT>(in[0] + j0);
                const vec2 u = ld2<NT>(in[1] + j0);
                const vec2 v = ld2<NT>(in[2] + j0);
                const vec2 e = ld2<NT>(in[3] + j0);
                rho.v[0] = r.x; rho.v[K - 1] = r.y;
                ua.v[0] = u.x; ua.v[K - 1] = u.y;
                ut.v[0] = v.x; ut.v[K - 1] = v.y;
                E.v[0] = e.x; E.v[K - 1] = e.y;
            } else {
                rho.v[0] = in[0][j0]; ua.v[0] = in[1][j0]; ut.v[0] = in[2][j0]; E.v[0] = in[3][j0];
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                // clamp into the block (ghosts included), then mirror physical boundaries
                int64_t j = j0 + k;
                j = j < -(int64_t)a.g ? -(int64_t)a.g : (j > a.nx + a.g - 1 ? a.nx + a.g - 1 : j);
                real fa, ft;
                const int64_t src = bc_source(a, a.nx, j, fa, ft);
                rho.v[k] = in[0][src];
                ua.v[k] = in[1][src] * fa;
                ut.v[k] = in[2][src] * ft;
                E.v[k] = in[3][src];
            }
        }
    };
    auto strip_exists = [&](int it) { return it < niter && w_first + (int64_t)it * STRIDE < a.o_hi; };
    auto do_strip = [&](auto slot, int it) {
        constexpr int B = decltype(slot)::value;
        if (!SINGLE && strip_exists(it + 1)) load_strip(std::integral_constant<int, 1 - B>{}, it + 1);
        const int64_t w0 = w_first + (int64_t)it * STRIDE;    // first cell this strip produces
        const int64_t j0 = w0 - HALO + (int64_t)lane * K;

        St o_rho, o_u, o_v, o_E, p, cs;
#ifdef ARMON_PROBE_NOCOMPUTE
        o_rho = buf[B][0]; o_u = buf[B][1]; o_v = buf[B][2]; o_E = buf[B][3]; p = buf[B][0]; cs = buf[B][0];
#else
        sw.run(buf[B][0], buf[B][1], buf[B][2], buf[B][3], o_rho, o_u, o_v, o_E, p, cs);
#endif

        // cells this lane may store: inside the strip's valid window and inside the block
        const int64_t hi = (w0 + STRIDE < a.o_hi) ? w0 + STRIDE : a.o_hi;
        const int64_t lo = w0 > a.o_lo ? w0 : a.o_lo;
        if (K == 2 && vec_ok && j0 >= lo && j0 + 1 < hi) {
            st2(out[0] + j0, o_rho.v[0], o_rho.v[K - 1]);
            st2(out[1] + j0, o_u.v[0], o_u.v[K - 1]);
            st2(out[2] + j0, o_v.v[0], o_v.v[K - 1]);
            st2(out[3] + j0, o_E.v[0], o_E.v[K - 1]);
            if (a.emit) {
                if (a.emit & 1) st2(a.p_out + row_off + j0, p.v[0], p.v[K - 1]);
                if (a.emit & 2) st2(a.c_out + row_off + j0, cs.v[0], cs.v[K - 1]);
            }
            if (TRACK) {
                cfl.add(o_u.v[0], o_v.v[0], cs.v[0]);
                cfl.add(o_u.v[K - 1], o_v.v[K - 1], cs.v[K - 1]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int64_t j = j0 + k;
                if (j >= lo && j < hi) {
                    out[0][j] = o_rho.v[k];
                    out[1][j] = o_u.v[k];
                    out[2][j] = o_v.v[k];
                    out[3][j] = o_E.v[k];
                    if (a.emit & 1) (a.p_out + row_off)[j] = p.v[k];
                    if (a.emit & 2) (a.c_out + row_off)[j] = cs.v[k];
                    if (TRACK) cfl.add(o_u.v[k], o_v.v[k], cs.v[k]);
                }
            }
        }
    };
    if (SINGLE) {
        if (row_ok && strip_exists(0)) {
            load_strip(std::integral_constant<int, 0>{}, 0);
#if ARMON_X_PRIO
            __builtin_amdgcn_s_setprio(0);
#endif
            do_strip(std::integral_constant<int, 0>{}, 0);
        }
    } else if (row_ok && strip_exists(0)) {
        load_strip(std::integral_constant<int, 0>{}, 0);
#if ARMON_X_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        for (int it = 0; strip_exists(it); it += 2) {
            do_strip(std::integral_constant<int, 0>{}, it);
            if (!strip_exists(it + 1)) break;
            do_strip(std::integral_constant<int, 1>{}, it + 1);
        }
    }
    // The waves of this kernel are short-lived (2 strips): a block-level LDS reduction + one partial per block cost
    // more than the strips themselves (282k blocks at 16384²: +1.1 ms), and atomic maxima into shared slots go to the
    // memory side on this part (2.3 M of them: +0.5 ms). Each wave simply stores its two maxima in its own slot
    // (18 MB at 16384², 0.1 % of the sweep's traffic); fold_dt_launch reduces them in two levels.
    if (TRACK) {
        const real au = red::wave_reduce<red::op_max>(cfl.au), av = red::wave_reduce<red::op_max>(cfl.av);
        if (threadIdx.x == 0) {
            const int64_t wave_id = ((int64_t)blockIdx.y * a.gx + blockIdx.x) * kXSRows + threadIdx.y;
            st2(a.partials + 2 * wave_id, au, av);
        }
    }
}

#ifndef ARMON_XS_WAVES
#define ARMON_XS_WAVES 1         // minimum waves per SIMD the X sweep is compiled for (tuning macro; 3 = cap at 168 VGPRs)
#endif
// hipcc loads a kernel argument from the kernarg segment in the basic block that first uses it: this kernel's prologue then
// holds FOUR dependent scalar-load round trips (st, the geometry, niter, the pointers) before its first vector load — and a
// wave of the one-strip form lives for one strip, so that latency is paid per strip with nothing of the wave's own in
// flight. Naming every field the hot path reads in one empty asm statement at entry makes the compiler issue all the
// s_loads together, behind ONE wait (ARMON_X_PRELOAD=0: the lazy form, for A/B).
#ifndef ARMON_X_PRELOAD
#define ARMON_X_PRELOAD 1
#endif
__device__ __forceinline__ void preload_x_args(const sweep_args& a, int niter)
{
#if ARMON_X_PRELOAD
    asm volatile("" ::"s"(a.nx), "s"(a.ny), "s"(a.row_len), "s"(a.out_len), "s"(a.g), "s"(a.bc_low), "s"(a.bc_high), "s"(a.emit), "s"(a.o_lo),
                 "s"(a.o_hi), "s"(a.x_first), "s"(a.xcd_remap), "s"(a.x_wg_along_x), "s"(a.x_row_align), "s"(niter), "s"(a.gx), "s"(a.gy));
    asm volatile("" ::"s"(a.dt), "s"(a.dx), "s"(a.gamma), "s"(a.inv_dx), "s"(a.dt_dx), "s"(a.rho_in), "s"(a.ua_in), "s"(a.ut_in),
                 "s"(a.E_in), "s"(a.rho_out), "s"(a.ua_out), "s"(a.ut_out), "s"(a.E_out));
#endif
}

template <int SCHEME, int LIM, int PROJ, int EOS, bool EXACT, int K, bool TRACK, bool SINGLE = true, int ROW = 0>
__global__ void __launch_bounds__(64 * kXSRows, ARMON_XS_WAVES)
k_sweep_x_dpp(sweep_args a, int niter)
{
#if ARMON_X_PRIO
    __builtin_amdgcn_s_setprio(ARMON_X_PRIO);     // until the strip's loads are issued (sweep_x_dpp_body lowers it again)
#endif
    preload_x_args(a, niter);
    if (!sweep_begin(a)) return;
    sweep_x_dpp_body<SCHEME, LIM, PROJ, EOS, EXACT, K, TRACK, SINGLE, ROW>(a, niter);
}

}  // namespace
