// fused_sweep.hpp — armon_hip_sweep: one directional sweep of solver_cycle (ref src/solver.jl:300-316)
// as ONE kernel launch: EOS → boundary mirror → fluxes → cell update → advection → projection, reading
// ρ,u,v,E once and writing them once (64 B per cell instead of the 352 B of the five staged passes),
// optionally followed by the dt/CFL reduction of the next cycle (ref src/reductions.jl:2-53) on the state
// it has just produced. This header is the host side: the launch model and the entry points (the descriptor checks, the
// common fill of sweep_args and the ladder from a descriptor to its flavour are sweep_device.hpp's: the scalar sweep shares them).
//
// Where the kernels live:
//  * sweep_device.hpp: sweep_args, boundary and dt-state helpers, buffer addressing, dt/CFL tracking, k_fold_pairs / k_fold_dt;
//    host side: check_sweep_desc, base_sweep_args, with_flavour.
//  * sweep_y_kernel.hpp: Y sweep (k_sweep_y): lane ↔ column (fp32 tuned: two adjacent columns), the register pipeline of
//    sweep_pipeline.hpp marches along y; optional store exchange through LDS (sweep_args::y_sx).
//  * sweep_x_kernel.hpp: X sweep, spatial form (k_sweep_x_dpp): lane ↔ cell(s) of a row, neighbours fetched with
//    DPP wavefront shifts (sweep_spatial.hpp, lane_shift.hpp); no LDS, no barrier, coalesced 16-B accesses.
//  * sweep_stages.hpp: the tuned arithmetic of the seven stages of a sweep, one function per stage (fast::), with the tuned
//    primitives rcp, rcp1, sqrt_, float2v. PipeFast and SpatialSweep::run_fast only fetch operands, call these and store.
//  * fused_sweep_alt_kernels.hpp / fused_sweep_alt_cycle.hpp (-DARMON_ALT_KERNELS): k_sweep_x_lds, k_cycle_xy / k_cycle_pc.
//  * placement.hip: armon_hip_tune_placement / armon_hip_choose_placement (they call armon_hip_sweep / armon_hip_sweep_pair).
// Redundant work is confined to the LAG (≤4) cells at both ends of a run / strip. Block and strip origins are
// aligned to the 64-B sectors of the ghosted rows, stores are non-temporal (profiles/NOTES.md has the A/B numbers).
// Tuning knobs (tools/ab_sweep.py, parity tests), read from the environment once per context or set with
// armon_hip_set_tuning: ARMON_SWEEP_ALIGN, ARMON_XS_NITER, ARMON_Y_SEG, ARMON_Y_COLS1, ARMON_Y_SX, ARMON_Y_NT, ARMON_X_XCD, ARMON_X_ROWS, ARMON_PAIR_ONLY;
// compile-time: ARMON_NT_X, ARMON_NT_Y, ARMON_Y_PF, ARMON_Y_PRIO, ARMON_Y_WAVES, ARMON_Y_BLOCK, ARMON_XS_ROWS, ARMON_XS_WAVES,
// ARMON_X_PRIO, ARMON_X_PRELOAD, ARMON_PROBE_NOCOMPUTE, ARMON_ONLY_HEADLINE, ARMON_Y_NT_ALL.
#pragma once
#include "sweep_device.hpp"
#include "sweep_y_kernel.hpp"
#include "sweep_x_kernel.hpp"

namespace {

// =====================================================================================================================
// Measured-and-rejected alternatives: the whole-cycle kernels k_cycle_xy / k_cycle_pc, the
// LDS-transposed X march k_sweep_x_lds (and, in launch(), the one-cell-per-lane form of the DPP sweep). They are correct and
// tested but 1.3-4x slower than what the solver runs, so they are only compiled with -DARMON_ALT_KERNELS, into
// libarmon_hip_alt.so (build.py), which the tests and tools that exercise them load; the product library carries none.
#ifdef ARMON_ALT_KERNELS
#include "fused_sweep_alt_kernels.hpp"
#endif  // ARMON_ALT_KERNELS

// ---- launch ----------------------------------------------------------------------------------------------
// Shape of a Y launch, decided once per sweep (armon_hip_sweep sizes the runs with it, launch() picks the kernel and the grid).
struct y_shape {
    int cols = 1;                    // columns per lane
    int block = kYBlock;             // lanes per workgroup
    bool sx = false;                 // rows stored through LDS (sweep_args::y_sx)
    bool nt = false;                 // rows loaded non-temporally (y_nt_loads; the flavours without that form ignore it)
};
// `in_len`, `out_len`: pitch of the rows the march reads / writes
y_shape y_launch_shape(const armon_ctx* ctx, const ARMON_SWEEP_DESC* d, int64_t in_len, int64_t out_len)
{
    y_shape s;
    // fp32, tuned arithmetic: two columns per lane when every row is 8-B aligned (even pitch and ghost width): half the
    // workgroups per row. (Not instantiated for the exact flavour: build time; the tests require it to equal the one-column kernel.)
    if (std::is_same<real, float>::value && !d->exact && d->nx % 2 == 0 && d->nghost % 2 == 0 && d->nx >= 2 && !ctx->tune_y_cols1)
        s.cols = 2;
    // the Y march stores through LDS when its rows do not all start on sectors (ARMON_Y_SX: 1 always, 2 never). Tuned
    // arithmetic only: the exact flavour is bound by its arithmetic (§4.2) and is not instantiated with the exchange.
    if (ctx->tune_align != 0 && ctx->tune_y_sx != 2 && !d->exact) {
        const uintptr_t outs = (uintptr_t)d->rho_out | (uintptr_t)d->u_out | (uintptr_t)d->v_out | (uintptr_t)d->E_out;
        s.sx = outs % 64 == 0 && ((out_len * (int64_t)sizeof(real)) % 64 != 0 || ctx->tune_y_sx == 1);
    }
    s.block = s.sx ? kYSxBlock : kYBlock;
    // Non-temporal row loads when every row the march reads starts on a 128-B line: a wave's 512-B segment (the block origin
    // is shifted onto a line, a.xshift) then shares no line with its neighbours. The intermediate of armon_hip_sweep_pair
    // is laid out for it; a block whose own pitch is whole lines qualifies as it stands. ARMON_Y_NT = 2: never (A/B).
    {
        const uintptr_t ins = (uintptr_t)d->rho_in | (uintptr_t)d->u_in | (uintptr_t)d->v_in | (uintptr_t)d->E_in;
        s.nt = ctx->tune_align != 0 && ctx->tune_y_nt != 2 && s.cols == 1 && !s.sx && ins % 128 == 0 &&
               (in_len * (int64_t)sizeof(real)) % 128 == 0;
    }
    return s;
}

template <class PIPE, bool TRACK>
int launch(armon_ctx* ctx, const sweep_args& a, int axis, const y_shape& ys, int64_t* n_blocks)
{
    const int64_t n_out = a.o_hi - a.o_lo;
    if (axis == ARMON_AXIS_Y) {
        const int64_t per_block = (int64_t)ys.block * ys.cols;
        dim3 grid((unsigned)((a.nx + a.xshift + per_block - 1) / per_block), (unsigned)((n_out + a.seg - 1) / a.seg));
        *n_blocks = (int64_t)grid.x * grid.y;
        if constexpr (std::is_same<real, float>::value && !PIPE::kExact) {
            if (ys.cols == 2) {
                if (ys.sx)
                    hipLaunchKernelGGL((k_sweep_y<PIPE, TRACK, kYSxBlock, true, 2>), grid, dim3(ys.block), 0, ctx->stream, a);
                else
                    hipLaunchKernelGGL((k_sweep_y<PIPE, TRACK, kYBlock, false, 2>), grid, dim3(ys.block), 0, ctx->stream, a);
                return check_launch("sweep_y2");
            }
        }
        if constexpr (!PIPE::kExact) {                       // (the store exchange is never chosen for the exact flavour: library size)
            if (ys.sx) {
                hipLaunchKernelGGL((k_sweep_y<PIPE, TRACK, kYSxBlock, true>), grid, dim3(ys.block), 0, ctx->stream, a);
                return check_launch("sweep_y (store exchange)");
            }
        }
        if constexpr (y_nt_loads(PIPE::EOS, PIPE::kExact)) {
            if (ys.nt) {
                hipLaunchKernelGGL((k_sweep_y<PIPE, TRACK, kYBlock, false, 1, true>), grid, dim3(ys.block), 0, ctx->stream, a);
                return check_launch("sweep_y (nt loads)");
            }
        }
        hipLaunchKernelGGL((k_sweep_y<PIPE, TRACK>), grid, dim3(ys.block), 0, ctx->stream, a);
        return check_launch("sweep_y");
    }
#if defined(ARMON_ALT_KERNELS) && !defined(ARMON_ONLY_HEADLINE)
    if (a.x_kernel == 2) {
        dim3 grid((unsigned)((n_out + a.seg - 1) / a.seg), (unsigned)((a.ny + kXRows - 1) / kXRows));
        *n_blocks = (int64_t)grid.x * grid.y;
        const size_t lds = (size_t)(a.emit ? 6 : 4) * kXRows * (kXChunk + 1) * sizeof(real);
        hipLaunchKernelGGL((k_sweep_x_lds<PIPE, kXChunk, TRACK>), grid, dim3(kXRows), lds, ctx->stream, a);
        return check_launch("sweep_x_lds");
    }
#endif
    // one strip per wave; the A/B build also carries the multi-strip form with its prefetch buffer (ARMON_XS_NITER > 1)
    int niter = 1;
#if defined(ARMON_ALT_KERNELS) && !defined(ARMON_ONLY_HEADLINE)
    if (ctx->tune_xs_niter > 1) niter = ctx->tune_xs_niter;
#elif defined(ARMON_XS_MULTI)      // tools/build_variant.sh: the round-2 form alone, for A/B timing
    niter = ctx->tune_xs_niter > 0 ? ctx->tune_xs_niter : 2;
#endif
    const bool k1 = a.x_kernel == 3;
    // the boundary strips of a tile (partial sweeps of at most 8 cells): four rows of 16 lanes per wave
    if (a.x_kernel == 0 && a.o_hi - a.o_lo <= 8) {
        const int64_t per_block = 16 - 2 * PIPE::LAG;
        dim3 grid((unsigned)((a.o_hi - a.x_first + per_block - 1) / per_block), (unsigned)((a.ny + 4 * kXSRows - 1) / (4 * kXSRows)));
        *n_blocks = (int64_t)grid.x * grid.y * kXSRows;
        sweep_args b = a;
        b.gx = (int32_t)grid.x;
        b.gy = (int32_t)grid.y;
        hipLaunchKernelGGL((k_sweep_x_dpp<PIPE::SCHEME, PIPE::LIM, PIPE::PROJ, PIPE::EOS, PIPE::kExact, 1, TRACK, true, 1>),
                           grid, dim3(64, kXSRows), 0, ctx->stream, b, 1);
        return check_launch("sweep_x_dpp (narrow)");
    }
    const int halo = k1 ? PIPE::LAG : 4;
    const int64_t per_block = (int64_t)niter * (64 * (k1 ? 1 : 2) - 2 * halo);
    const int64_t x_lowest = a.x_row_align ? a.o_lo - (64 / (int64_t)sizeof(real) - 1) : a.x_first;   // strips are counted from the lowest origin of any row
    dim3 grid((unsigned)((a.o_hi - x_lowest + per_block - 1) / per_block), (unsigned)((a.ny + kXSRows - 1) / kXSRows));
    if (a.x_wg_along_x && !k1 && niter == 1)                  // kXSRows strips of one row per workgroup
        grid = dim3((unsigned)((a.o_hi - x_lowest + kXSRows * per_block - 1) / (kXSRows * per_block)), (unsigned)a.ny);
    *n_blocks = (int64_t)grid.x * grid.y * kXSRows;          // one pair of maxima per wave
    sweep_args b = a;
    b.gx = (int32_t)grid.x;
    b.gy = (int32_t)grid.y;
#if defined(ARMON_ALT_KERNELS) && !defined(ARMON_ONLY_HEADLINE)
    if (k1)
        hipLaunchKernelGGL((k_sweep_x_dpp<PIPE::SCHEME, PIPE::LIM, PIPE::PROJ, PIPE::EOS, PIPE::kExact, 1, TRACK, false>),
                           grid, dim3(64, kXSRows), 0, ctx->stream, b, niter);
    else if (niter > 1)
        hipLaunchKernelGGL((k_sweep_x_dpp<PIPE::SCHEME, PIPE::LIM, PIPE::PROJ, PIPE::EOS, PIPE::kExact, 2, TRACK, false>),
                           grid, dim3(64, kXSRows), 0, ctx->stream, b, niter);
    else
#endif
#ifdef ARMON_XS_MULTI
        hipLaunchKernelGGL((k_sweep_x_dpp<PIPE::SCHEME, PIPE::LIM, PIPE::PROJ, PIPE::EOS, PIPE::kExact, 2, TRACK, false>),
                           grid, dim3(64, kXSRows), 0, ctx->stream, b, niter);
#else
        hipLaunchKernelGGL((k_sweep_x_dpp<PIPE::SCHEME, PIPE::LIM, PIPE::PROJ, PIPE::EOS, PIPE::kExact, 2, TRACK, true>),
                           grid, dim3(64, kXSRows), 0, ctx->stream, b, niter);
#endif
    return check_launch("sweep_x_dpp");
}

// Rows per run of the Y march. A run re-reads 2·LAG halo rows (and recomputes them), so long runs are cheaper per
// cell, but the launch must still fill the device evenly: the chip holds n_cu·ARMON_Y_WAVES·4 waves of this kernel
// at once and a launch of 4.06 such rounds takes nearly 5. Choose the number of runs per column that minimises
// rounds × (rows + halo), the rounds counted half-way between the exact ratio and its ceiling (waves drift apart,
// so a partial last round costs less than a whole one), among the launches of at least two rounds (a single round
// of long-lived workgroups exposes the whole ramp-up and tail: 4096², 137 rows in one round is 5 % slower than 32
// rows in 4.25). Measured at 16384² (tools/y_ab_r02.sh, one process): 128 rows 3.17 ms, 256: 3.12, 421: 3.09,
// 529: 3.08, 713: 3.09, 1093: 3.12, 2341 (one round, 11 % of the slots empty): 3.19.
int y_run_length(int n_cu, int64_t nx, int64_t ny, int lag, int cols_per_lane, int block)
{
    const double slots = (double)n_cu * ARMON_Y_WAVES * 4 / (block / 64);           // workgroups resident at once
    const int64_t cols = (nx + 16 + (int64_t)block * cols_per_lane - 1) / ((int64_t)block * cols_per_lane);
    int best = (int)(ny < 32 ? ny : 32);
    double best_cost = 1e300;
    for (int64_t nruns = 1; nruns <= ny; nruns++) {
        const int64_t seg = (ny + nruns - 1) / nruns;
        if (seg < 32) break;
        if ((ny + seg - 1) / seg != nruns) continue;                              // same launch as a smaller nruns
        const double rounds = (double)(cols * nruns) / slots;
        // One round that (nearly) fills every slot is the other good launch: every workgroup is resident from the start,
        // the runs are as long as they can be. Small tiles need it — 4096 x 8192 (the tile of 16384² on 8 GPUs): 273 rows in
        // 0.996 rounds 0.388 ms, 137 rows in 1.99 rounds 0.394, 92 rows in 2.99 rounds (the choice until round 3) 0.401,
        // 512 rows in 0.53 rounds 0.590 (profiles/r03_ab_yseg_4096x8192.txt) — while at 16384² the only single round
        // leaves 11 % of the slots empty and stays excluded (3.19 ms against 3.08).
        const bool full_single_round = rounds <= 1. && rounds >= 0.93;
        if (rounds < 2. && !full_single_round) continue;
        const double cost = (full_single_round ? 1. : 0.5 * (rounds + std::ceil(rounds))) * (double)(seg + 2 * lag);
        if (cost < best_cost) {
            best_cost = cost;
            best = (int)seg;
        }
    }
    return best;
}

// Upper bound of the number of workgroups any form launches for this block (sizes the partials buffer).
int64_t max_blocks(const sweep_args& a)
{
    const int64_t by = (a.nx + 16 + kYBlock - 1) / kYBlock * ((a.ny + a.seg - 1) / a.seg);
#ifdef ARMON_ALT_KERNELS
    const int64_t bx_lds = (a.nx + a.seg - 1) / a.seg * ((a.ny + kXRows - 1) / kXRows);
#else
    const int64_t bx_lds = 0;
#endif
    // per wave; niter >= 1, K = 1, LAG = 4; + kXSRows: a row's strips are rounded up to whole workgroups (x_wg_along_x)
    const int64_t bx_dpp = ((a.nx + 8) / 56 + 1 + kXSRows) * ((a.ny + kXSRows - 1) / kXSRows) * kXSRows;
    int64_t m = by > bx_lds ? by : bx_lds;
    m = m > bx_dpp ? m : bx_dpp;
    return m + kFoldBlocks;                                   // + the first-level results of fold_dt_launch
}

template <class PIPE>
int dispatch_track(armon_ctx* ctx, const sweep_args& a, int axis, const y_shape& ys, bool track, int64_t* n_blocks)
{
    if (track) return launch<PIPE, true>(ctx, a, axis, ys, n_blocks);
    return launch<PIPE, false>(ctx, a, axis, ys, n_blocks);
}

}  // namespace

// One sweep of the block `d` describes, reading arrays of pitch `in_len` and writing arrays of pitch `out_len` (cell (x, y) at
// (y + g)·pitch + x + g in both). armon_hip_sweep: both are the block's own nx + 2g.
static int sweep_pitched(armon_ctx* ctx, const ARMON_SWEEP_DESC* d, int64_t in_len, int64_t out_len)
{
    ARMON_REQUIRE(ctx && d, "NULL argument");
    int lag;
    if (const int bad = check_sweep_desc(d, &lag); bad != ARMON_OK) return bad;
    const bool X = d->axis == ARMON_AXIS_X;
    const int64_t n_axis = X ? d->nx : d->ny;
    ARMON_REQUIRE(d->rho_in && d->u_in && d->v_in && d->E_in && d->rho_out && d->u_out && d->v_out && d->E_out,
                  "NULL state array");
    ARMON_REQUIRE(d->rho_in != d->rho_out && d->u_in != d->u_out && d->v_in != d->v_out && d->E_in != d->E_out,
                  "in and out arrays must not alias (ping-pong)");
#ifdef ARMON_ALT_KERNELS
    ARMON_REQUIRE(d->x_kernel == 0 || d->x_kernel == 2 || d->x_kernel == 3, "unknown x_kernel form %d", d->x_kernel);
#else
    ARMON_REQUIRE(d->x_kernel == 0, "x_kernel form %d is a measured alternative: only libarmon_hip_alt.so (-DARMON_ALT_KERNELS) carries it",
                  d->x_kernel);
#endif
    // only the kernels the solver runs read the device-resident time step (sweep_begin): the LDS X march of the A/B build
    // would take `dt` (then a factor) for the step itself, silently
    ARMON_REQUIRE(!d->dt_state || d->x_kernel == 0 || d->x_kernel == 3,
                  "dt_state is not honoured by x_kernel form %d (only the DPP X sweeps and the Y march read it)", d->x_kernel);
    const bool track = d->dt_cfl_out != nullptr;
    ARMON_REQUIRE(!track || (d->cfl_dx > 0 && d->cfl_dy > 0), "dt_cfl_out needs cfl_dx, cfl_dy > 0");

    sweep_args a = base_sweep_args(d, in_len, out_len);
    a.emit = (d->p_out ? 1 : 0) | (d->c_out ? 2 : 0);
    a.rho_out = d->rho_out;
    a.ua_out = X ? d->u_out : d->v_out;
    a.ut_out = X ? d->v_out : d->u_out;
    a.E_out = d->E_out;
    a.p_out = d->p_out;
    a.c_out = d->c_out;
    a.st = d->dt_state;
    const bool align = ctx->tune_align != 0;
    const y_shape ys = X ? y_shape{} : y_launch_shape(ctx, d, in_len, out_len);
    a.y_sx = ys.sx;
    if (X) {
        a.seg = 512;
    } else if (ctx->tune_y_seg > 0) {
        a.seg = ctx->tune_y_seg;
    } else {
        if (ctx->seg_nx != d->nx || ctx->seg_ny != n_axis || ctx->seg_lag != lag || ctx->seg_cols != ys.cols * ys.block) {
            ctx->seg_value = y_run_length(ctx->n_cu, d->nx, n_axis, lag, ys.cols, ys.block);
            ctx->seg_cols = ys.cols * ys.block;
            ctx->seg_nx = d->nx;
            ctx->seg_ny = n_axis;
            ctx->seg_lag = lag;
        }
        a.seg = ctx->seg_value;
    }
    // the Y march addresses a run of rows with 32-bit byte offsets from the run's first row
    ARMON_REQUIRE(X || (in_len > out_len ? in_len : out_len) * (int64_t)sizeof(real) * (a.seg + 2 * lag + 16) < (1ll << 32),
                  "block too wide for 32-bit row offsets (%lld cells per row, runs of %d rows)", (long long)d->nx, a.seg);
    a.x_kernel = d->x_kernel;
    a.o_lo = 0;
    a.o_hi = n_axis;
    if (d->out_hi != 0) {
        ARMON_REQUIRE(d->out_lo >= 0 && d->out_lo < d->out_hi && d->out_hi <= n_axis,
                      "invalid partial sweep [%lld, %lld) of %lld cells", (long long)d->out_lo, (long long)d->out_hi, (long long)n_axis);
        a.o_lo = d->out_lo;
        a.o_hi = d->out_hi;
    }
    a.xshift = (X || !align) ? 0 : d->nghost % 16;
    a.x_first = X ? (align ? a.o_lo - (a.o_lo + d->nghost) % 8 : a.o_lo) : 0;
    // XCD-aware placement of the X sweep's workgroups (sweep_x_dpp_body): neighbouring strips of a row — they share a 128-B
    // line, a strip's loads start 32 B before its sector-aligned stores — then follow each other on ONE XCD's L2 instead of
    // being fetched from the fabric by two. With one strip per wave that is the whole over-fetch of the sweep: 18.90 ->
    // 17.3 GB per launch by counters at 16384² (1.10x -> 1.01x the algorithmic bytes), time equal to 1.5 % better
    // (profiles/r04_ab_x_xcd.txt). fp64 only: fp32 shares its lines inside a workgroup instead (x_wg_along_x below).
    // The order assumes what the part does in its default mode: 8 XCDs of 32 CUs, workgroups dealt round-robin. A device
    // that shows another CU count (a partitioned MI355X: CPX / DPX modes) has fewer XCDs per agent, the map would only
    // scramble rows there: it is switched off. The workgroup shape is decided first (a block with more than 65535 rows cannot
    // take the along-x shape and falls back to one strip of 4 rows, which the remap then serves); the explicit knob wins.
    const bool want_along_x = ctx->tune_x_rows == 2 || (ctx->tune_x_rows == 0 && sizeof(real) == 4);
    const bool along_x = X && want_along_x && d->ny <= 65535 && ctx->tune_x_xcd <= 0;
    const bool eight_xcds = ctx->n_cu == 256;
    a.xcd_remap = (ctx->tune_x_xcd < 0 ? sizeof(real) == 8 : ctx->tune_x_xcd != 0) && !along_x && eight_xcds;
    // origins row by row when one origin cannot align every row (the one-strip-per-wave form only; the A/B forms keep one)
    a.x_row_align = 0;
#ifndef ARMON_XS_MULTI
    {
        const uintptr_t bases = (uintptr_t)d->rho_in | (uintptr_t)d->u_in | (uintptr_t)d->v_in | (uintptr_t)d->E_in |
                                (uintptr_t)d->rho_out | (uintptr_t)d->u_out | (uintptr_t)d->v_out | (uintptr_t)d->E_out |
                                (uintptr_t)d->p_out | (uintptr_t)d->c_out;
        a.x_row_align = X && align && d->x_kernel == 0 && ctx->tune_xs_niter <= 1 && a.out_len % (64 / (int64_t)sizeof(real)) != 0 &&
                        bases % 64 == 0;
    }
#endif
    // workgroup shape of the X sweep (profiles/r03_ab_x_workgroup_shape.txt): 4 consecutive strips of one row pay for fp32
    // (1.54 -> 1.43 ms at 16384²: a 512-B strip shares a quarter of its 128-B lines with its neighbours) and not for fp64
    // (equal at 16384² and 4096 x 8192, +3 % at 8192²), which keeps one strip of 4 rows. ARMON_X_ROWS: 1 / 2 force a shape.
    a.x_wg_along_x = along_x ? 1 : 0;                                                            // grid.y carries the rows
    a.partials = nullptr;
    if (track) {
        int rc = ensure_partials(ctx, (size_t)(2 * max_blocks(a)));
        if (rc != ARMON_OK) return rc;
        a.partials = reinterpret_cast<real*>(ctx->partials);
    }

    int64_t n_blocks = 0;
    int rc;
    auto go = [&](auto fl) { return dispatch_track<typename decltype(fl)::PIPE>(ctx, a, d->axis, ys, track, &n_blocks); };
#ifdef ARMON_ONLY_HEADLINE   // variant builds for A/B timing (tools/build_variant.sh): one instantiation, seconds to compile
#ifndef ARMON_ONLY_EOS
#define ARMON_ONLY_EOS ARMON_EOS_PERFECT_GAS       // -DARMON_ONLY_EOS=ARMON_EOS_BIZARRIUM: the one instantiation is config 5's
#endif
    ARMON_REQUIRE(d->scheme == ARMON_SCHEME_GAD && d->limiter == ARMON_LIMITER_MINMOD && d->projection == ARMON_PROJECTION_EULER_2ND &&
                  d->eos == ARMON_ONLY_EOS && d->x_kernel == 0, "headline-only variant build");
    rc = d->exact ? go(flavour<ARMON_SCHEME_GAD, ARMON_LIMITER_MINMOD, ARMON_PROJECTION_EULER_2ND, ARMON_ONLY_EOS, true>{})
               : go(flavour<ARMON_SCHEME_GAD, ARMON_LIMITER_MINMOD, ARMON_PROJECTION_EULER_2ND, ARMON_ONLY_EOS, false>{});
#else
    rc = with_flavour(d, go);
#endif
    if (rc != ARMON_OK || !track) return rc;
    return fold_dt_launch(ctx, a.partials, n_blocks, (real)d->cfl_dx, (real)d->cfl_dy, d->dt_cfl_out, d->dt_accumulate, d->dt_state);
}

extern "C" int ARMON_SWEEP_FN(armon_ctx* ctx, const ARMON_SWEEP_DESC* d)
{
    ARMON_REQUIRE(ctx && d, "NULL argument");
    const int64_t pitch = d->nx + 2 * (int64_t)d->nghost;
    return sweep_pitched(ctx, d, pitch, pitch);
}

// ---- the X and the Y sweep of one Sequential cycle, the state between them in rows of whole 128-B lines ----------------
// Nobody outside looks at the X sweep's output before the Y sweep has consumed it, so its layout is the library's: the
// ghost offsets are kept — cell (x, y) at (y + g)·P + x + g — and the pitch P is nx + 2g rounded up to a whole line. Every
// row the Y march reads then starts on a line, which is what its non-temporal loads need (y_launch_shape); the 32-B phase
// between the X sweep's loads and its sector-aligned stores, and the strip origins, are what they are with one pitch.
#ifdef ARMON_PAIR_FN
extern "C" int64_t ARMON_PAIR_PITCH_FN(int64_t nx, int nghost)
{
    const int64_t line = 128 / (int64_t)sizeof(real);
    return (nx + 2 * (int64_t)nghost + line - 1) / line * line;
}

extern "C" int ARMON_PAIR_FN(armon_ctx* ctx, const ARMON_SWEEP_DESC* x, const ARMON_SWEEP_DESC* y, size_t mid_bytes)
{
    ARMON_REQUIRE(ctx && x && y, "NULL argument");
    ARMON_REQUIRE(x->axis == ARMON_AXIS_X && y->axis == ARMON_AXIS_Y, "the pair is an X sweep followed by a Y sweep");
    ARMON_REQUIRE(x->nx == y->nx && x->ny == y->ny && x->nghost == y->nghost && x->nx > 0 && x->ny > 0 && x->nghost >= 0,
                  "the two descriptors describe different blocks");
    ARMON_REQUIRE(x->rho_out == y->rho_in && x->u_out == y->u_in && x->v_out == y->v_in && x->E_out == y->E_in && x->rho_out,
                  "the Y sweep must read the arrays the X sweep writes");
    // the Y march then reads real cells only (mirror rows come from inside the block): no ghost of the intermediate is ever read
    ARMON_REQUIRE(y->bc_low && y->bc_high, "a block with a remote Y side cannot use the pair (its ghost rows come from a neighbour)");
    ARMON_REQUIRE(x->out_hi == 0 && y->out_hi == 0, "the pair runs whole sweeps");
    ARMON_REQUIRE(!x->p_out && !x->c_out && !x->dt_cfl_out, "the X sweep of the pair has no output of its own");
    ARMON_REQUIRE(x->x_kernel == 0, "x_kernel form %d cannot write the intermediate layout", x->x_kernel);
    const int64_t pitch = x->nx + 2 * (int64_t)x->nghost, mid = ARMON_PAIR_PITCH_FN(x->nx, x->nghost);
    ARMON_REQUIRE((uint64_t)mid_bytes >= (uint64_t)(mid * (x->ny + 2 * (int64_t)x->nghost)) * sizeof(real),
                  "the intermediate arrays hold %zu bytes, rows of %lld cells need %lld", mid_bytes, (long long)mid,
                  (long long)(mid * (x->ny + 2 * (int64_t)x->nghost) * (int64_t)sizeof(real)));
    // ARMON_PAIR_ONLY (A/B tools): 1 = the X sweep alone, 2 = the Y sweep alone (on the intermediate an earlier call left)
    if (ctx->tune_pair_only != 2) {
        const int rc = sweep_pitched(ctx, x, pitch, mid);
        if (rc != ARMON_OK) return rc;
    }
    if (ctx->tune_pair_only != 1) return sweep_pitched(ctx, y, mid, pitch);
    return ARMON_OK;
}
#endif

// ---- whole cycle (X sweep then Y sweep, Sequential splitting) in one launch: k_cycle_xy --------------------------------
#if defined(ARMON_CYCLE_FN) && !defined(ARMON_ALT_KERNELS)
extern "C" int ARMON_CYCLE_FN(armon_ctx* ctx, const ARMON_SWEEP_DESC* x, const ARMON_SWEEP_DESC* y)
{
    ARMON_REQUIRE(ctx && x && y, "NULL argument");
    ARMON_REQUIRE(false, "the whole-cycle kernel is a measured alternative (slower than the two sweeps, DESIGN.md section 4.2): "
                         "only libarmon_hip_alt.so (-DARMON_ALT_KERNELS) carries it");
    return ARMON_ERR_INVALID_ARG;
}
#endif
#if defined(ARMON_CYCLE_FN) && defined(ARMON_ALT_KERNELS)
#include "fused_sweep_alt_cycle.hpp"
#endif
