// sweep_y_kernel.hpp — the Y march of the fused sweep (k_sweep_y) and its tuning macros. Not a stand-alone header
// (see fused_sweep.hpp).
#pragma once
#include "sweep_device.hpp"

namespace {

// ---- Y sweep ---------------------------------------------------------------------------------------
#ifndef ARMON_Y_BLOCK
#define ARMON_Y_BLOCK 256        // columns (= lanes) per workgroup of the Y march (tuning macro)
#endif
constexpr int kYBlock = ARMON_Y_BLOCK;
constexpr int kYSxBlock = 512;     // lanes per workgroup of the Y march with the LDS store exchange (sweep_args::y_sx)
#ifndef ARMON_Y_PF
#define ARMON_Y_PF 4             // rows prefetched ahead of the march (≤ 5: the cell ring has 8 slots)
#endif
#ifndef ARMON_Y_PRIO
#define ARMON_Y_PRIO 0           // > 0: issue priority of a step's loads (s_setprio around them)
#endif
#ifndef ARMON_Y_WAVES
#define ARMON_Y_WAVES 2          // minimum waves per SIMD the Y march is compiled for (register budget)
#endif

// What a lane of the march holds: one column, or — the fp32 form — two adjacent ones. With 4-B elements one column per
// lane moves only 256 B per wave and instruction; two adjacent columns per lane (8-B accesses, two independent pipelines =
// twice the ILP at the register cost of one fp64 pipeline) restore the 512-B row segments of the fp64 kernel.
template <int COLS, class PIPE> struct y_lane;
template <class PIPE> struct y_lane<1, PIPE> {
    using V = real;
    using pipe_t = PIPE;
    using lds_t = real;              // element of the store exchange
    template <bool NT = false>
    static __device__ __forceinline__ V load(rsrc_t r, unsigned voff, unsigned soff)
    {
        if constexpr (NT && std::is_same<real, double>::value) return buf_load_nt(r, voff, soff);
        else return buf_load<real>(r, voff, soff);
    }
    static __device__ __forceinline__ void store(rsrc_t r, unsigned voff, unsigned soff, V v) { buf_store(r, voff, soff, v); }
    static __device__ __forceinline__ void track(cfl_track& t, const V& u, const V& v, const V& c) { t.add(u, v, c); }
};
template <class PIPE> struct y_lane<2, PIPE> {
    // the two columns of a lane are ONE pipeline on 2-vectors: packed v_pk_* arithmetic (sweep_stages.hpp, float2v)
    using V = fused::fast::float2v;
    using pipe_t = fused::PipeFast<PIPE::SCHEME, PIPE::LIM, PIPE::PROJ, PIPE::EOS, V>;
    using lds_t = float2;
    // (row loads: written out in the kernel's load step, buf_load2 and a float2 -> V lambda as before the forms were merged)
    static __device__ __forceinline__ void store(rsrc_t r, unsigned voff, unsigned soff, V v) { buf_store2(r, voff, soff, v.x, v.y); }
    static __device__ __forceinline__ void store(rsrc_t r, unsigned voff, unsigned soff, float2 q) { buf_store2(r, voff, soff, q.x, q.y); }
    static __device__ __forceinline__ void track(cfl_track& t, const V& u, const V& v, const V& c)
    {
        t.add(u.x, v.x, c.x);
        t.add(u.y, v.y, c.y);
    }
};

// Which instantiations of the march exist with non-temporal row loads (NTL; ARMON_NT_Y above is the policy of all the
// others). The host chooses the form per launch, when every row the march READS is a whole number of 128-B lines from the
// next (launch() in fused_sweep.hpp): a wave's 512-B segment then shares no line with its neighbours, and a line that is
// not kept is not fetched twice (profiles/r05_ab_nt.txt §5, profiles/y_line_pitch_ab.txt). The tuned fp64 perfect-gas
// march only: the flavour it was measured to pay for, as for the X sweep (x_nt_loads).
constexpr bool y_nt_loads(int eos, bool exact)
{
#ifdef ARMON_Y_NT_ALL            // A/B builds (tools/build_variant.sh): every fp64 flavour
    return sizeof(real) == 8;
#endif
    return sizeof(real) == 8 && eos == ARMON_EOS_PERFECT_GAS && !exact;
}

template <class PIPE, bool TRACK, int BLOCK = kYBlock, bool SX = false, int COLS = 1, bool NTL = false>
__global__ void __launch_bounds__(BLOCK, ARMON_Y_WAVES)
k_sweep_y(sweep_args a)
{
    if (!sweep_begin(a)) return;
    using lane_t = y_lane<COLS, PIPE>;
    using V = typename lane_t::V;
    constexpr int LAG = PIPE::LAG;
    constexpr int PF = ARMON_Y_PF;   // rows in flight per lane, ahead of the march
    const int nx = (int)a.nx, ny = (int)a.ny, g = a.g;
    // The block origin is shifted left by a.xshift columns so that a wave's 512-B row segment starts on a
    // 64-B sector / 128-B line of the ghosted row instead of g cells into one (probe_access: -9 % time).
    // COLS = 2: two adjacent columns per lane (nx, g and a.xshift are even here): xr, xr + 1; 8-B accesses.
    const int xr = (int)(blockIdx.x * BLOCK + threadIdx.x) * COLS - a.xshift;
    const bool active = xr >= 0 && xr < nx;
    const int x = active ? xr : (xr < 0 ? 0 : nx - COLS);   // idle lanes shadow an edge column (pair) and never store
    const int o_hi = (int)a.o_hi;
    const int o0 = (int)a.o_lo + (int)blockIdx.y * a.seg;
    const int o1 = (o0 + a.seg < o_hi) ? o0 + a.seg : o_hi;
    const int jb = o0 - LAG, je = o1 + LAG;

    // Descriptors are based at the first row this run touches, so every scalar row offset is a small
    // non-negative 32-bit number whatever the size of the arrays (mirrored rows lie inside the run).
    const unsigned colb = (unsigned)(x + g) * (unsigned)sizeof(real);
    // pitch of the rows it reads and of the rows it writes: the same number for a plain sweep; the pair's Y march reads an
    // intermediate of whole lines per row (armon_hip_sweep_pair)
    const unsigned pitchb = (unsigned)a.row_len * (unsigned)sizeof(real), opitchb = (unsigned)a.out_len * (unsigned)sizeof(real);
    const int64_t in_base = (int64_t)(jb + g) * a.row_len, out_base = (int64_t)(o0 + g) * a.out_len;
    const rsrc_t r_rho = make_rsrc(a.rho_in + in_base), r_ua = make_rsrc(a.ua_in + in_base);
    const rsrc_t r_ut = make_rsrc(a.ut_in + in_base), r_E = make_rsrc(a.E_in + in_base);
    const rsrc_t w_rho = make_rsrc(a.rho_out + out_base), w_ua = make_rsrc(a.ua_out + out_base);
    const rsrc_t w_ut = make_rsrc(a.ut_out + out_base), w_E = make_rsrc(a.E_out + out_base);

    typename lane_t::pipe_t pipe(a.dt, a.dx, a.gamma, a.inv_dx, a.dt_dx);
    cfl_track cfl;

    int lj = jb;                     // next row to load and its offset from the run's first row
    unsigned lo_off = 0;
    unsigned so_off = (unsigned)(jb - LAG - o0) * opitchb;    // row j - LAG relative to row o0 (wraps until valid)

    // Store exchange (SX, chosen by sweep_args::y_sx; rows that do not all start on 64-B sectors, i.e. a pitch that is not a multiple of a sector).
    // A lane's column is fixed for the whole march, so on such rows every wave's 512-B store would begin and end inside a
    // sector, and it is the partial-sector STORES that cost (tools/probes/probe_ypitch.hip: misplaced loads +0.6 %, stores
    // +11 % at half a sector, +21 % on odd pitches). The workgroup's row is therefore passed through LDS: thread t stores
    // column (t - r) mod BLOCK of the workgroup, r = the row's phase in cells, so that all but the workgroup's two end
    // pieces are whole sectors; one barrier per row, two LDS buffers. The kernel is instantiated for it with workgroups of
    // kYSxBlock = 512 lanes (half as many end pieces: fp32 bench shape 1.55 -> 1.50 ms; without the exchange 256 lanes are
    // faster, profiles/r03_row_pitch_repairs.txt) and without any of this code for the usual, sector-aligned pitches.
    // COLS = 2: in units of a lane's column PAIR (8 B; eight pairs per sector).
    __shared__ typename lane_t::lds_t sx_lds[SX ? 2 : 1][SX ? 4 : 1][SX ? BLOCK : 1];
    static_assert((BLOCK & (BLOCK - 1)) == 0, "the store exchange wraps columns with a mask");
    static_assert(!NTL || (COLS == 1 && !SX), "non-temporal row loads: the one-column march without the store exchange");
    constexpr int kSec = 64 / (COLS * (int)sizeof(real));    // lane units (cells, pairs) per sector
    const int c0 = (int)(blockIdx.x * BLOCK) * COLS - a.xshift;   // first column of the workgroup (COLS = 2: even)
    int sx_r = (int)((((int64_t)(jb - LAG + g) * a.out_len + g + c0) >> (COLS - 1)) & (kSec - 1));    // phase of row j - LAG, j = jb
    const int sx_dr = (int)((a.out_len >> (COLS - 1)) & (kSec - 1));
    int sx_buf = 0;

    // The state of row lj is loaded straight into the pipeline's cell ring, slot lj mod 8, PF steps before
    // the march reaches it. CHECKED steps handle everything (mirrored / clamped loads, masked stores,
    // p/c output); the steady state of a run uses the unchecked form: plain loads, unconditional stores.
    auto load = [&](auto slot, auto checked) {
        constexpr int K = decltype(slot)::value & 7;
        constexpr bool CHECKED = decltype(checked)::value;
        auto& dst = pipe.c[K];
        if constexpr (COLS == 2) {                     // (its own load path, lambdas and all, as before the forms were merged:
                                                     //  hipcc's instruction order follows the shape of the source, and the ISA is pinned)
            auto vec = [](float2 q) { return V{q.x, q.y}; };
            auto put = [&](unsigned off, real fa, real ft) {
                dst.rho = vec(buf_load2(r_rho, colb, off));
                dst.ua = vec(buf_load2(r_ua, colb, off)) * fa;
                dst.ut = vec(buf_load2(r_ut, colb, off)) * ft;
                dst.E = vec(buf_load2(r_E, colb, off));
            };
            if (CHECKED) {
                const bool m_lo = lj < 0 && a.bc_low, m_hi = lj >= ny && a.bc_high;     // uniform, rare
                // physical boundary: mirror of the inside (ref src/halo_exchange.jl:2-29)
                const int src = m_lo ? -1 - lj : (m_hi ? 2 * ny - 1 - lj : lj);
                const unsigned off = (unsigned)(src - jb) * pitchb;
                const real fa = m_lo ? a.fa_low : (m_hi ? a.fa_high : real(1));
                const real ft = m_lo ? a.ft_low : (m_hi ? a.ft_high : real(1));
                put(off, fa, ft);
                if (lj + 1 < je) {       // stay on the last row once the run is exhausted (padding steps)
                    lj++;
                    lo_off += pitchb;
                }
            } else {
                dst.rho = vec(buf_load2(r_rho, colb, lo_off));
                dst.ua = vec(buf_load2(r_ua, colb, lo_off));
                dst.ut = vec(buf_load2(r_ut, colb, lo_off));
                dst.E = vec(buf_load2(r_E, colb, lo_off));
                lj++;
                lo_off += pitchb;
            }
        } else {
            if (CHECKED) {
                const bool m_lo = lj < 0 && a.bc_low, m_hi = lj >= ny && a.bc_high;     // uniform, rare
                // physical boundary: mirror of the inside (ref src/halo_exchange.jl:2-29)
                const int src = m_lo ? -1 - lj : (m_hi ? 2 * ny - 1 - lj : lj);
                const unsigned off = (unsigned)(src - jb) * pitchb;
                const real fa = m_lo ? a.fa_low : (m_hi ? a.fa_high : real(1));
                const real ft = m_lo ? a.ft_low : (m_hi ? a.ft_high : real(1));
                dst.rho = lane_t::template load<NTL>(r_rho, colb, off);
                dst.ua = lane_t::template load<NTL>(r_ua, colb, off) * fa;
                dst.ut = lane_t::template load<NTL>(r_ut, colb, off) * ft;
                dst.E = lane_t::template load<NTL>(r_E, colb, off);
                if (lj + 1 < je) {       // stay on the last row once the run is exhausted (padding steps)
                    lj++;
                    lo_off += pitchb;
                }
            } else {
                dst.rho = lane_t::template load<NTL>(r_rho, colb, lo_off);
                dst.ua = lane_t::template load<NTL>(r_ua, colb, lo_off);
                dst.ut = lane_t::template load<NTL>(r_ut, colb, lo_off);
                dst.E = lane_t::template load<NTL>(r_E, colb, lo_off);
                lj++;
                lo_off += pitchb;
            }
        }
    };
    using std::integral_constant;
    auto step = [&](auto ph, auto checked, int j) {
        constexpr int PH8 = decltype(ph)::value;
        constexpr bool CHECKED = decltype(checked)::value;
#if ARMON_Y_PRIO
        __builtin_amdgcn_s_setprio(ARMON_Y_PRIO);            // the row's loads go out ahead of the other wave's arithmetic
#endif
        load(integral_constant<int, PH8 + PF>{}, checked);   // row j + PF → slot (j + PF) mod 8
#if ARMON_Y_PRIO
        __builtin_amdgcn_s_setprio(0);
#endif
        V p, c, c_lag;
#ifdef ARMON_PROBE_NOCOMPUTE   // calibration build: same loads/stores, no arithmetic (tools/build_variant.sh)
        p = c = c_lag = V(real(0));
        const auto& cc = pipe.c[PH8 & 7];
        const fused::Out4<V> out{cc.rho, cc.ua, cc.ut, cc.E};
#else
        const fused::Out4<V> out = pipe.template advance<true, PH8>(p, c, c_lag);
#endif
        const int o = j - LAG;
        if (CHECKED) {
            if (a.emit && j >= o0 && j < o1 && active) {
                const unsigned off = so_off + LAG * opitchb;
                if (a.emit & 1) lane_t::store(make_rsrc(a.p_out + out_base), colb, off, p);
                if (a.emit & 2) lane_t::store(make_rsrc(a.c_out + out_base), colb, off, c);
            }
        }
        if (!CHECKED || (o >= o0 && o < o1)) {
            if constexpr (SX) {
                auto& L = sx_lds[sx_buf];
                if constexpr (COLS == 2) {                   // (written out: behind a helper of lane_t hipcc schedules the tracked form differently)
                    L[0][threadIdx.x] = float2{out.rho.x, out.rho.y};
                    L[1][threadIdx.x] = float2{out.ua.x, out.ua.y};
                    L[2][threadIdx.x] = float2{out.ut.x, out.ut.y};
                    L[3][threadIdx.x] = float2{out.E.x, out.E.y};
                } else {
                    L[0][threadIdx.x] = out.rho;
                    L[1][threadIdx.x] = out.ua;
                    L[2][threadIdx.x] = out.ut;
                    L[3][threadIdx.x] = out.E;
                }
                __syncthreads();
                const int ci = ((int)threadIdx.x - sx_r) & (BLOCK - 1);
                const int cx = c0 + COLS * ci;
                if (cx >= 0 && cx < nx) {
                    const unsigned cb = (unsigned)(cx + g) * (unsigned)sizeof(real);
                    if constexpr (COLS == 2) {               // (the order of LDS reads and stores of either form is the one it was tuned with)
                        const float2 q0 = L[0][ci], q1 = L[1][ci], q2 = L[2][ci], q3 = L[3][ci];
                        lane_t::store(w_rho, cb, so_off, q0);
                        lane_t::store(w_ua, cb, so_off, q1);
                        lane_t::store(w_ut, cb, so_off, q2);
                        lane_t::store(w_E, cb, so_off, q3);
                    } else {
                        lane_t::store(w_rho, cb, so_off, L[0][ci]);
                        lane_t::store(w_ua, cb, so_off, L[1][ci]);
                        lane_t::store(w_ut, cb, so_off, L[2][ci]);
                        lane_t::store(w_E, cb, so_off, L[3][ci]);
                    }
                }
                sx_buf ^= 1;
            } else if (active) {
                lane_t::store(w_rho, colb, so_off, out.rho);
                lane_t::store(w_ua, colb, so_off, out.ua);
                lane_t::store(w_ut, colb, so_off, out.ut);
                lane_t::store(w_E, colb, so_off, out.E);
            }
            if (TRACK) lane_t::track(cfl, out.ut, out.ua, c_lag);      // Y sweep: ut = u, ua = v
        }
        so_off += opitchb;
        sx_r = (sx_r + sx_dr) & (kSec - 1);
    };
    auto run = [&](auto checked, int t0, int t1) {           // steps [t0, t1), both multiples of 8
        for (int t = t0; t < t1; t += 8)
            static_for(std::make_integer_sequence<int, 8>{}, [&](auto ph) { step(ph, checked, jb + t + decltype(ph)::value); });
    };

    const int T = je - jb;                                   // steps of the run
    const int T8 = (T + 7) & ~7;                             // … padded to the unroll
    const int P = (2 * LAG + 7) & ~7;                        // after P steps every step emits a valid cell
    // last step (exclusive) whose prefetch needs neither mirroring nor clamping and whose store is valid
    const int plain_end = (a.bc_high && ny < je ? ny : je) - jb - PF;
    int M = (T < plain_end ? T : plain_end) & ~7;
    if (M < P || (a.emit & 3)) M = P;                        // p/c output: everything through the checked form

    // The block origin shift leaves the last workgroup of a row mostly past the last column: a wave with no
    // column at all skips the march (it still joins the block reduction below with neutral values).
    // (not with the store exchange: every wave of the workgroup takes part in its barriers; not with two columns per lane)
    const bool wave_idle = COLS == 1 && !SX && (int)(blockIdx.x * BLOCK + (threadIdx.x & ~63u)) - a.xshift >= nx;   // wave-uniform
    if (!wave_idle) {
        static_for(std::make_integer_sequence<int, PF>{}, [&](auto k) { load(k, std::true_type{}); });
        run(std::true_type{}, 0, P < T8 ? P : T8);
        run(std::false_type{}, P, M);
        run(std::true_type{}, M, T8);
    }

    if (TRACK) cfl_block_store<BLOCK / 64>(cfl, a.partials, (int64_t)blockIdx.y * gridDim.x + blockIdx.x, threadIdx.x);
}

}  // namespace
