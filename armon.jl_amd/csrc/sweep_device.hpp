// sweep_device.hpp — what the fused sweep's kernels share: sweep_args, the boundary / dt-state helpers, buffer addressing
// and its cache policy, the dt/CFL tracking and its fold kernels; and what the host sides of armon_hip_sweep and
// armon_hip_sweep_scalars share: the descriptor checks (check_sweep_desc), the common fill of sweep_args (base_sweep_args)
// and the ladder from a descriptor to its flavour (with_flavour). Not a stand-alone header (see fused_sweep.hpp).
#pragma once
#include "common.hpp"
#include "dt_state.hpp"
#include "reduce.hpp"
#include "sweep_pipeline.hpp"
#include "sweep_spatial.hpp"

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <type_traits>
#include <utility>

using namespace armon;

// The fused sweep's headers are compiled twice: fused_sweep_f64.hip (real = double, armon_hip_sweep) and fused_sweep_f32.hip
// (real = float, armon_hip_sweep_f32); everything else lives in the translation unit's anonymous namespace.
#ifndef ARMON_SWEEP_REAL
#error "include through fused_sweep_f64.hip / fused_sweep_f32.hip"
#endif

namespace {

using real = ARMON_SWEEP_REAL;
using vec2 = std::conditional<std::is_same<real, double>::value, double2, float2>::type;

// Streaming hints (tuning macros, see tools/build_variant.sh): the state is read once and written once per sweep and is far
// larger than L2 + MALL. Bit 0: `nt` loads, bit 1: `nt` stores; one macro per sweep kernel family, because they answer
// differently (profiles/r05_ab_nt.txt, launches interleaved in one process):
//  * ARMON_NT_X (the X sweep's 16-B global loads / stores): 3. Non-temporal LOADS too since round 5 — for the flavour they
//    pay for, the tuned fp64 perfect-gas sweep (x_nt_loads below): 2.755 -> 2.68-2.72 ms at 16384², 0.682 -> 0.666 at 8192²,
//    0.342 -> 0.330 at 4096 x 8192, every size 2.4-3.8 % — a strip is read once by one wave, and lines that are not kept do not
//    push the rest out. The same hint costs the Bizarrium sweep 2.4 % and the fp32 one 3.3 % (their waves hold their loads
//    longer / share lines inside the workgroup) and does nothing for the exact flavour: they keep ordinary loads.
//  * ARMON_NT_Y (the Y march's buffer loads / stores): 2. Its runs re-read 2·LAG halo rows that the run below has just
//    loaded: with `nt` loads they are gone (+4 % at 16384² with nt stores, +21 % without).
#ifdef ARMON_NT
#define ARMON_NT_X ARMON_NT
#define ARMON_NT_Y ARMON_NT
#endif
#ifndef ARMON_NT_X
#define ARMON_NT_X 3
#endif
#ifndef ARMON_NT_Y
#define ARMON_NT_Y 2
#endif
typedef real vreal2 __attribute__((ext_vector_type(2)));
template <bool NT = false>
__device__ __forceinline__ vec2 ld2(const real* p)
{
    const vreal2* q = reinterpret_cast<const vreal2*>(p);
    const vreal2 v = NT ? __builtin_nontemporal_load(q) : *q;
    return vec2{v.x, v.y};
}
// which instantiations of the X sweep load their strips non-temporally (see ARMON_NT_X above)
constexpr bool x_nt_loads(int eos, bool exact)
{
    return (ARMON_NT_X & 1) && sizeof(real) == 8 && eos == ARMON_EOS_PERFECT_GAS && !exact;
}
__device__ __forceinline__ void st2(real* p, real x, real y)
{
    vreal2* q = reinterpret_cast<vreal2*>(p);
    const vreal2 v = {x, y};
    if (ARMON_NT_X & 2) __builtin_nontemporal_store(v, q);
    else *q = v;
}

struct sweep_args {
    int64_t nx, ny, row_len;       // real cells and pitch of the arrays the sweep READS (nx + 2g; the pair's intermediate: line_pitch())
    int64_t out_len;               // pitch of the arrays it WRITES (p_out / c_out included); cell (x, y) sits at (y + g)·pitch + x + g in both
    int32_t g;                     // ghost layers
    int32_t bc_low, bc_high;       // mirror BC applied in-kernel on that side of the sweep axis
    int32_t emit;                  // bit 0: write p_out, bit 1: write c_out
    int32_t seg;                   // cells per run along the sweep axis (marching kernels)
    int32_t x_kernel;              // X sweep form: 0 spatial K=2, 3 spatial K=1, 2 LDS-transposed march
    int64_t o_lo, o_hi;            // cells to produce along the sweep axis: [o_lo, o_hi)
    int64_t x_first;               // X sweep: first cell of strip 0 (<= o_lo, sector-aligned in the ghosted row)
    int32_t xshift;                // Y sweep: columns the block origin is moved left (line-aligned row segments)
    int32_t xcd_remap;             // X sweep: XCD-aware workgroup placement (ARMON_X_XCD)
    int32_t gx = 0, gy = 0;        // X sweep: the launch's grid (gridDim comes from the dispatch packet: one more dependent scalar load)
    int32_t x_wg_along_x = 0;      // X sweep: a workgroup = kXSRows consecutive strips of one row (else: one strip of kXSRows rows)
    int32_t x_row_align = 0;       // X sweep: strip origins aligned row by row (row pitch not a multiple of a 64-B sector)
    int32_t y_sx = 0;              // Y sweep: rows are stored in sector-aligned windows handed over through LDS (see k_sweep_y)
    armon_dt_state* st = nullptr;   // device-resident time step (graph replay): dt is then a factor of st->current_dt
    real dt, dx, gamma;
    real inv_dx, dt_dx;            // 1 / dx and dt / dx in the run's precision (host; sweep_begin redoes dt / dx under a device-resident dt)
    real fa_low, ft_low, fa_high, ft_high;   // BC factors: axial / transverse velocity
    const real *rho_in, *ua_in, *ut_in, *E_in;    // ua = velocity along the sweep axis
    real *rho_out, *ua_out, *ut_out, *E_out;
    real *p_out, *c_out;
    real* partials;              // dt/CFL tracking: [2 * n_blocks] (max |u|±c, max |v|±c per workgroup)
    // whole-cycle kernel only: boundary of the SECOND (y) sweep — mirror flags and (u, v) factors per side
    int32_t bc_low_t = 0, bc_high_t = 0;
    real tu_low = 1, tv_low = 1, tu_high = 1, tv_high = 1;
};

// Source index and velocity factors of cell `j` (0-based real coordinate along the sweep axis, may be
// a ghost): physical boundaries mirror the inside (ref src/halo_exchange.jl:2-29), process boundaries
// read the ghost cells filled by the halo exchange.
__device__ __forceinline__ int64_t bc_source(const sweep_args& a, int64_t n, int64_t j, real& fa, real& ft)
{
    fa = 1;
    ft = 1;
    if (j < 0 && a.bc_low) {
        fa = a.fa_low;
        ft = a.ft_low;
        return -1 - j;
    }
    if (j >= n && a.bc_high) {
        fa = a.fa_high;
        ft = a.ft_high;
        return 2 * n - 1 - j;
    }
    return j;
}

// Device-resident time step (armon_dt_state): nothing to do once the time loop is over; otherwise the sweep's step is its
// factor times the cycle's step — the product the host forms in the run's precision (ref src/solver_state.jl:339-345) —
// and p is only materialised on the cycle the state machine marked as the last one.
__device__ __forceinline__ bool sweep_begin(sweep_args& a)
{
    if (a.st) {
        // nothing writes the state machine while a sweep runs (it steps in the fold kernel that follows), so it is read
        // through the constant address space: scalar loads whatever the compiler can prove about the rest of the kernel
        const auto* st = (const __attribute__((address_space(4))) armon_dt_state*)a.st;
        if (st->done) return false;
        a.dt = (real)st->current_dt * a.dt;
        a.dt_dx = a.dt / a.dx;
        if (!st->emit_p) a.emit &= ~1;
    }
    return true;
}

template <int... Is, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, Is...>, F&& f)
{
    (f(std::integral_constant<int, Is>{}), ...);
}

// Buffer addressing (T8): 128-bit resource descriptor in SGPRs + 32-bit lane offset + 32-bit scalar
// row offset. No per-access 64-bit VALU address arithmetic; advancing a row is one s_add_u32.
typedef unsigned int v2u __attribute__((ext_vector_type(2)));
using rsrc_t = __amdgpu_buffer_rsrc_t;

__device__ __forceinline__ rsrc_t make_rsrc(const void* p)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0xFFFFFFFFu, 0x00020000);
}
// gfx950 cache policy of a buffer access: bit 0 = sc0, bit 1 = nt, bit 4 = sc1 (ARMON_Y_AUX_LD / _ST: raw values, A/B builds)
#ifndef ARMON_Y_AUX_LD
#define ARMON_Y_AUX_LD ((ARMON_NT_Y & 1) ? 2 : 0)
#endif
#ifndef ARMON_Y_AUX_ST
#define ARMON_Y_AUX_ST ((ARMON_NT_Y & 2) ? 2 : 0)
#endif
constexpr int kAuxLoad = ARMON_Y_AUX_LD, kAuxStore = ARMON_Y_AUX_ST;
template <typename T> __device__ __forceinline__ T buf_load(rsrc_t r, unsigned voff, unsigned soff);
template <>
__device__ __forceinline__ double buf_load<double>(rsrc_t r, unsigned voff, unsigned soff)
{
    const v2u v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kAuxLoad);
    return __builtin_bit_cast(double, v);
}
// the Y march's non-temporal row loads (y_nt_loads in sweep_y_kernel.hpp): the ordinary policy + nt
__device__ __forceinline__ double buf_load_nt(rsrc_t r, unsigned voff, unsigned soff)
{
    const v2u v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kAuxLoad | 2);
    return __builtin_bit_cast(double, v);
}
template <>
__device__ __forceinline__ float buf_load<float>(rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, kAuxLoad));
}
__device__ __forceinline__ float2 buf_load2(rsrc_t r, unsigned voff, unsigned soff)      // fp32 pairs only
{
    // NB: cast the whole vector. Extracting .x/.y from the builtin's <2 x i32> result makes hipcc (ROCm 7.2) narrow
    // the load to one dword and hand element 0 to both users (seen in the ISA: buffer_load_dword + op_sel_hi:[0,1]).
    typedef float v2f __attribute__((ext_vector_type(2)));
    const v2f v = __builtin_bit_cast(v2f, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kAuxLoad));
    return float2{v.x, v.y};
}
__device__ __forceinline__ void buf_store2(rsrc_t r, unsigned voff, unsigned soff, float x, float y)
{
    const v2u v = {__builtin_bit_cast(unsigned int, x), __builtin_bit_cast(unsigned int, y)};
    __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, soff, kAuxStore);
}
__device__ __forceinline__ void buf_store(rsrc_t r, unsigned voff, unsigned soff, double x)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u, x), r, voff, soff, kAuxStore);
}
__device__ __forceinline__ void buf_store(rsrc_t r, unsigned voff, unsigned soff, float x)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, x), r, voff, soff, kAuxStore);
}

// dt/CFL tracking (ref src/reductions.jl:13-20). The reference takes min over cells of
// min(dx/|max(|u+c|,|u-c|)|, dy/|max(|v+c|,|v-c|)|); IEEE division is monotonic, so that minimum equals
// min(dx / max_cells(..u..), dy / max_cells(..v..)) bit for bit: track the two maxima, divide once.
struct cfl_track {
    real au = 0, av = 0;
    __device__ __forceinline__ void add(real u, real v, real c)
    {
#ifdef ARMON_CFL_PLAIN_MAX     // A/B builds (tools/build_variant.sh): the floating-point maxima of rounds 1-2, which drop a NaN
        au = phys::mx(au, phys::abs_(phys::mx(phys::abs_(u + c), phys::abs_(u - c))));
        av = phys::mx(av, phys::abs_(phys::mx(phys::abs_(v + c), phys::abs_(v - c))));
#else
        // max(|u + c|, |u - c|) = |u| + |c| — bit for bit, not only in exact arithmetic: the two candidates are fl(|u| + |c|)
        // and |fl(|u| - |c|)| in some order, and rounding is monotone and symmetric. One addition instead of two, two
        // absolute values and a select. amax: unsigned maximum of the bit patterns — the same maximum for these
        // non-negative values, and a NaN sticks.
#ifdef ARMON_CFL_TWO_SUMS      // A/B builds: the reference's expression as it stands
        au = phys::amax(au, phys::abs_(phys::mx(phys::abs_(u + c), phys::abs_(u - c))));
        av = phys::amax(av, phys::abs_(phys::mx(phys::abs_(v + c), phys::abs_(v - c))));
#else
        au = phys::amax(au, phys::abs_(u) + phys::abs_(c));
        av = phys::amax(av, phys::abs_(v) + phys::abs_(c));
#endif
#endif
    }
};

template <int NWAVES>
__device__ __forceinline__ void cfl_block_store(const cfl_track& t, real* partials, int64_t block, int tid)
{
    __shared__ real lds[NWAVES];
    const real au = red::block_reduce<red::op_max, NWAVES>(t.au, lds, tid);
    const real av = red::block_reduce<red::op_max, NWAVES>(t.av, lds, tid);
    if (tid == 0) {
        partials[2 * block] = au;
        partials[2 * block + 1] = av;
    }
}

constexpr int kFoldBlocks = 512;

// first level of the fold when a launch leaves more partial pairs than one workgroup should walk
__global__ void __launch_bounds__(256)
k_fold_pairs(const real* __restrict__ partials, int64_t n, real* __restrict__ out)
{
    __shared__ real lds[4];
    real au = 0, av = 0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
        const vec2 v = ld2(partials + 2 * k);
        au = phys::amax(au, v.x);
        av = phys::amax(av, v.y);
    }
    au = red::block_reduce<red::op_max, 4>(au, lds, threadIdx.x);
    av = red::block_reduce<red::op_max, 4>(av, lds, threadIdx.x);
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = au;
        out[2 * blockIdx.x + 1] = av;
    }
}

__global__ void __launch_bounds__(256)
k_fold_dt(const real* __restrict__ partials, int64_t n_blocks, real dx, real dy, real* __restrict__ out,
          int accumulate, armon_dt_state* st = nullptr)
{
    if (st && st->done) return;                     // the sweep did nothing either (graph replay past the last cycle)
    __shared__ real lds[4];
    real au = 0, av = 0;
    for (int64_t k = threadIdx.x; k < n_blocks; k += blockDim.x) {
        au = phys::amax(au, partials[2 * k]);
        av = phys::amax(av, partials[2 * k + 1]);
    }
    au = red::block_reduce<red::op_max, 4>(au, lds, threadIdx.x);
    av = red::block_reduce<red::op_max, 4>(av, lds, threadIdx.x);
    if (threadIdx.x == 0) {
        const real dt = phys::mn_nan(dx / au, dy / av);             // a NaN maximum gives a NaN step, and it wins
        out[0] = accumulate ? phys::mn_nan(out[0], dt) : dt;
        // graph replay: the state machine steps right here instead of in a kernel of its own (armon_dt_state::auto_step)
        if (st && st->auto_step && !accumulate)
            dt_state_step<real>(st, dt, (real)st->cfl, (real)st->maxtime, st->maxcycle, st->cst_dt, (real)st->Dt);
    }
}

// min(dx / max au, dy / max av) over `n` partial pairs into *out, on the context's stream
int fold_dt_launch(armon_ctx* ctx, real* partials, int64_t n, real dx, real dy, real* out, int accumulate,
                   armon_dt_state* st = nullptr)
{
    if (n > 16384) {
        real* level1 = partials + 2 * n;                      // room reserved by max_blocks()
        hipLaunchKernelGGL(k_fold_pairs, dim3(kFoldBlocks), dim3(256), 0, ctx->stream, partials, n, level1);
        int rc = check_launch("fold_pairs");
        if (rc != ARMON_OK) return rc;
        partials = level1;
        n = kFoldBlocks;
    }
    hipLaunchKernelGGL(k_fold_dt, dim3(1), dim3(256), 0, ctx->stream, partials, n, dx, dy, out, accumulate, st);
    return check_launch("fold_dt");
}

// ---- host side: what armon_hip_sweep and armon_hip_sweep_scalars both do with a descriptor ----------------------------------
// What both refuse, from the axis through the mirror factors (each then checks its own arrays). *lag: cells the
// scheme / projection reads past a cell.
int check_sweep_desc(const ARMON_SWEEP_DESC* d, int* lag_out)
{
    ARMON_REQUIRE(d->axis == ARMON_AXIS_X || d->axis == ARMON_AXIS_Y, "invalid axis %d", d->axis);
    ARMON_REQUIRE(d->scheme == ARMON_SCHEME_GODUNOV || d->scheme == ARMON_SCHEME_GAD, "unknown scheme %d", d->scheme);
    ARMON_REQUIRE(d->projection == ARMON_PROJECTION_EULER || d->projection == ARMON_PROJECTION_EULER_2ND,
                  "unknown projection %d", d->projection);
    ARMON_REQUIRE(d->eos == ARMON_EOS_PERFECT_GAS || d->eos == ARMON_EOS_BIZARRIUM, "unknown EOS %d", d->eos);
    ARMON_REQUIRE(d->scheme != ARMON_SCHEME_GAD || (d->limiter >= ARMON_LIMITER_NONE && d->limiter <= ARMON_LIMITER_SUPERBEE),
                  "unknown limiter tag %d", d->limiter);
    ARMON_REQUIRE(d->nx > 0 && d->ny > 0, "empty block %lld x %lld", (long long)d->nx, (long long)d->ny);
    ARMON_REQUIRE(d->ny < (1ll << 30) && d->nx < (1ll << 30), "block too large (%lld x %lld)", (long long)d->nx, (long long)d->ny);
    const int lag = (d->scheme == ARMON_SCHEME_GAD ? 1 : 0) + (d->projection == ARMON_PROJECTION_EULER_2ND ? 1 : 0) + 2;
    *lag_out = lag;
    ARMON_REQUIRE(d->nghost >= lag, "nghost = %d but this scheme/projection reads %d cells past the block", d->nghost, lag);
    const int64_t n_axis = d->axis == ARMON_AXIS_X ? d->nx : d->ny;
    ARMON_REQUIRE(!(d->bc_low || d->bc_high) || n_axis >= lag,
                  "mirror boundary needs at least %d cells along the sweep axis", lag);
    // The in-tile mirror scales the velocities of the mirrored cell and evaluates the EOS of the ghost cell from them, where
    // the reference copies p and c along with the state (ref src/halo_exchange.jl:2-29): the same bits when u² and v² are
    // unchanged, i.e. for factors of magnitude 1 — the only ones the reference has (ref src/tests.jl:150-161).
    ARMON_REQUIRE(!d->bc_low || (std::fabs(d->u_factor_low) == 1. && std::fabs(d->v_factor_low) == 1.),
                  "mirror factors of the low side must be +1 or -1 (got %g, %g)", d->u_factor_low, d->v_factor_low);
    ARMON_REQUIRE(!d->bc_high || (std::fabs(d->u_factor_high) == 1. && std::fabs(d->v_factor_high) == 1.),
                  "mirror factors of the high side must be +1 or -1 (got %g, %g)", d->u_factor_high, d->v_factor_high);
    return ARMON_OK;
}

// sweep_args of a checked descriptor with what every sweep sets: the block, the step, the mirrors (axial / transverse by the
// sweep axis) and the arrays it reads, of pitch `in_len`; it writes rows of `out_len`. Everything else is zero / null.
sweep_args base_sweep_args(const ARMON_SWEEP_DESC* d, int64_t in_len, int64_t out_len)
{
    sweep_args a{};
    a.nx = d->nx;
    a.ny = d->ny;
    a.row_len = in_len;
    a.out_len = out_len;
    a.g = d->nghost;
    a.bc_low = d->bc_low;
    a.bc_high = d->bc_high;
    a.dt = (real)d->dt;
    a.dx = (real)d->dx;
    a.gamma = (real)d->gamma;
    a.inv_dx = real(1) / a.dx;        // IEEE quotients: the bits the kernels' own divisions gave until round 4
    a.dt_dx = a.dt / a.dx;
    const bool X = d->axis == ARMON_AXIS_X;
    a.fa_low = (real)(X ? d->u_factor_low : d->v_factor_low);
    a.ft_low = (real)(X ? d->v_factor_low : d->u_factor_low);
    a.fa_high = (real)(X ? d->u_factor_high : d->v_factor_high);
    a.ft_high = (real)(X ? d->v_factor_high : d->u_factor_high);
    a.rho_in = d->rho_in;
    a.ua_in = X ? d->u_in : d->v_in;
    a.ut_in = X ? d->v_in : d->u_in;
    a.E_in = d->E_in;
    return a;
}

// The flavour a descriptor selects, as a type; PIPE: its marching pipeline.
template <int SCHEME_, int LIM_, int PROJ_, int EOS_, bool EXACT_>
struct flavour {
    static constexpr int SCHEME = SCHEME_, LIM = LIM_, PROJ = PROJ_, EOS = EOS_;
    static constexpr bool EXACT = EXACT_;
    using PIPE = typename std::conditional<EXACT, fused::Pipe<SCHEME, LIM, PROJ, EOS, real>,
                                           fused::PipeFast<SCHEME, LIM, PROJ, EOS, real>>::type;
};

// The ladder: f(flavour<...>{}) of a checked descriptor's scheme, limiter (Godunov has none), projection, EOS, arithmetic.
template <class F>
int with_flavour(const ARMON_SWEEP_DESC* d, F&& f)
{
    using std::integral_constant;
    auto by_exact = [&](auto s, auto l, auto p, auto e) {
        if (d->exact) return f(flavour<s.value, l.value, p.value, e.value, true>{});
        return f(flavour<s.value, l.value, p.value, e.value, false>{});
    };
    auto by_eos = [&](auto s, auto l, auto p) {
        if (d->eos == ARMON_EOS_BIZARRIUM) return by_exact(s, l, p, integral_constant<int, ARMON_EOS_BIZARRIUM>{});
        return by_exact(s, l, p, integral_constant<int, ARMON_EOS_PERFECT_GAS>{});
    };
    auto by_proj = [&](auto s, auto l) {
        if (d->projection == ARMON_PROJECTION_EULER_2ND) return by_eos(s, l, integral_constant<int, ARMON_PROJECTION_EULER_2ND>{});
        return by_eos(s, l, integral_constant<int, ARMON_PROJECTION_EULER>{});
    };
    const integral_constant<int, ARMON_SCHEME_GAD> gad;
    if (d->scheme == ARMON_SCHEME_GODUNOV)
        return by_proj(integral_constant<int, ARMON_SCHEME_GODUNOV>{}, integral_constant<int, ARMON_LIMITER_NONE>{});
    switch (d->limiter) {
    case ARMON_LIMITER_MINMOD: return by_proj(gad, integral_constant<int, ARMON_LIMITER_MINMOD>{});
    case ARMON_LIMITER_SUPERBEE: return by_proj(gad, integral_constant<int, ARMON_LIMITER_SUPERBEE>{});
    default: return by_proj(gad, integral_constant<int, ARMON_LIMITER_NONE>{});
    }
}

}  // namespace
