/*
 * armon_hip.h — C ABI of libarmon_hip.so, the MI355X (gfx950) device backend for the
 * direction-split hot path of Armon.jl.
 *
 * Every entry point below is what a Julia `ccall` (or any FFI) binds; no C++/torch types cross the
 * boundary. The design follows the reference's own precedent for a C-ABI kernel library, the Kokkos
 * extension: symbol = kernel name without `!` (ref src/generic_kernel.jl:616-620), iteration ranges
 * passed first as plain structs (ref src/generic_kernel.jl:576-614, ext/ArmonKokkos.jl:10-30),
 * limiter / test case as C int tags (ref ext/ArmonKokkos.jl:50-69), `flt_size`/`idx_size` sanity
 * exports (ref ext/ArmonKokkos.jl:122-139), errors reported through a return code + message
 * (ref ext/ArmonKokkos.jl:72-76 → `solver_error(:cpp, msg)`, ref src/utils.jl:108).
 *
 * Conventions
 *  - All floating point data is fp64 (`double`) unless the symbol ends in `_f32`.
 *  - All indices/strides are int64_t and 0-BASED on this side of the boundary (Julia subtracts 1).
 *  - Arrays are flat device pointers of `(Nx+2g)*(Ny+2g)` elements, x-contiguous rows
 *    (ref src/blocking/blocks.jl:18-50, src/blocking/blocking.jl:129-131). They are owned by the
 *    caller; the library never frees or retains them beyond the stream-ordered call.
 *  - Every kernel call is ASYNCHRONOUS on the context's stream and returns 0 on success or a
 *    non-zero `armon_status`; `armon_hip_last_error()` gives the message. `armon_hip_sync`
 *    implements `Base.wait(params)` (ref src/parameters.jl:1031-1038).
 *  - One host thread per context.
 */
#ifndef ARMON_HIP_H
#define ARMON_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(ARMON_BUILDING_LIB)
#define ARMON_API __attribute__((visibility("default")))
#else
#define ARMON_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------------------------- */
typedef enum {
    ARMON_OK = 0,
    ARMON_ERR_INVALID_ARG = 1,   /* bad range / null pointer / unsupported option          */
    ARMON_ERR_HIP = 2,           /* a HIP runtime call failed (message has hipGetErrorString) */
    ARMON_ERR_NO_DEVICE = 3,     /* no usable gfx950 device                                   */
    ARMON_ERR_INVALID_DT = 4     /* non finite or <= 0 time step (ref src/solver_state.jl:123) */
} armon_status;

/* ---- tags ------------------------------------------------------------------------------------ */
/* ref ext/ArmonKokkos.jl:50-57 (limiter tags), src/limiters.jl:6-8 */
enum { ARMON_LIMITER_NONE = 0, ARMON_LIMITER_MINMOD = 1, ARMON_LIMITER_SUPERBEE = 2 };
/* ref ext/ArmonKokkos.jl:60-69 (test tags), src/tests.jl:5-11; DebugIndexes ref src/tests.jl:195 */
enum { ARMON_TEST_SOD = 0, ARMON_TEST_SOD_Y = 1, ARMON_TEST_SOD_CIRC = 2, ARMON_TEST_BIZARRIUM = 3,
       ARMON_TEST_SEDOV = 4, ARMON_TEST_DEBUG_INDEXES = 5 };
/* ref src/riemann_schemes.jl:5-6 */
enum { ARMON_SCHEME_GODUNOV = 0, ARMON_SCHEME_GAD = 1 };
/* ref src/projection_schemes.jl:4-5 */
enum { ARMON_PROJECTION_EULER = 0, ARMON_PROJECTION_EULER_2ND = 1 };
/* EOS selected by the test case: ref src/kernels.jl:151-161 */
enum { ARMON_EOS_PERFECT_GAS = 0, ARMON_EOS_BIZARRIUM = 1 };
/* ref src/blocking/blocking.jl Axis / Side enums (Axis.X=1,Y=2; Side.Left=1,Right,Bottom,Top) */
enum { ARMON_AXIS_X = 0, ARMON_AXIS_Y = 1 };
enum { ARMON_SIDE_LEFT = 0, ARMON_SIDE_RIGHT = 1, ARMON_SIDE_BOTTOM = 2, ARMON_SIDE_TOP = 3 };
enum { ARMON_MEMCPY_H2D = 1, ARMON_MEMCPY_D2H = 2, ARMON_MEMCPY_D2D = 3 };

/*
 * Iteration range = the reference's DomainRange (ref src/domain_ranges.jl:39-61), 0-based:
 * cell index = col_start + j*col_step + row_start + i,  j in [0,col_len), i in [0,row_len).
 * From Julia: col_start = first(range.col)-1, col_step = step(range.col), col_len = length(range.col),
 *             row_start = first(range.row)-1, row_len = length(range.row).
 */
typedef struct {
    int64_t col_start, col_step, col_len;
    int64_t row_start, row_len;
} armon_range;

typedef struct armon_ctx armon_ctx;

/* ---- sanity / context (ref ext/ArmonKokkos.jl:122-139, src/parameters.jl:751-802,921-926) ---- */
ARMON_API int         armon_hip_flt_size(void);              /* sizeof(double) = 8                         */
ARMON_API int         armon_hip_idx_size(void);              /* sizeof(int64_t) = 8                        */
ARMON_API const char* armon_hip_version(void);
ARMON_API const char* armon_hip_last_error(void);            /* thread-local message of the last failure   */
ARMON_API int         armon_hip_device_count(int* count);

/* `stream` = an existing hipStream_t to enqueue on (e.g. the caller's), or NULL to create one. */
ARMON_API int armon_hip_init(int device_id, void* stream, armon_ctx** ctx);   /* create_device/init_backend */
ARMON_API int armon_hip_destroy(armon_ctx* ctx);
ARMON_API int armon_hip_sync(armon_ctx* ctx);                                  /* Base.wait(params)          */
ARMON_API int armon_hip_device_memory_info(armon_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
ARMON_API int armon_hip_device_name(armon_ctx* ctx, char* buf, size_t buf_len);
ARMON_API void* armon_hip_stream(armon_ctx* ctx);                              /* the hipStream_t in use     */
/* Tuning knobs of the fused sweeps (measurement tools and tests; no reference counterpart). A context reads the
 * environment variables of the same names ONCE, when it is created; this call changes them afterwards.
 * "ARMON_XS_NITER" strips per wave of the X sweep (values > 1 select the multi-strip form with its prefetch buffer, which only
 * the A/B build libarmon_hip_alt.so carries; the product library runs one strip per wave), "ARMON_Y_SEG" rows per run of the Y march (0 = automatic),
 * "ARMON_SWEEP_ALIGN" 0 = unaligned block/strip origins, "ARMON_Y_COLS1" 1 = fp32 Y march with one column per lane,
 * "ARMON_X_XCD" XCD-aware workgroup order of the X sweep: 1 = on, 0 = off, < 0 = automatic (on for fp64, off for fp32, whose
 * workgroups share their lines themselves), "ARMON_X_ROWS" workgroup shape of the X sweep: 1 = one strip of
 * 4 rows, 2 = 4 consecutive strips of one row, 0 = automatic (the former for fp64, the latter for fp32),
 * "ARMON_Y_SX" store exchange of the Y march (rows stored in sector-aligned windows handed over through LDS): 1 = always,
 * 2 = never, 0 = automatic (when the row pitch is not a multiple of a 64-B sector), "ARMON_Y_NT" non-temporal row loads of the
 * Y march: 2 = never, 0 = automatic (when the rows it reads are whole 128-B lines apart), "ARMON_PAIR_ONLY" armon_hip_sweep_pair
 * enqueues 1 = its X sweep only, 2 = its Y sweep only, 0 = both (not read from the environment), "ARMON_COPY_NT" the measurement aid
 * armon_hip_stream_copy4 with non-temporal loads (bit 0) / stores (bit 1), "PROFILE_WGS" cap on the workgroups of
 * armon_hip_profile / armon_hip_profile_bounds, 0 = automatic (not read from the environment).
 * None of them changes a result bit. */
ARMON_API int armon_hip_set_tuning(armon_ctx* ctx, const char* knob, int value);
/* the current value of a knob; and, read-only, "Y_RUN_ROWS": rows per run the last automatic choice of the Y march took (0
 * before the first Y sweep of the context) — tests use it to check that a shape really has several runs per column */
ARMON_API int armon_hip_get_tuning(armon_ctx* ctx, const char* knob, int* value);

/* device array type support: V{T,1}(undef, n) / copyto! (ref src/blocking/blocks.jl:36-44,121-143) */
ARMON_API int armon_hip_malloc(armon_ctx* ctx, size_t bytes, void** ptr);
ARMON_API int armon_hip_free(armon_ctx* ctx, void* ptr);
ARMON_API int armon_hip_memcpy(armon_ctx* ctx, void* dst, const void* src, size_t bytes, int kind); /* async */
ARMON_API int armon_hip_memset(armon_ctx* ctx, void* dst, int byte_value, size_t bytes);             /* async */
/* Pinned host memory + truly asynchronous copies: how the host reads the fused dt/CFL scalar one cycle late
 * (the reference consumes a cycle's reduction in the NEXT cycle, src/solver_state.jl:89-99,145-166) without ever
 * draining the stream: memcpy_async into a pinned slot, event_record, and event_sync a cycle later. The host
 * buffer of memcpy_async must come from malloc_host and stay untouched until the copy's event has completed. */
ARMON_API int armon_hip_malloc_host(armon_ctx* ctx, size_t bytes, void** ptr);
ARMON_API int armon_hip_free_host(armon_ctx* ctx, void* ptr);
ARMON_API int armon_hip_memcpy_async(armon_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);

/* Measurement aid (bench.py): plain streaming copy of four arrays into four others in ONE launch —
 * the traffic shape of a fused sweep (4 read + 4 written, 16 B per lane) with no arithmetic. Its rate on
 * the device at hand is the practical ceiling the sweep kernels are compared with, next to the 8 TB/s
 * spec. `bytes` per array, multiple of 16; async on the context's stream. No reference counterpart. */
ARMON_API int armon_hip_stream_copy4(armon_ctx* ctx, const void* const in[4], void* const out[4], size_t bytes);

/* stream timers for benchmarks (hipEvents on the context's stream).
 * event_record/event_elapsed: a pool of ARMON_HIP_MAX_EVENTS reusable events, recorded without any
 * host synchronisation; event_elapsed_ms synchronises on event `b` and returns t(b) - t(a). */
#define ARMON_HIP_MAX_EVENTS 1024
ARMON_API int armon_hip_event_record(armon_ctx* ctx, int slot);
ARMON_API int armon_hip_event_elapsed_ms(armon_ctx* ctx, int a, int b, double* elapsed_ms);
ARMON_API int armon_hip_event_sync(armon_ctx* ctx, int slot);                   /* host waits for that event only */
ARMON_API int armon_hip_timer_start(armon_ctx* ctx);
ARMON_API int armon_hip_timer_stop(armon_ctx* ctx, double* elapsed_ms);        /* synchronises on the stop event */

/* ---- staged kernels: one per reference @generic_kernel ---------------------------------------- */

/* perfect_gas_EOS!(params, data, range, γ)           ref src/kernels.jl:4-13, call :154 */
ARMON_API int armon_hip_perfect_gas_EOS(armon_ctx*, armon_range, double gamma,
        const double* rho, const double* E, const double* u, const double* v,
        double* p, double* c, double* g);

/* bizarrium_EOS!(params, data, range)                ref src/kernels.jl:16-55, call :160 */
ARMON_API int armon_hip_bizarrium_EOS(armon_ctx*, armon_range,
        const double* rho, const double* u, const double* v, const double* E,
        double* p, double* c, double* g);

/* acoustic!(params, data, range, s, uˢ_, pˢ_, uₐ)    ref src/riemann_schemes.jl:33-52 */
ARMON_API int armon_hip_acoustic(armon_ctx*, armon_range, int64_t s, double* us, double* ps,
        const double* rho, const double* ua, const double* p, const double* c);

/* acoustic_GAD!(params, data, range, s, dt, dx, uₐ, lim)   ref src/riemann_schemes.jl:55-113 */
ARMON_API int armon_hip_acoustic_GAD(armon_ctx*, armon_range, int64_t s, double dt, double dx,
        double* us, double* ps,
        const double* rho, const double* ua, const double* p, const double* c, int limiter);

/* cell_update!(params, data, range, s, dx, dt, uₐ)   ref src/kernels.jl:58-68,217-223 */
ARMON_API int armon_hip_cell_update(armon_ctx*, armon_range, int64_t s, double dx, double dt,
        const double* us, const double* ps, double* rho, double* ua, double* E);

/* advection_first_order!(params, data, range, s, dt, a_ρ, a_uρ, a_vρ, a_Eρ)
 *                                                    ref src/projection_schemes.jl:62-89 */
ARMON_API int armon_hip_advection_first_order(armon_ctx*, armon_range, int64_t s, double dt,
        const double* us, const double* rho, const double* u, const double* v, const double* E,
        double* adv_rho, double* adv_urho, double* adv_vrho, double* adv_Erho);

/* advection_second_order!(params, data, range, s, dx, dt, a×4)
 *                                                    ref src/projection_schemes.jl:15-20,92-135 */
ARMON_API int armon_hip_advection_second_order(armon_ctx*, armon_range, int64_t s, double dx, double dt,
        const double* us, const double* rho, const double* u, const double* v, const double* E,
        double* adv_rho, double* adv_urho, double* adv_vrho, double* adv_Erho);

/* euler_projection!(params, data, range, s, dx, dt, a×4)   ref src/projection_schemes.jl:23-52 */
ARMON_API int armon_hip_euler_projection(armon_ctx*, armon_range, int64_t s, double dx, double dt,
        const double* us, double* rho, double* u, double* v, double* E,
        const double* adv_rho, const double* adv_urho, const double* adv_vrho, const double* adv_Erho);

/* boundary_conditions!(params, data, range, bsize, axis, side, u_factor, v_factor)
 * ref src/halo_exchange.jl:2-36. `range` = border_domain(bsize, side) (one strip of real cells);
 * `incr` = ±stride_along(bsize, axis), signed towards the edge (ref :8-10); `nghost` = ghosts(bsize). */
ARMON_API int armon_hip_boundary_conditions(armon_ctx*, armon_range, int64_t incr, int nghost,
        double u_factor, double v_factor,
        double* rho, double* u, double* v, double* p, double* c, double* g, double* E);

/* pack_to_array!/unpack_from_array!(params, range, bsize, side, array, vars)
 * ref src/halo_exchange.jl:187-216. `range` = border_domain / ghost_domain (single_strip=false);
 * `face` = real_face_size(bsize, side); buffer index (i_g*face + i)*nvars + v with
 * (i, i_g) = divrem(iter, nghost), iter = 0-based position in the range (row-major).
 * `vars` = HOST array of `nvars` device pointers (comm_vars: ρ,u,v,E,p,c,g  ref src/blocking/blocks.jl:50). */
ARMON_API int armon_hip_pack_to_array(armon_ctx*, armon_range, int nghost, int64_t face,
        double* array, int nvars, const double* const* vars);
ARMON_API int armon_hip_unpack_from_array(armon_ctx*, armon_range, int nghost, int64_t face,
        const double* array, int nvars, double* const* vars);

/* dtCFL_kernel(params, state, blk, Δx)::T            ref src/reductions.jl:2-110
 * Min over `range` (real cells) of min(dx/max|u±c|, dy/max|v±c|). Two forms:
 *  _async: result left in device memory `*result_dev` (one double), no host sync;
 *  plain : synchronises and returns the value in `*result_host`. */
ARMON_API int armon_hip_dtCFL_async(armon_ctx*, armon_range, double dx, double dy,
        const double* u, const double* v, const double* c, double* result_dev);
ARMON_API int armon_hip_dtCFL(armon_ctx*, armon_range, double dx, double dy,
        const double* u, const double* v, const double* c, double* result_host);

/* conservation_vars(params, blk)::(T,T)              ref src/reductions.jl:202-323
 * out[0] = ds*Σρ, out[1] = ds*ΣρE over `range`; synchronises. */
ARMON_API int armon_hip_conservation_vars(armon_ctx*, armon_range, double ds,
        const double* rho, const double* E, double out_host[2]);

/* init_test(params, data, range, global_pos, bsize, ΔX, vars_to_zero, test_case)
 * ref src/kernels.jl:71-145,176-207, src/tests.jl:59-121.
 * `range` = full domain (real+ghost); row_length = Nx+2g; global_pos = 0-based global index of the
 * block's first real cell (ref src/kernels.jl:181-182); global_N = global grid (for DebugIndexes);
 * sedov_r (ref src/tests.jl:15-19) is only read for ARMON_TEST_SEDOV. All 16 arrays are written; x, y, rho, u, v, E are
 * required, any of the other ten may be NULL and is then skipped — the reference's `vars_to_zero` argument (ref
 * src/kernels.jl:142-144,188-191): a host that runs the fused sweeps only never reads us, ps, work_1..4 and mask. */
typedef struct {
    double *x, *y, *rho, *u, *v, *E, *p, *c, *g, *us, *ps, *work_1, *work_2, *work_3, *work_4, *mask;
} armon_block_data;   /* ref src/blocking/blocks.jl:18-35 (BlockData) */

ARMON_API int armon_hip_init_test(armon_ctx*, armon_range, int test, int64_t row_length, int64_t col_length,
        int nghost, const int64_t global_pos[2], const int64_t global_N[2],
        const double origin[2], const double dX[2], double sedov_r, const armon_block_data* data);

/* User-defined initial states (csrc/init_regions.hip; no reference counterpart): a background state
 * and a list of regions, each with a state of its own. OVERWRITES rho, u, v, E on `range` (ghost cells included when the
 * range holds them, as init_test does over the full domain) and nothing else: a host first calls armon_hip_init_test with
 * any two-state tag for x, y, mask and the zeroed work vectors, then this. row_length, nghost, global_pos, origin, dX as for
 * armon_hip_init_test. A cell's state depends on its GLOBAL position only, so tiles and ghost widths change no bit.
 * All arithmetic in the data type, one IEEE operation per operation written, comparisons inclusive:
 *   corner   x = (T)gx dX[0] + origin[0],  y likewise (init_test's own formulas)
 *   samples  xs_i = x + dX[0] T((2 i + 1) / (2 samples)), i = 0 .. samples - 1, the same along y: samples^2 points per cell
 *            (samples = 1: init_test's x + dX/2, bit for bit)
 *   HALF_PLANE  a0 xs + a1 ys <= a2
 *   BOX         a0 <= xs && xs <= a1 && a2 <= ys && ys <= a3      (+-inf = an open side)
 *   DISC        (xs - a0)(xs - a0) + (ys - a1)(ys - a1) <= a2      (a2 = r^2)
 *   ELLIPSE     (xs - a0)(xs - a0) a2 + (ys - a1)(ys - a1) a3 <= 1 (a2, a3 = 1/rx^2, 1/ry^2, rounded by the caller)
 * A point belongs to the LAST region of the list that holds it, to the background if none does. A cell whose samples all
 * belong to the same region (or all to the background) stores that state verbatim. Any other cell accumulates, y sample
 * outer, x sample inner, m += rho, mu += rho u, mv += rho v, mE += rho E and stores rho = m / T(samples^2), u = mu / m,
 * v = mv / m, E = mE / m: the conservative mix of mass, momentum and total energy.
 * Refused (ARMON_ERR_INVALID_ARG, before any launch, nothing written): a NULL pointer, nregions outside 0 .. 32, an unknown
 * kind, samples not 1, 2, 4 or 8, a NaN anywhere, an infinity anywhere but in the bounds of a BOX, a rho <= 0, an origin or
 * dX that is not finite, dX <= 0. `background` and `regions` are HOST memory, read before the call returns (the table is a
 * kernel argument: no allocation, no copy, no synchronisation). Async on the context's stream. */
enum { ARMON_REGION_HALF_PLANE = 0, ARMON_REGION_BOX = 1, ARMON_REGION_DISC = 2, ARMON_REGION_ELLIPSE = 3 };
typedef struct { int32_t kind, reserved; double a[4]; double rho, u, v, E; } armon_region;
typedef struct { int32_t kind, reserved; float a[4]; float rho, u, v, E; } armon_region_f32;

ARMON_API int armon_hip_init_regions(armon_ctx*, armon_range, int64_t row_length, int nghost,
        const int64_t global_pos[2], const double origin[2], const double dX[2], int samples,
        const double background[4] /* rho, u, v, E */, int nregions, const armon_region* regions,
        double* rho, double* u, double* v, double* E);
ARMON_API int armon_hip_init_regions_f32(armon_ctx*, armon_range, int64_t row_length, int nghost,
        const int64_t global_pos[2], const float origin[2], const float dX[2], int samples,
        const float background[4], int nregions, const armon_region_f32* regions,
        float* rho, float* u, float* v, float* E);

/* Body forces (csrc/body_force.hip; no reference counterpart): a constant acceleration (gx, gy)
 * applied as one kick at the end of every cycle. The rule, word for word:
 * A body force is a constant acceleration (gx, gy). Each cycle ends with a kick. The kick uses that cycle's full step
 * dt = current_dt, whatever the axis splitting and its factors. It touches every real cell and no ghost cell. It is
 * evaluated in the data type T, one IEEE operation per operation written (the library is built with -ffp-contract=off, so
 * no FMA appears):
 *   hx = T(0.5) * dt * gx          hy = T(0.5) * dt * gy          (uniform, formed once per launch)
 *   E  = E + dt * (gx * (u + hx) + gy * (v + hy))                  (u, v: the values BEFORE the kick)
 *   u  = u + dt * gx               v  = v + dt * gy
 * This is E += 1/2 (|u'|^2 - |u|^2) without its cancellation: the internal energy, and so p and c, do not change except by
 * rounding. A component whose g is exactly zero is neither read for its own sake nor written: with gx == 0 the u plane is
 * not written (a -0.0 stays -0.0) and not read (its term is left out of the sum: E = E + dt * (gy * (v + hy))); the same for
 * gy and v. With both components zero nothing is launched. The products are formed left to right: (T(0.5) * dt) * gx.
 * `real` is the range of the cells to kick (a block's real cells; any armon_range is walked like every staged kernel's).
 * dt, gx, gy arrive as doubles and are rounded to T before anything else (the _f32 entry takes floats).
 * Refused (ARMON_ERR_INVALID_ARG, before any launch, nothing written; armon_hip_last_error names the argument): a NULL ctx,
 * an invalid range, a dt, gx or gy that is a NaN or an infinity, a NULL E when either component is non-zero, a NULL u with
 * gx != 0, a NULL v with gy != 0 (a plane that is not touched may be NULL). Traffic per fp64 cell: one component 32 B
 * (2 planes read, 2 written), both 48 B. Async on the context's stream. */
ARMON_API int armon_hip_body_force(armon_ctx* ctx, armon_range real, double dt, double gx, double gy,
        double* u, double* v, double* E);
ARMON_API int armon_hip_body_force_f32(armon_ctx* ctx, armon_range real, float dt, float gx, float gy,
        float* u, float* v, float* E);

/* Periodic sides (csrc/periodic.hip; the oracle's periodic_ghosts, no reference counterpart: the
 * reference's domain is never periodic): the ghost cells of a periodic axis are filled from the opposite border of the same
 * block, after which a sweep treats both sides of that axis as sides whose ghosts already hold neighbour data (bc_low =
 * bc_high = 0). The rule, word for word, for each of the nvars <= 8 vectors, with cell (x, y) at
 * (y + nghost)·row_length + x + nghost:
 * n is the number of real cells along `axis` (nx for axis 0, ny for axis 1). Every real index k across the axis (every row
 * for axis 0, every column for axis 1) and every l < layers is covered. Ghost -1-l takes real cell n-1-l. Ghost n+l takes
 * real cell l.
 * The call reads real cells only. It writes exactly the 2·layers·m ghost cells of the two sides along `axis` (m = the real
 * cells across it) and nothing else: no corner, no real cell, no ghost of the other axis, no padding past nx + 2·nghost when
 * row_length is larger (any row_length >= nx + 2·nghost is a valid pitch, that of armon_hip_sweep_pair's intermediate
 * included). Values are moved, not computed: NaN payloads and signed zeros arrive as they are.
 * `vars` is a HOST array of nvars device pointers (copied into the launch: it may be released on return).
 * Refused (ARMON_ERR_INVALID_ARG, before any launch, nothing written; armon_hip_last_error names the argument): a NULL ctx,
 * a NULL vars or vars[k], nvars outside 1..8, layers outside 1..nghost, n < layers, row_length < nx + 2·nghost, an axis other
 * than 0 or 1 (and nx or ny outside 1..2^31-1). One launch for all variables and both sides, a 1-D grid with 64-bit item
 * numbers (any number of rows). Asynchronous on the context's stream, no scratch, can be captured into a graph. */
ARMON_API int armon_hip_periodic_ghosts(armon_ctx*, int axis, int64_t row_length, int nghost, int layers,
        int64_t nx, int64_t ny, int nvars, double* const* vars /* HOST array of device pointers */);
ARMON_API int armon_hip_periodic_ghosts_f32(armon_ctx*, int axis, int64_t row_length, int nghost, int layers,
        int64_t nx, int64_t ny, int nvars, float* const* vars);

/* ---- in-situ reduced output (no reference counterpart: the reference writes whole fields, ref src/io.jl:2-27) ---- */
/* Conservative coarsening of one block by the integer factors (fx, fy) >= 1. The block has rows of `row_length` elements,
 * `nghost` ghost layers and nx x ny real cells (row_length >= nx + 2 nghost); only real cells are read. Coarse cell (I, J)
 * covers the real cells i in [I fx, min((I+1) fx, nx)), j in [J fy, min((J+1) fy, ny)) — n cells; the coarse grid is
 * cnx x cny = ceil(nx/fx) x ceil(ny/fy). `out_dev` receives five dense planes [cny][cnx], in this order:
 *   rho = S(rho)/n,  u = S(rho u)/S(rho),  v = S(rho v)/S(rho),  E = S(rho E)/S(rho),  p = S(p)/n
 * (cells are uniform: volume averages of rho and p, mass-weighted averages of u, v, E; n rho_c ds summed over the coarse
 * cells is the mass armon_hip_conservation_vars returns). `p` may be NULL: the fifth plane is then left untouched, and
 * `out_dev` may hold four planes only. One pass over the 4 (5) vectors, no atomics; the value of a coarse cell is a fixed
 * function of the values it covers — the same summation order (csrc/coarsen.hip) wherever the block sits in memory and
 * whatever the grid size. fx a power of two <= 64 with fy <= 64 is one kernel and needs no scratch. Any other factor takes
 * two kernels through the context's reduction scratch, which must hold nx * ceil(ny / min(fy, 64)) elements per plane read
 * (4, or 5 with p): 1/64 of the fields for fy >= 64, but as much as the fields themselves for fy = 1 (8.6 GB at 16384^2
 * fp64 without p). That scratch grows, with one stream synchronisation, the first time it is too small, stays with the
 * context until armon_hip_destroy, and — like every reduction scratch of this library — cannot grow inside a stream
 * capture or while a captured graph of the context is alive (ARMON_ERR_INVALID_ARG then: run the call once before
 * capturing). Async on the context's stream. */
ARMON_API int armon_hip_coarsen(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
        const double* rho, const double* u, const double* v, const double* E, const double* p, double* out_dev);

/* Strided gather: out_dev[q*count + i] = vars[q][start + i*stride], q < nvars <= 8, i < count. `vars` = HOST array of
 * `nvars` device pointers to vectors of `n_cells` elements; a slice that leaves [0, n_cells) is refused. The middle row of a
 * block is stride 1, its middle column stride = row pitch, its diagonal stride = row pitch + 1. Async on the stream. */
ARMON_API int armon_hip_gather_strided(armon_ctx*, int64_t n_cells, int nvars, const double* const* vars,
        int64_t start, int64_t stride, int64_t count, double* out_dev);

/* ---- derived flow fields for in-situ images (no reference counterpart; csrc/derive.hip) ---- */
enum { ARMON_DERIVE_RHO, ARMON_DERIVE_P, ARMON_DERIVE_EINT, ARMON_DERIVE_SPEED, ARMON_DERIVE_MACH,
       ARMON_DERIVE_GRAD_RHO, ARMON_DERIVE_VORTICITY, ARMON_DERIVE_DIVERGENCE, ARMON_DERIVE_COUNT };
enum { ARMON_REDUCE_MEAN, ARMON_REDUCE_MAX, ARMON_REDUCE_MIN };
typedef struct {
    int32_t nq, quantity[8], reduce[8]; /* 1 .. 8 planes: ARMON_DERIVE_* and ARMON_REDUCE_* of each                */
    int32_t eos;            /* ARMON_EOS_*                                                                           */
    int32_t neighbours;     /* bit 0 left, 1 right, 2 bottom (row -1), 3 top: the FIRST ghost layer of that side holds
                               the neighbour tile's cells                                                            */
    double gamma, dx, dy;   /* perfect gas: its gamma; the cell sizes, converted to the data type                    */
} armon_derive_spec;        /* HOST memory, read before the call returns */

/* One pass over the real cells of a block (described as in armon_hip_coarsen): per cell up to 8 selected quantities from
 * rho, u, v, E, each reduced over the fx x fy coarse cells of armon_hip_coarsen (same cell -> coarse cell map, same
 * clamping of a factor larger than the grid) into the dense planes out_dev[nq][cny][cnx] of the data type. No p vector is
 * read: pressure and sound speed are the EOS of the cell itself, as in armon_hip_profile. 32 B read per fp64 cell, plus the
 * two rows around each chunk of 64 rows when a stencil quantity is selected.
 *   PER CELL, all arithmetic in the data type, one IEEE operation per operation written, IEEE division and square root:
 *     e = E - 0.5 (u u + v v);  p, c = the EOS (perfect gas: p = (gamma - 1) rho e, c = sqrt((gamma p) / rho))
 *     speed = sqrt(u u + v v);  mach = speed / c
 *     d_x f = (f_R - f_L) / (T(w) dx): f_R = f[i+1] if that cell exists, else f[i]; f_L likewise; w = how many of the two
 *             exist; w = 0: the derivative is 0 and nothing is divided; d_y likewise with dy. A neighbour exists if it is a
 *             real cell of this block or lies in the first ghost layer of a side whose bit of `neighbours` is set: central
 *             differences inside and across tile edges, one-sided ones at the edge of the global domain.
 *     grad_rho = sqrt(gx gx + gy gy);  vorticity = d_x v - d_y u;  divergence = d_x u + d_y v
 *   Only the four edge-adjacent ghost strips of flagged sides are read: no corner, no deeper layer, no ghost cell of an
 *   unflagged side.
 *   REDUCTION: ARMON_REDUCE_MEAN = the sum, in the summation order of armon_hip_coarsen (csrc/coarsen.hip), divided by the
 *   number of cells covered: a function of the values covered only, not of the launch shape, the alignment path, the ghost
 *   width or the tile split. MAX / MIN: plain, +0 above -0. In all three a NaN among the covered values gives the canonical
 *   quiet NaN.
 * fx a power of two <= 64 with fy <= 64 is one kernel and needs no scratch. Any other factor takes two kernels through the
 * context's reduction scratch, which must hold nq * nx * ceil(ny / min(fy, 64)) elements of the data type; it grows, stays
 * and is refused inside a capture exactly as for armon_hip_coarsen. Refused (ARMON_ERR_INVALID_ARG, before any launch,
 * nothing written): a NULL pointer, nq outside 1 .. 8, an unknown quantity, reduction or EOS, dx or dy not finite and > 0,
 * factors < 1, a bit of `neighbours` set with nghost == 0, and the block checks of armon_hip_coarsen. Async on the stream. */
ARMON_API int armon_hip_derive(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
        const double* rho, const double* u, const double* v, const double* E, const armon_derive_spec* spec, double* out_dev);

/* ---- checkpoint / restart (no reference counterpart; csrc/checkpoint.hip) ---- */
/* Move a window of REAL cells between the vectors of one block and a dense buffer, and digest it, in one pass. The block has
 * rows of `row_length` elements, `nghost` ghost layers and nx x ny real cells; the window is the real cells
 * [col0, col0 + wnx) x [row0, row0 + wny) and may not leave the real domain; no ghost cell is read or written. `vars` = HOST
 * array of `nvars` <= 8 device pointers; the dense side is [nvars][wny][wnx] in device memory. `global_first` = global 0-based
 * index gy * global_nx + gx of the window's first cell, `global_nx` the global row length.
 * state_pack: vectors -> dense (`dense_dev` NULL = digest only); state_unpack: dense -> vectors (digest of what it wrote).
 * Both ADD to `digest_dev[k]` (device, one 64-bit word per variable, cleared by the caller) the sum mod 2^64 over the cells of
 *     mix64(b + mix64(8 g + k + 1)),   b = the value's bit pattern zero-extended to 64 bits, g = its global index,
 *     mix64(z): z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31
 * — a function of the values and their global positions only, so the digests of the parts of a domain add up to the
 * digest of the domain whatever the split. Async on the context's stream, no atomics. One partial per workgroup and variable
 * goes through the context's reduction scratch (8 x 8 x CUs words at most): like every reduction of this library the call
 * synchronises the stream ONCE if that scratch has to grow, and is refused (ARMON_ERR_INVALID_ARG) when it would have to grow
 * inside a stream capture or while a captured graph of the context is alive. Otherwise no host synchronisation. */
ARMON_API int armon_hip_state_pack(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
        const double* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
        int64_t global_nx, double* dense_dev, uint64_t* digest_dev);
ARMON_API int armon_hip_state_unpack(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
        double* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
        int64_t global_nx, const double* dense_dev, uint64_t* digest_dev);

/* ---- lossless plane codec "xorplane16" of packed checkpoints (no reference counterpart; csrc/plane_codec.hip) ---- */
/* A CHUNK encodes one dense plane of `rows` x `wnx` elements of W = 64 or 32 bits, row-major; u[r][c] = the bit pattern.
 *   t[r][c] = u[r][c] if r % 16 == 0, else u[r][c] ^ u[r-1][c]                    (row blocks of 16 rows from the first row)
 *   a row is cut into G = ceil(wnx / 64) groups of 64 columns; group g = r G + j, n = rows G; lane l = column 64 j + l
 *   base = t[r][64 j]; res[0] = 0; res[l] = t[r][64 j + l] ^ t[r][64 j + l - 1] inside the plane, 0 past it
 *   mask = OR of res over the lanes; per set bit k of mask, ascending, one 64-bit word whose bit l is bit k of res[l]
 * Chunk bytes, little-endian: base[n] (W/8 bytes each, zero-padded to a multiple of 8), mask[n] (the same), then the words
 * of group 0, 1, ... back to back: 2 pad8(n W / 8) + 8 sum popcount(mask) bytes, a function of the values and the shape only.
 * armon_hip_plane_encode_bound: the largest chunk of that shape, 2 pad8(n W / 8) + 8 W n (0 for an invalid shape or width).
 * armon_hip_plane_encode: `dense_dev` = [nplanes][rows][wnx], nplanes <= 8; the chunk of plane q lands at
 * `out_dev + q * plane_capacity` (device, 8-byte aligned), its size in `sizes_dev[q]` (device); no byte past that size is
 * written. `plane_capacity` must be a multiple of 8 and at least the bound.
 * armon_hip_plane_decode: the sub-window [col0, col0 + snx) x [row0, row0 + sny) of the chunk at `chunk_dev` (device, 8-byte
 * aligned, `chunk_bytes` long) into the dense `out_dev` = [sny][snx]. Nothing past `chunk_bytes` is read: a group whose words
 * would end beyond it decodes as if it had none and sets `*status_dev` (device, cleared by the caller) to 1. Whether a chunk
 * is consistent is the host's to check before it gets here (plane_codec.check_chunk).
 * Both are async on the context's stream, use no atomics, and keep the offsets of the groups (n 64-bit words per plane, plus
 * one per 2048) in the context's reduction scratch, which grows as in armon_hip_state_pack: one stream synchronisation, refused
 * inside a capture or while a captured graph is alive. Refused (ARMON_ERR_INVALID_ARG, before any launch): a NULL context or
 * pointer, non-positive sizes, a capacity below the bound, a sub-window that leaves the chunk, `chunk_bytes` below the tables. */
ARMON_API uint64_t armon_hip_plane_encode_bound(int elem_bytes, int64_t rows, int64_t wnx);
ARMON_API int armon_hip_plane_encode(armon_ctx*, const double* dense_dev, int nplanes, int64_t rows, int64_t wnx,
        void* out_dev, uint64_t plane_capacity, uint64_t* sizes_dev);
ARMON_API int armon_hip_plane_decode(armon_ctx*, const void* chunk_dev, uint64_t chunk_bytes, int64_t rows, int64_t wnx,
        int64_t col0, int64_t row0, int64_t snx, int64_t sny, double* out_dev, uint32_t* status_dev);

/* ---- state comparison on the device (no reference counterpart; csrc/state_compare.hip) ---- */
/* What separates two states, per variable: 64 bytes, every field MERGES (counts add, first_out is a minimum, a (value, position)
 * pair takes the larger bit pattern and on equal patterns the smaller position), so the record of a domain is the merge of
 * the records of its parts whatever the split, and does not depend on the launch shape, the alignment, the ghost width or the
 * decomposition. Positions are GLOBAL 0-based indices g = gy * global_nx + gx. */
typedef struct {
    uint64_t n_cells;       /* cells compared                                                          (sum) */
    uint64_t n_bits;        /* cells whose bit patterns differ                                         (sum) */
    uint64_t n_out;         /* cells outside the tolerance                                             (sum) */
    uint64_t first_out;     /* smallest g of such a cell, UINT64_MAX = none                            (min) */
    uint64_t max_abs;       /* bit pattern, zero-extended, of the largest d                            (pair max) */
    uint64_t max_abs_at;    /* smallest g that attains it; UINT64_MAX while max_abs == 0 */
    uint64_t max_rel;       /* the same for d / m                                                      (pair max) */
    uint64_t max_rel_at;
} armon_state_diff;

/* Write the neutral element of the merge (zeros, positions UINT64_MAX) into diff_dev[0 .. nvars), 1 <= nvars <= 8. Async. */
ARMON_API int armon_hip_state_diff_reset(armon_ctx*, int nvars, armon_state_diff* diff_dev);

/* Compare the window of REAL cells [col0, col0 + wnx) x [row0, row0 + wny) of the `nvars` <= 8 vectors of one block with the
 * dense reference `ref_dense_dev` = [nvars][wny][wnx] (device memory) and MERGE the result into diff_dev[0 .. nvars). Block,
 * window, `vars`, `global_first`, `global_nx` and their checks are those of armon_hip_state_pack; in addition `ref_dense_dev`
 * and `diff_dev` must not be NULL and rtol, atol must be >= 0 and not NaN (ARMON_ERR_INVALID_ARG otherwise, nothing written).
 * Per cell, a = the vector's value, b = the reference's, all arithmetic in the data type (rtol, atol converted to it on the
 * host), no contraction, correctly rounded division:
 *     same = (a == b) or both are NaN:  d = 0 and the relative difference is 0   (equal infinities included);
 *     otherwise  d = |a - b|,  m = max(|a|, |b|),  relative difference = d / m;
 *     within tolerance = same, or both finite and d <= max(atol, rtol * m)
 * — Julia's isapprox as the reference's tests use it, two NaNs counted as equal. A cell counts for n_bits when the bit
 * patterns differ (-0.0 against +0.0: n_bits, not n_out). A NaN in d or d / m enters the maxima as the canonical quiet NaN
 * (0x7ff8000000000000 / 0x7fc00000): the unsigned maximum of bit patterns is then sticky and unique.
 * `row_out_dev` (device, [nvars][wny] 32-bit words zeroed by the caller, or NULL): row_out_dev[q * wny + r] += the cells of
 * window row r of variable q that are outside the tolerance (integer atomic add: order-independent).
 * No ghost cell is read, nothing outside the dense window is read, nothing is written except diff_dev, row_out_dev and the
 * context's reduction scratch (7 x 8 x CUs words at most), which grows as in armon_hip_state_pack: one stream synchronisation
 * the first time, refused inside a stream capture or while a captured graph of the context is alive. Async on the stream. */
ARMON_API int armon_hip_state_compare(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
        const double* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
        int64_t global_nx, const double* ref_dense_dev, double rtol, double atol, armon_state_diff* diff_dev,
        uint32_t* row_out_dev);
ARMON_API int armon_hip_state_compare_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
        const float* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
        int64_t global_nx, const float* ref_dense_dev, double rtol, double atol, armon_state_diff* diff_dev,
        uint32_t* row_out_dev);

/* ---- in-situ profiles: exact binned sums along x, y or a radius (no reference counterpart; csrc/profile.hip) ---- */
enum { ARMON_PROFILE_X = 0, ARMON_PROFILE_Y = 1, ARMON_PROFILE_R = 2 };
/* One bin: 24 words = 192 B; every field merges by an associative, commutative integer operation, so the record of a domain
 * is the merge of the records of its parts, word for word, whatever the split, the launch shape, the alignment or the ghost
 * width. A sum is kept as three signed limbs: its value is (sum[k][0] + sum[k][1] 2^32 + sum[k][2] 2^64) 2^s_k. Every cell
 * adds limbs below 2^32, so NO LIMB CAN OVERFLOW WHILE FEWER THAN 2^31 CELLS ARE MERGED INTO ONE BIN (a 32768^2 grid has 2^30
 * cells); beyond that the words wrap silently. The order keys are key(x) = bits ^ (sign ? ~0 : 1 << 63) of the fp64 value:
 * their unsigned order is the numerical order, with -0.0 below +0.0. */
typedef struct {
    uint64_t n;             /* cells added                                              (sum) */
    uint64_t n_bad;         /* cells refused, see armon_hip_profile                     (sum) */
    int64_t  sum[5][3];     /* rho, rho*un, rho*ut, rho*E, p: three signed limbs each   (sum, limb by limb, no carry) */
    uint64_t rho_min, rho_max, p_min, p_max;   /* order keys                            (min / max) */
    uint64_t reserved[3];   /* zero */
} armon_profile_bin;
typedef struct {
    int32_t kind, eos;      /* ARMON_PROFILE_*; ARMON_EOS_* or -1 = no p (sum[4], p_min, p_max stay neutral) */
    int64_t nbins, width;   /* width: cells per bin, X and Y */
    double  cx, cy, dx, dy, inv_dr;   /* R: centre in cell units of the GLOBAL grid (cell gx covers [gx, gx+1)), cell sizes, 1/dr */
    double  gamma;
    int32_t scale_exp[5];   /* s_k: quantum of sum k is 2^s_k, -4096 <= s_k <= 4096 */
} armon_profile_spec;

/* Write the neutral element of the merge into bins_dev[0 .. nbins): zeros, the min keys all ones, the max keys zero. Async. */
ARMON_API int armon_hip_profile_reset(armon_ctx*, int64_t nbins, armon_profile_bin* bins_dev);

/* MERGE the real cells [col0, col0 + wnx) x [row0, row0 + wny) of one block into bins_dev[0 .. nbins). Block, window and
 * their checks are those of armon_hip_state_pack; (global_col0, global_row0) >= 0 is the global 0-based position of the
 * window's first cell. Also refused (ARMON_ERR_INVALID_ARG, nothing written): a NULL pointer, nbins < 1, width < 1, an unknown
 * kind or eos, a scale_exp outside [-4096, 4096], and for R a dx, dy or inv_dr that is not finite and > 0 or a centre that is
 * not finite. `spec` is HOST memory, read before the call returns.
 * Per cell at the global position (gx, gy), all arithmetic in fp64 whatever the data type (fp32 values are converted
 * first), one IEEE operation per operation written, correctly rounded division and square root:
 *   bin    X: b = gx / width.  Y: b = gy / width.  R: rx = ((double)gx + 0.5 - cx) dx, ry likewise,
 *          rr = sqrt(rx rx + ry ry), b = floor(rr inv_dr). A cell with b >= nbins is skipped and counted nowhere.
 *   un, ut X: u, v.  Y: v, u.  R: (u rx + v ry) / rr and (v rx - u ry) / rr, both 0 when rr == 0.
 *   terms  t0 = rho, t1 = rho un, t2 = rho ut, t3 = rho E, t4 = p: the EOS of this cell's (rho, E, u, v) evaluated IN THE DATA
 *          TYPE with the operations of the EOS kernels, then converted to fp64. No p vector is read.
 *   Q_k    = round-half-even(t_k / 2^s_k), an exact integer.
 *   bad    any of rho, u, v, E or a t_k not finite, or a |Q_k| >= 2^95: the cell adds 1 to n_bad and nothing else.
 *   limbs  with a = |Q_k|: a & 0xffffffff, (a >> 32) & 0xffffffff, a >> 64, each negated when Q_k < 0, each added to its own
 *          int64. rho and p enter rho_min .. p_max through their order keys.
 * No ghost cell is read. Integer atomics only (order-independent: the words are a function of the state, the spec and the
 * scale), no scratch, async on the context's stream with no host synchronisation. The tuning knob PROFILE_WGS
 * (armon_hip_set_tuning; 0 = automatic) caps the number of workgroups and changes no result bit. */
ARMON_API int armon_hip_profile(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        const double* rho, const double* u, const double* v, const double* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_profile_spec* spec, armon_profile_bin* bins_dev);
ARMON_API int armon_hip_profile_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        const float* rho, const float* u, const float* v, const float* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_profile_spec* spec, armon_profile_bin* bins_dev);

/* Same geometry, spec and checks (scale_exp is not used): bounds_dev[k] = max(bounds_dev[k], bit pattern of the largest FINITE
 * |t_k| of the window's cells), as unsigned integers; cells past the last bin count too. The default scale comes from this. */
ARMON_API int armon_hip_profile_bounds(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        const double* rho, const double* u, const double* v, const double* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_profile_spec* spec, uint64_t bounds_dev[5]);
ARMON_API int armon_hip_profile_bounds_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        const float* rho, const float* u, const float* v, const float* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_profile_spec* spec, uint64_t bounds_dev[5]);

/* ---- exact solutions: the state's distance from one, and the state filled with one (no reference counterpart;
 * csrc/analytic.hip) ---- */
enum { ARMON_EXACT_RIEMANN = 0, ARMON_EXACT_TABLE = 1 };
/* What the exact solution is. HOST memory, read before the call returns; only `table` points to device memory.
 * The coordinate of a point is q = x (coord = ARMON_PROFILE_X), y (Y) or the distance from the centre (R), with
 * x = (((double)gx + o) - cx) dx for the point at the fraction o of cell gx, y likewise: (cx, cy) is where the coordinate
 * is 0 (the jump of a Riemann problem, the centre of a blast), in cell units of the GLOBAL grid.
 * RIEMANN (perfect gas, gamma = 7/5 only: the fans use the integer powers 5 = 2/(gamma-1) and 7 = 2 gamma/(gamma-1)):
 *   xi = q / time, the region is the first of  xi < speed[0]: left state;  xi < speed[1]: left fan;  xi < speed[2]: left star
 *   state;  xi < speed[3]: right star state;  xi < speed[4]: right fan;  otherwise the right state. In a fan of side K, with
 *   sign = +1 (left) or -1 (right):  r = g1 + sign (g2[K] (u_K - xi)),  r2 = r r, r4 = r2 r2, r5 = r4 r, r7 = r5 r2,
 *   rho = rho_K r5,  p = p_K r7,  un = g1 (((sign c_K) + g3 u_K) + xi),  where the caller has set g1 = 2/(gamma+1),
 *   g2[K] = (gamma-1)/((gamma+1) c_K), g3 = (gamma-1)/2. A shock has speed[head] == speed[tail]: its fan is never chosen.
 * TABLE: lam = q inv_scale; not (lam < 1): the outer state; otherwise s = lam M, j = floor(s) clamped to [0, M - 1],
 *   f = s - j, value = t[j] + f (t[j+1] - t[j]) for each of the three rows rho, un, p of table[3][M + 1]. */
typedef struct {
    int32_t form, coord;        /* ARMON_EXACT_*; ARMON_PROFILE_X / Y / R */
    int32_t samples, eos;       /* 1, 2 or 4 points per cell and axis; ARMON_EOS_PERFECT_GAS */
    int64_t global_nx;          /* row length of the global grid: positions are g = gy * global_nx + gx */
    double  cx, cy, dx, dy, gamma;
    double  coord_min, coord_max;   /* a cell whose CENTRE coordinate lies outside [min, max) is skipped and counted nowhere */
    int32_t scale_exp[4][2];    /* per variable rho, un, ut, p: the quanta 2^s of (d, |d|) and of d^2; -4096 <= s <= 4096 */
    double  time;               /* RIEMANN, > 0 */
    double  side[2][4];         /* RIEMANN: rho, u, p, c of the left and of the right state */
    double  star[4];            /* RIEMANN: p*, u*, rho*L, rho*R */
    double  speed[5];           /* RIEMANN: left head, left tail, contact, right tail, right head, in order */
    double  g1, g2[2], g3;      /* RIEMANN: see above */
    double  inv_scale;          /* TABLE */
    int64_t M;                  /* TABLE: intervals, >= 1 */
    double  outer[3];           /* TABLE: rho, un, p where lam >= 1 */
    const double* table;        /* TABLE: DEVICE memory, [3][M + 1] fp64 */
} armon_exact_spec;
/* One variable's distance from the exact solution: 16 words = 128 B. Every field merges by integer addition or by the
 * pair maximum of armon_state_diff, so the record of a domain is the merge of the records of its parts, word for word.
 * Sums are three signed limbs as in armon_profile_bin: value = (s[0] + s[1] 2^32 + s[2] 2^64) 2^scale. */
typedef struct {
    uint64_t n;             /* cells added                                              (sum) */
    uint64_t n_bad;         /* cells refused                                            (sum) */
    int64_t  sum_d[3];      /* d = state - reference, quantum 2^scale_exp[k][0]         (sum, limb by limb) */
    int64_t  sum_abs[3];    /* |d|, quantum 2^scale_exp[k][0] */
    int64_t  sum_sq[3];     /* d d, quantum 2^scale_exp[k][1] */
    uint64_t max_abs;       /* bit pattern of the largest |d|                           (pair max) */
    uint64_t max_abs_at;    /* smallest g that attains it; UINT64_MAX while max_abs == 0 */
    uint64_t reserved[3];   /* zero */
} armon_exact_norm;

/* Write the neutral element of the merge into out_dev[0 .. 4): zeros, max_abs_at = UINT64_MAX. Async. */
ARMON_API int armon_hip_exact_norms_reset(armon_ctx*, armon_exact_norm* out_dev);

/* MERGE the distance of the real cells [col0, col0 + wnx) x [row0, row0 + wny) of one block from the exact solution `spec`
 * into out_dev[0 .. 4), one record for each of rho, un, ut, p. Block, window, (global_col0, global_row0) and their checks
 * are those of armon_hip_profile. Also refused (ARMON_ERR_INVALID_ARG, nothing written): a NULL pointer, an unknown form or
 * coord, samples not 1, 2 or 4, an eos other than the perfect gas, RIEMANN with gamma != 7/5 or time not finite and > 0,
 * TABLE with M < 1, a NULL table or an inv_scale not finite and > 0, dx, dy not finite and > 0, a centre or a coord_min /
 * coord_max that is NaN, global_nx < 1, a scale_exp outside [-4096, 4096].
 * Per cell at (gx, gy), all arithmetic in fp64 unless said otherwise, one IEEE operation per operation written, correctly
 * rounded division and square root:
 *   centre   rx = (((double)gx + 0.5) - cx) dx, ry likewise, rr = sqrt(rx rx + ry ry); q = rx, ry or rr; the cell is skipped
 *            unless coord_min <= q < coord_max.
 *   samples  o_i = ((double)i + 0.5) / samples. X and Y: the points o_i along the coordinate, i = 0 .. samples-1. R: the
 *            points (o_i, o_j), j outer. Each point's (rho, un, p) by the rule of armon_exact_spec, summed in that order
 *            from 0.0, the sum times 1 / (number of points).
 *   stored   the reference AS THE DATA TYPE HOLDS IT (exactly what armon_hip_exact_fill writes): u, v = (un, 0), (0, un)
 *            or (un rx / rr, un ry / rr) (both 0 where rr == 0), E = p / ((gamma - 1) rho) + 0.5 (u u + v v), then rho, u,
 *            v, E converted to the data type.
 *   vars     of the state's (rho, u, v, E) and of the stored reference's alike: rho; un, ut = u, v (X), v, u (Y) or
 *            (u rx + v ry) / rr, (v rx - u ry) / rr, both 0 where rr == 0 (R), of the values converted to fp64; p = the
 *            EOS evaluated IN THE DATA TYPE with the operations of the EOS kernels, then converted. No p vector is read.
 *   d_k      = the state's variable k - the reference's. So a state written by armon_hip_exact_fill has d_k == 0 in every
 *            cell, and the reference's transverse velocity is exactly 0 for X and Y.
 *   sums     Q = round-half-even(t / 2^s) of t = d_k, |d_k| (s = scale_exp[k][0]) and d_k d_k (s = scale_exp[k][1]), limbs
 *            as in armon_hip_profile; max_abs takes the bit pattern of |d_k| with g = gy * global_nx + gx.
 *   bad      any of the eight values, a variable of either side or a d_k d_k not finite, or a |Q| >= 2^95: the cell adds 1
 *            to n_bad of all four records and nothing else.
 * No ghost cell is read, no float atomics; writes out_dev and the context's reduction scratch (52 x 8 x CUs words at most),
 * which grows as in armon_hip_state_pack. Async on the context's stream. */
ARMON_API int armon_hip_exact_norms(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        const double* rho, const double* u, const double* v, const double* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_exact_spec* spec, armon_exact_norm* out_dev);
ARMON_API int armon_hip_exact_norms_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        const float* rho, const float* u, const float* v, const float* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_exact_spec* spec, armon_exact_norm* out_dev);

/* Same geometry, spec and checks (scale_exp is not used): write the stored reference into rho, u, v, E of the window's real
 * cells whose centre coordinate lies in [coord_min, coord_max). Ghosts and every other vector are untouched. Async. */
ARMON_API int armon_hip_exact_fill(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        double* rho, double* u, double* v, double* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_exact_spec* spec);
ARMON_API int armon_hip_exact_fill_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny,
        float* rho, float* u, float* v, float* E, int64_t col0, int64_t row0, int64_t wnx,
        int64_t wny, int64_t global_col0, int64_t global_row0, const armon_exact_spec* spec);

/* ---- run history: exact global sums, extrema with their cells and point gauges, sampled into a device-resident ring (no
 * reference counterpart; csrc/history.hip) ---- */
/* One sample of a window: 40 words = 320 B. Every field merges by integer addition or by a pair minimum / maximum, so the
 * record of a domain is the merge of the records of its parts, word for word, whatever the split, the launch shape, the
 * alignment or the ghost width. Sums are three signed limbs as in armon_profile_bin: value = (s[0] + s[1] 2^32 + s[2] 2^64)
 * 2^scale_exp[k]; no limb overflows while fewer than 2^31 cells are merged. An extremum is a pair (order key of the fp64 value
 * as in armon_profile_bin, g = gy * global_nx + gx of the cell): a minimum takes the smaller key, a maximum the larger, and
 * equal keys the smaller g, so the pair does not depend on the order the cells are visited in. While n == 0 the minima are
 * (UINT64_MAX, UINT64_MAX) and the maxima (0, UINT64_MAX): the neutral elements. */
enum { ARMON_HISTORY_RHO_MIN = 0, ARMON_HISTORY_RHO_MAX = 1, ARMON_HISTORY_P_MIN = 2, ARMON_HISTORY_P_MAX = 3,
       ARMON_HISTORY_E_MIN = 4, ARMON_HISTORY_E_MAX = 5, ARMON_HISTORY_Q2_MAX = 6, ARMON_HISTORY_MACH2_MAX = 7 };
typedef struct {
    uint64_t n;             /* cells added                                              (sum) */
    uint64_t n_bad;         /* cells refused, see armon_hip_history_sample              (sum) */
    int64_t  sum[6][3];     /* rho, rho u, rho v, rho E, (0.5 rho) q2, p: three signed limbs each   (sum, limb by limb, no carry) */
    uint64_t ext[8][2];     /* ARMON_HISTORY_*: (order key, g)                          (pair min / max) */
    uint64_t reserved[4];   /* zero */
} armon_history_record;
typedef struct {
    int32_t eos, reserved;  /* ARMON_EOS_* */
    double  gamma;          /* perfect gas */
    int64_t global_nx;      /* row length of the global grid: positions are g = gy * global_nx + gx */
    int32_t scale_exp[6];   /* s_k: quantum of sum k is 2^s_k, -4096 <= s_k <= 4096 */
} armon_history_spec;
#define ARMON_HISTORY_MAX_GAUGES 64
typedef struct armon_history armon_history;

/* A ring of `capacity` (1 .. 65536) slots on the context's device, each one armon_history_record followed by 5 x max_gauges
 * (0 .. ARMON_HISTORY_MAX_GAUGES) fp64 words, with the reduction scratch of the sample pass (36 words per workgroup, sized
 * here once: the pass never touches the context's own scratch, which may move and holds the dt partials of the fused sweep),
 * the gauge table and a pinned landing zone for armon_hip_history_read. Destroy it before the context. */
ARMON_API int armon_hip_history_create(armon_ctx*, int capacity, int max_gauges, armon_history** out);
ARMON_API int armon_hip_history_destroy(armon_ctx*, armon_history*);
/* The cells of the n <= max_gauges gauges as linear indices row * wnx + col INTO THE WINDOW later samples are given, -1 = not in
 * that window (the gauge's five words are then written as 0). Synchronises the stream; a sample refuses a cell outside its window. */
ARMON_API int armon_hip_history_set_gauges(armon_ctx*, armon_history*, const int64_t* cells, int n);

/* WRITE the sample of the real cells [col0, col0 + wnx) x [row0, row0 + wny) of one block into slot `slot` of the ring (what
 * the slot held is lost). Block, window, (global_col0, global_row0) and their checks are those of armon_hip_profile. Also
 * refused (ARMON_ERR_INVALID_ARG, nothing written): a NULL pointer, a handle of another context, a slot outside [0, capacity),
 * an unknown eos, a perfect gas whose gamma is not finite and > 1, global_nx < global_col0 + wnx, a scale_exp outside
 * [-4096, 4096], a gauge cell >= wnx wny. `spec` is HOST memory, read before the call returns.
 * Per cell at the global position (gx, gy), all arithmetic in fp64 whatever the data type (fp32 values are converted
 * first), one IEEE operation per operation written, correctly rounded division:
 *   q2     = u u + v v,  e = E - 0.5 q2
 *   p, c   the EOS of this cell's (rho, E, u, v) evaluated IN THE DATA TYPE with the operations of the EOS kernels, then
 *          converted to fp64. No p vector is read.
 *   terms  t0 = rho, t1 = rho u, t2 = rho v, t3 = rho E, t4 = (0.5 rho) q2, t5 = p
 *   Q_k    = round-half-even(t_k / 2^s_k), an exact integer; limbs as in armon_hip_profile.
 *   m      = 0 when q2 == 0, q2 / (c c) otherwise: the square of the Mach number (+inf where c c == 0).
 *   ext    rho, p and e enter a minimum and a maximum, q2 and m a maximum, each with g = gy * global_nx + gx.
 *   bad    any of rho, u, v, E, e, c or a t_k not finite, or a |Q_k| >= 2^95: the cell adds 1 to n_bad and nothing else.
 * Internal energy is not summed: with scale_exp[3] == scale_exp[4] it is sum[3] - sum[4], exactly.
 * Then the gauges: for each gauge with a cell, (double)rho, (double)u, (double)v, (double)E and (double)p of that cell, p by the
 * same EOS, as the five words of the gauge in the slot.
 * No ghost cell is read, no atomics; two launches on the context's stream, no host synchronisation: the slot holds the
 * sample once the stream has reached it (armon_hip_history_read waits for that). */
ARMON_API int armon_hip_history_sample(armon_ctx*, armon_history*, int slot, const armon_history_spec* spec, int64_t row_length,
        int nghost, int64_t nx, int64_t ny, const double* rho, const double* u, const double* v, const double* E, int64_t col0,
        int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0);
ARMON_API int armon_hip_history_sample_f32(armon_ctx*, armon_history*, int slot, const armon_history_spec* spec, int64_t row_length,
        int nghost, int64_t nx, int64_t ny, const float* rho, const float* u, const float* v, const float* E, int64_t col0,
        int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0, int64_t global_row0);

/* Slots [first_slot, first_slot + count) -> records_host[count] and gauges_host[count][max_gauges][5] (either may be NULL):
 * ONE device-to-host copy behind everything enqueued so far and ONE stream synchronisation. The library does not track which
 * slots were written since the last read: the caller does. */
ARMON_API int armon_hip_history_read(armon_ctx*, armon_history*, int first_slot, int count, armon_history_record* records_host,
        double* gauges_host);

/* ---- fp32 variants (ref data_type=Float32, src/parameters.jl:185): same kernels, float arrays and scalars ---- */
typedef struct {
    float *x, *y, *rho, *u, *v, *E, *p, *c, *g, *us, *ps, *work_1, *work_2, *work_3, *work_4, *mask;
} armon_block_data_f32;

ARMON_API int armon_hip_perfect_gas_EOS_f32(armon_ctx*, armon_range, float gamma,
        const float* rho, const float* E, const float* u, const float* v, float* p, float* c, float* g);
ARMON_API int armon_hip_bizarrium_EOS_f32(armon_ctx*, armon_range,
        const float* rho, const float* u, const float* v, const float* E, float* p, float* c, float* g);
ARMON_API int armon_hip_acoustic_f32(armon_ctx*, armon_range, int64_t s, float* us, float* ps,
        const float* rho, const float* ua, const float* p, const float* c);
ARMON_API int armon_hip_acoustic_GAD_f32(armon_ctx*, armon_range, int64_t s, float dt, float dx, float* us, float* ps,
        const float* rho, const float* ua, const float* p, const float* c, int limiter);
ARMON_API int armon_hip_cell_update_f32(armon_ctx*, armon_range, int64_t s, float dx, float dt,
        const float* us, const float* ps, float* rho, float* ua, float* E);
ARMON_API int armon_hip_advection_first_order_f32(armon_ctx*, armon_range, int64_t s, float dt,
        const float* us, const float* rho, const float* u, const float* v, const float* E,
        float* adv_rho, float* adv_urho, float* adv_vrho, float* adv_Erho);
ARMON_API int armon_hip_advection_second_order_f32(armon_ctx*, armon_range, int64_t s, float dx, float dt,
        const float* us, const float* rho, const float* u, const float* v, const float* E,
        float* adv_rho, float* adv_urho, float* adv_vrho, float* adv_Erho);
ARMON_API int armon_hip_euler_projection_f32(armon_ctx*, armon_range, int64_t s, float dx, float dt,
        const float* us, float* rho, float* u, float* v, float* E,
        const float* adv_rho, const float* adv_urho, const float* adv_vrho, const float* adv_Erho);
ARMON_API int armon_hip_boundary_conditions_f32(armon_ctx*, armon_range, int64_t incr, int nghost,
        float u_factor, float v_factor, float* rho, float* u, float* v, float* p, float* c, float* g, float* E);
ARMON_API int armon_hip_pack_to_array_f32(armon_ctx*, armon_range, int nghost, int64_t face,
        float* array, int nvars, const float* const* vars);
ARMON_API int armon_hip_unpack_from_array_f32(armon_ctx*, armon_range, int nghost, int64_t face,
        const float* array, int nvars, float* const* vars);
ARMON_API int armon_hip_dtCFL_async_f32(armon_ctx*, armon_range, float dx, float dy,
        const float* u, const float* v, const float* c, float* result_dev);
ARMON_API int armon_hip_dtCFL_f32(armon_ctx*, armon_range, float dx, float dy,
        const float* u, const float* v, const float* c, float* result_host);
ARMON_API int armon_hip_conservation_vars_f32(armon_ctx*, armon_range, float ds,
        const float* rho, const float* E, float out_host[2]);
ARMON_API int armon_hip_init_test_f32(armon_ctx*, armon_range, int test, int64_t row_length, int64_t col_length,
        int nghost, const int64_t global_pos[2], const int64_t global_N[2],
        const float origin[2], const float dX[2], float sedov_r, const armon_block_data_f32* data);
ARMON_API int armon_hip_coarsen_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
        const float* rho, const float* u, const float* v, const float* E, const float* p, float* out_dev);
ARMON_API int armon_hip_derive_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int64_t fx, int64_t fy,
        const float* rho, const float* u, const float* v, const float* E, const armon_derive_spec* spec, float* out_dev);
ARMON_API int armon_hip_gather_strided_f32(armon_ctx*, int64_t n_cells, int nvars, const float* const* vars,
        int64_t start, int64_t stride, int64_t count, float* out_dev);
ARMON_API int armon_hip_state_pack_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
        const float* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
        int64_t global_nx, float* dense_dev, uint64_t* digest_dev);
ARMON_API int armon_hip_state_unpack_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, int nvars,
        float* const* vars, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_first,
        int64_t global_nx, const float* dense_dev, uint64_t* digest_dev);
ARMON_API int armon_hip_plane_encode_f32(armon_ctx*, const float* dense_dev, int nplanes, int64_t rows, int64_t wnx,
        void* out_dev, uint64_t plane_capacity, uint64_t* sizes_dev);
ARMON_API int armon_hip_plane_decode_f32(armon_ctx*, const void* chunk_dev, uint64_t chunk_bytes, int64_t rows, int64_t wnx,
        int64_t col0, int64_t row0, int64_t snx, int64_t sny, float* out_dev, uint32_t* status_dev);

/* ---- fused sweep: EOS → BC (in-tile mirror) → fluxes → cell update → advection → projection ---- */
/* One call = one directional sweep of solver_cycle (ref src/solver.jl:300-316) over one block, reading
 * (ρ,u,v,E) from `in` and writing them to `out` (ping-pong; `in` and `out` must not alias).
 * Algorithmic traffic 64 B per real cell. Optionally materialises p (saved_vars, ref
 * src/blocking/blocks.jl:49) and the per-cell CFL minimum for the next cycle. */
struct armon_dt_state;       /* the time-step state on the device, defined below */
typedef struct {
    int32_t axis;            /* ARMON_AXIS_X / _Y                                               */
    int32_t scheme;          /* ARMON_SCHEME_*                                                  */
    int32_t limiter;         /* ARMON_LIMITER_*  (GAD only)                                     */
    int32_t projection;      /* ARMON_PROJECTION_*                                              */
    int32_t eos;             /* ARMON_EOS_*                                                     */
    int32_t nghost;          /* ghost layers of the arrays (>= scheme·projection stencil)       */
    int32_t bc_low, bc_high; /* 1: physical boundary on the low/high side of `axis` → mirror BC
                                applied in-tile; 0: ghosts already hold neighbour data (halo)   */
    int32_t exact;           /* 1: IEEE division/sqrt, no contraction: bit-identical to the staged kernels and to the
                                CPU restatement of the reference — every bit, subnormal results included
                                (-DARMON_LOOSE_SUBNORMAL at build time trades that last case for 5 %);
                                0: tuned (shared 1-ulp reciprocals + FMA, within the reference's golden tolerance) */
    int32_t x_kernel;        /* X-sweep kernel form: 0 = the one the library runs (lanes along x, DPP
                                shifts, 2 cells per lane). 3 (1 cell per lane) and 2 (LDS-transposed
                                march) are measured alternatives that exist only in the A/B build
                                libarmon_hip_alt.so (-DARMON_ALT_KERNELS); the product library refuses them */
    int64_t nx, ny;          /* real cells of the block                                         */
    double  dt, dx;          /* sweep time step (current_dt·factor) and cell size along axis    */
    double  gamma;           /* perfect gas only                                                */
    /* BC factors per side (read where bc_* = 1). Each must be +1 or -1, the values the reference's test cases have (ref
     * src/tests.jl:150-161), anything else is refused with ARMON_ERR_INVALID_ARG: the in-tile mirror evaluates the EOS of a
     * ghost cell from the scaled velocities, where boundary_conditions! copies p and c of the mirrored cell — the same bits
     * only while u² and v² are unchanged. (armon_hip_boundary_conditions of the staged path takes any factor.) */
    double  u_factor_low, v_factor_low, u_factor_high, v_factor_high;
    const double *rho_in, *u_in, *v_in, *E_in;
    /* What a sweep writes, and nothing else: of rho_out, u_out, v_out, E_out, p_out and c_out the real cells with
     * out_lo <= i < out_hi along the sweep axis (every real cell across it) — no ghost cell, no real cell outside the piece;
     * one element of dt_cfl_out. tests/test_gpu_sweep_random_state.py fills the arrays with a marker and checks it. */
    double *rho_out, *u_out, *v_out, *E_out;
    double *p_out;           /* nullable: EOS pressure of the PRE-sweep state (real cells)      */
    double *c_out;           /* nullable: EOS sound speed of the PRE-sweep state (real cells)   */
    /* Fused dt/CFL reduction of the NEXT cycle (ref src/reductions.jl:2-53, src/solver.jl:298): when
     * dt_cfl_out is non-NULL the sweep also reduces min(cfl_dx/max|u±c|, cfl_dy/max|v±c|) over the real
     * cells, with the post-sweep u, v and the pre-sweep c — exactly what dtCFL_kernel reads at the start
     * of the next cycle when this is the last sweep of a cycle — into *dt_cfl_out (one
     * device double, written by a follow-up fold kernel on the same stream). */
    double *dt_cfl_out;
    double  cfl_dx, cfl_dy;  /* GLOBAL cell sizes along x and y (ref src/reductions.jl:92)        */
    /* Partial sweeps, for overlapping the halo exchange with compute: produce only the cells
     * out_lo <= i < out_hi along the sweep axis (0-based real coordinates; out_hi == 0 means the whole
     * block). The interior [LAG, n-LAG) needs no ghost cell and can run while the halos travel; the two
     * LAG-wide boundary strips follow once the ghosts are in. dt_accumulate != 0: *dt_cfl_out =
     * min(*dt_cfl_out, this launch's value) instead of overwriting it. */
    int64_t out_lo, out_hi;
    int32_t dt_accumulate;
    int32_t reserved;
    /* Device-resident time step (armon_dt_state below), or NULL. When set, the sweep reads the cycle's time step from
     * device memory — its step is `dt` (then a FACTOR: 1, or 0.5 for Strang's half sweeps) x dt_state->current_dt —, does
     * nothing at all once dt_state->done is set, and writes p_out only when dt_state->emit_p is set: what lets a whole
     * cycle be captured once in a hipGraph and replayed without the host reading a scalar (armon_hip_graph_*). */
    struct armon_dt_state* dt_state;
} armon_sweep_desc;

ARMON_API int armon_hip_sweep(armon_ctx*, const armon_sweep_desc*);

/* ---- the dt state machine on the device + graph replay of a cycle -------------------------------------------------------- */
/* GlobalTimeStep (ref src/solver_state.jl:30-166) in device memory: update_dt! (:102-142: validity check, cfl scaling, the
 * 1.05 cap) and next_cycle! (:145-166) run as a one-thread kernel after the last sweep of a cycle, so that a cycle —
 * sweeps, dt reduction, state update, the time_loop's exit test (ref src/solver.jl:350) — has no host-read scalar and can
 * be replayed from a hipGraph. Values are stored as doubles; an fp32 run computes them in float (the _f32 step) exactly as
 * the reference's GlobalTimeStep{Float32} does. */
typedef struct armon_dt_state {
    double  current_dt;      /* time step of the cycle about to run / running                                        */
    double  time;            /* physical time at the start of that cycle                                            */
    double  L_prev;          /* CFL step of the state that cycle starts from (reduced by the previous cycle's last sweep) */
    int64_t cycle;
    int32_t done;            /* the time loop is over (time >= maxtime, cycle >= maxcycle, or an invalid step): sweeps and steps are no-ops */
    int32_t invalid;         /* a non-finite or non-positive step was seen (ref :123-124), at cycle `invalid_cycle`  */
    int32_t emit_p;          /* the cycle about to run is the last one: its last sweep materialises p               */
    int32_t pad;
    int64_t invalid_cycle;
    double  invalid_value;
    /* auto_step != 0: the fold of a sweep's fused dt reduction (dt_cfl_out with dt_state set, dt_accumulate == 0) performs
     * the state-machine step itself, with the constants below — one kernel less per replayed cycle than a separate
     * armon_hip_dt_state_step (a small grid's cycle time is its number of dependent launches). */
    int32_t auto_step, cst_dt;
    int64_t maxcycle;
    double  cfl, maxtime, Dt;
} armon_dt_state;

/* One state-machine step on the context's stream, after the last sweep of a cycle whose dt_cfl_out was `L_new_dev`:
 * next_cycle_dt = min(cfl x L_prev, 1.05 x current_dt) (or Dt with cst_dt), cycle += 1, time += current_dt,
 * current_dt = next_cycle_dt, L_prev = *L_new_dev, then done / emit_p for the next cycle from maxtime and maxcycle. */
ARMON_API int armon_hip_dt_state_step(armon_ctx*, armon_dt_state* state_dev, const double* L_new_dev, double cfl,
                                      double maxtime, int64_t maxcycle, int cst_dt, double Dt);
ARMON_API int armon_hip_dt_state_step_f32(armon_ctx*, armon_dt_state* state_dev, const float* L_new_dev, double cfl,
                                          double maxtime, int64_t maxcycle, int cst_dt, double Dt);

/* Stream capture of whatever the caller enqueues on the context's stream between _begin and _end (sweeps with dt_state,
 * the state step) into an executable graph; _launch replays it on that stream. Everything captured must already have run
 * once outside a capture (the library sizes its scratch on first use and cannot allocate while capturing).
 * The context must own its stream (armon_hip_init with stream = NULL): _begin refuses a caller-supplied or null stream.
 * Invalidation rule: the captured kernels hold the address of the context's reduction scratch, so while a graph of a
 * context is alive that scratch cannot grow — a launch on the same context that needs more of it (a larger block, a
 * first dtCFL) FAILS with ARMON_ERR_INVALID_ARG instead of moving it; run such launches before capturing, or destroy the
 * graph first. A graph should be destroyed before its context; the other order is safe (finalizers of a garbage-collected
 * host): armon_hip_destroy disowns the context's live graphs — their handles can then only be passed to
 * armon_hip_graph_destroy, armon_hip_graph_launch refuses them. */
typedef struct armon_graph armon_graph;
ARMON_API int armon_hip_graph_begin(armon_ctx*);
ARMON_API int armon_hip_graph_end(armon_ctx*, armon_graph** graph);
ARMON_API int armon_hip_graph_launch(armon_ctx*, armon_graph* graph);
ARMON_API int armon_hip_graph_destroy(armon_graph* graph);

/* Whole cycle in one launch (Sequential splitting: X sweep, then Y sweep — ref src/solver.jl:300-316 executed twice)
 * over one block: reads (rho,u,v,E) of x_desc->*_in ONCE and writes y_desc->*_out ONCE; the state between the two
 * sweeps stays in registers (32 B read + 32 B written per cell per CYCLE). x_desc gives the X sweep's dt, dx and
 * boundary; y_desc the Y sweep's, plus p_out (EOS pressure of the state before the Y sweep), dt_cfl_out and an
 * optional row range out_lo/out_hi. Results are the bits of armon_hip_sweep(x_desc) followed by armon_hip_sweep(y_desc).
 * fp64, GAD + minmod + euler_2nd, perfect gas, tuned arithmetic only; a block whose Y sides are remote cannot use it
 * (the rows received from a neighbour would have to be X-swept first). x_desc->x_kernel selects the form: 0 = one wave
 * runs both stages, 4 = producer / consumer waves through LDS. Both are measured alternatives (register-bound, slower
 * than the two launches today: DESIGN.md section 4.2), not what the solver runs: the kernels are compiled only into the
 * A/B build libarmon_hip_alt.so (-DARMON_ALT_KERNELS); in the product library this entry point returns
 * ARMON_ERR_INVALID_ARG. No reference counterpart. */
ARMON_API int armon_hip_cycle_xy(armon_ctx*, const armon_sweep_desc* x_desc, const armon_sweep_desc* y_desc);

/* The X sweep and the Y sweep of one Sequential cycle of a block, with the state BETWEEN them in a layout of the library's
 * own: rows of armon_hip_sweep_pair_pitch(nx, nghost) elements — nx + 2·nghost rounded up to a whole 128-B line — with the
 * ghost offsets kept, cell (x, y) at (y + nghost)·pitch + x + nghost. Every row the Y march reads then starts on a line and
 * it loads them non-temporally (tuned fp64 perfect gas; the other flavours run their ordinary kernels on the same layout).
 * Precondition: x_desc->*_out == y_desc->*_in — those four arrays, of `mid_bytes` bytes each, must hold
 * pitch·(ny + 2·nghost) elements; nothing but the two sweeps may rely on their content (the padding is never written). The
 * caller's own arrays, x_desc->*_in and y_desc->*_out, keep the pitch nx + 2·nghost. Both sweeps are whole (out_lo = out_hi
 * = 0), the Y sides are physical boundaries (bc_low, bc_high: a remote side's ghost rows would have to arrive in the
 * intermediate layout), the X sweep emits nothing of its own (p_out, c_out, dt_cfl_out NULL). Enqueues exactly what
 * armon_hip_sweep(x_desc) followed by armon_hip_sweep(y_desc) would — graph capture and dt_state included — and leaves the
 * same bits in y_desc->*_out, p_out, c_out and dt_cfl_out. fp64 only. No reference counterpart. */
ARMON_API int64_t armon_hip_sweep_pair_pitch(int64_t nx, int nghost);
ARMON_API int armon_hip_sweep_pair(armon_ctx*, const armon_sweep_desc* x_desc, const armon_sweep_desc* y_desc, size_t mid_bytes);

/* Placement of the 8 vectors a fused sweep streams (4 read + 4 written). On MI355X the same sweeps run 10-20 %
 * apart depending on where these vectors sit in HBM relative to each other (back-to-back allocations end up at a
 * regular physical spacing that makes the 8 streams collide on channels/banks), so a host
 * should allocate a few spare vectors once and let this call choose: `pool` holds n_pool >= 8 device vectors of
 * `bytes` bytes, pool[0..3] = the current (rho,u,v,E) WITH the state, pool[4..7] = their ping-pong partners, the
 * rest spares. `tries` role assignments (the first = pool[0..7] as given, the others random) are timed with the
 * caller's own descriptors as in a cycle — X reads roles 0..3 and writes 4..7, Y reads 4..7 and writes 0..3; all
 * other fields of x_desc / y_desc are used as they are (dt_cfl_out included), their 8 state pointers are ignored.
 * On return picks[role] = index in `pool` of the vector to use for that role, the state lives in pool[picks[0..3]],
 * every other vector of the pool is free for the caller to release; times_ms (nullable, [tries]) = the best
 * X+Y time of each assignment. Synchronous; needs 4 more vectors of `bytes` transiently. No reference counterpart.
 * fp64: when the descriptors satisfy armon_hip_sweep_pair's preconditions and `bytes` holds its intermediate, the draws are
 * timed with that call — the pitch and load policy such a host's cycles run — instead of two armon_hip_sweep calls (the
 * same holds for armon_hip_choose_placement). */
ARMON_API int armon_hip_tune_placement(armon_ctx*, const armon_sweep_desc* x_desc, const armon_sweep_desc* y_desc,
        void* const* pool, int n_pool, size_t bytes, int tries, int picks[8], double* times_ms);

/* The same choice for a pool that holds NO state yet — call it BEFORE init_test: nothing has to be parked or restored,
 * so the only transient memory is the caller's own spare vectors (n_pool - 8 of them). Candidates are timed on a uniform
 * state the call writes itself (every vector of the pool is overwritten); after 12 draws the search stops early once two
 * of them lie within `tolerance` (e.g. 0.01; 0 = never) of the best seen and a draw >= 7 % slower has been seen too,
 * after at most `tries`. picks[role] as above (roles 0..3:
 * where init_test should put rho,u,v,E; 4..7: their ping-pong partners); *tries_done (nullable) = draws timed. */
ARMON_API int armon_hip_choose_placement(armon_ctx*, const armon_sweep_desc* x_desc, const armon_sweep_desc* y_desc,
        void* const* pool, int n_pool, size_t bytes, int tries, double tolerance, int picks[8], double* times_ms,
        int* tries_done);

/* fp32 descriptor: field for field the fp64 one (see armon_sweep_desc for the meaning of each), with float arrays;
 * the scalars stay double and are rounded to float inside. */
typedef struct {
    int32_t axis, scheme, limiter, projection, eos, nghost;
    int32_t bc_low, bc_high;
    int32_t exact, x_kernel;
    int64_t nx, ny;
    double  dt, dx, gamma;
    double  u_factor_low, v_factor_low, u_factor_high, v_factor_high;
    const float *rho_in, *u_in, *v_in, *E_in;
    float *rho_out, *u_out, *v_out, *E_out;
    float *p_out, *c_out;
    float *dt_cfl_out;
    double  cfl_dx, cfl_dy;
    int64_t out_lo, out_hi;
    int32_t dt_accumulate, reserved;
    struct armon_dt_state* dt_state;
} armon_sweep_desc_f32;

ARMON_API int armon_hip_sweep_f32(armon_ctx*, const armon_sweep_desc_f32*);
ARMON_API int armon_hip_tune_placement_f32(armon_ctx*, const armon_sweep_desc_f32* x_desc, const armon_sweep_desc_f32* y_desc,
        void* const* pool, int n_pool, size_t bytes, int tries, int picks[8], double* times_ms);
ARMON_API int armon_hip_choose_placement_f32(armon_ctx*, const armon_sweep_desc_f32* x_desc, const armon_sweep_desc_f32* y_desc,
        void* const* pool, int n_pool, size_t bytes, int tries, double tolerance, int picks[8], double* times_ms,
        int* tries_done);

/* ---- passive scalars: advected fields carried through a fused sweep --------------------------------- */
/* No reference counterpart. The rule:
 * - Up to ARMON_MAX_SCALARS = 4 planes φ_k, in the layout of the state vectors: flat, ghosted, plain pitch nx + 2·nghost.
 * - For every directional sweep of the state, the scalar sweep uses the same axis, dt, dx, scheme, limiter, projection, EOS,
 *   `exact` flag and bc_low / bc_high. It computes, from the pre-sweep state and the pre-sweep φ_k, exactly what that sweep
 *   computes for its transverse velocity, with φ_k in place of `ut` everywhere except the EOS:
 *   - Lagrangian phase: φ unchanged.
 *   - q = ρ_lag·φ.
 *   - Limited slope, first or second order.
 *   - Advection flux from the upwind donor.
 *   - φ' = T_q / T_ρ.
 * - Use the same IEEE operations in the same order as the flavour in use:
 *   - Exact: the formulas of Pipe / run_exact.
 *   - Tuned: the fast:: stage functions.
 * - On a side with bc = 1, the ghost φ is the mirrored real cell with factor +1, whatever the velocity factors. This is the
 *   transverse factor of every case and every boundary type here.
 * - With bc = 0 the ghosts of φ are read as they are.
 * - The scalar sweep writes the real cells of phi_out[k] and nothing else. It leaves alone:
 *   - ghost cells and pitch padding;
 *   - phi_in;
 *   - all eight state arrays of the descriptor.
 *
 * armon_hip_sweep_scalars: one launch for all `ns` planes, on the context's stream. The fused sweeps are out of place, so the
 * call follows armon_hip_sweep with that sweep's own descriptor, before the caller swaps its ping-pong arrays. Read from the
 * descriptor: the pre-sweep state rho_in, u_in, v_in, E_in and the scalars (axis .. gamma, the mirror flags and factors);
 * ignored: rho_out .. E_out, p_out, c_out, dt_cfl_out and what goes with it. phi_in / phi_out: HOST arrays of `ns` device
 * pointers, copied into the launch. Traffic: (32 + 16·ns) B per fp64 cell. Refused before any launch (ARMON_ERR_INVALID_ARG,
 * armon_hip_last_error names the argument): ns outside 1..ARMON_MAX_SCALARS; a NULL plane; a phi_out[k] that is a phi_in, another
 * phi_out or a state array of the descriptor; dt_state != NULL (host-driven only); a partial piece (out_lo / out_hi not the
 * whole block); x_kernel != 0; and everything armon_hip_sweep refuses (tags, empty or oversized blocks, nghost below the
 * stencil's reach, mirror factors other than +1 / -1, a NULL rho_in .. E_in). */
#define ARMON_MAX_SCALARS 4
/* The initial plane of a region-built scalar: armon_hip_init_regions (same arguments, same device code, same rule) with the
 * scalar's values where the regions' densities stand — rho of `background` and of every region; their u, v, E are not used —
 * and `phi` where rho stands: bit for bit the rho plane of that call (the last region that holds a point wins; a cut cell
 * takes the mean of its samples). Values are any finite numbers, zero and negative ones included. scratch_1..3: three
 * planes of the same size whose content is lost. */
ARMON_API int armon_hip_init_scalar_regions(armon_ctx*, armon_range, int64_t row_length, int nghost, const int64_t global_pos[2],
        const double origin[2], const double dX[2], int samples, const double background[4], int nregions,
        const armon_region* regions, double* phi, double* scratch_1, double* scratch_2, double* scratch_3);
ARMON_API int armon_hip_init_scalar_regions_f32(armon_ctx*, armon_range, int64_t row_length, int nghost, const int64_t global_pos[2],
        const float origin[2], const float dX[2], int samples, const float background[4], int nregions,
        const armon_region_f32* regions, float* phi, float* scratch_1, float* scratch_2, float* scratch_3);
ARMON_API int armon_hip_sweep_scalars(armon_ctx*, const armon_sweep_desc*, int ns, const double* const* phi_in,
                                      double* const* phi_out);
ARMON_API int armon_hip_sweep_scalars_f32(armon_ctx*, const armon_sweep_desc_f32*, int ns, const float* const* phi_in,
                                          float* const* phi_out);
/* Bound-preserving transport of the planes: the arguments, the descriptor checks, the refusals, the
 * launch geometry, the mirrors and what is written are those of armon_hip_sweep_scalars; only the planes' rule differs. φ is
 * transported per unit mass, with the mass fluxes the state's own remap of ρ computes. Along the sweep axis, per plane:
 * - Lagrangian mass of cell c: m_c = Δx_lag,c · ρ_lag,c.
 * - Slope: σ_c = minmod(φ_c − φ_c−1, φ_c+1 − φ_c), not weighted by lengths or masses; projection `euler`: σ = 0.
 * - Interface on the low side of cell i, mass flux a_i (the advection flux of ρ), donor d = i−1 if it moves up (dt·u* > 0),
 *   else d = i: ν = |a_i| / m_d, φ*_i = φ_d ± σ_d · ½(1 − ν) (+ when it moves up), A_i = a_i · φ*_i.
 * - t_q = (m_i φ_i − (A_i+1 − A_i)) / dx, φ'_i = t_q / ρ'_i with ρ' the sweep's own new density.
 * - φ'_i = min(max(φ'_i, lo_i), hi_i), lo_i / hi_i the smallest / largest of φ_i−1, φ_i, φ_i+1 as the sweep read them (mirrored
 *   or wrapped ghosts included); taken by comparisons, so a NaN stays a NaN.
 * Exact flavour: one IEEE operation per operation written, in this order (tests/bounded_restated.py restates it in numpy).
 * Tuned flavour: the fast:: stages `inv_mass`, `leaving_weight`, `carry1` / `carry2`, `settle` (csrc/sweep_stages.hpp).
 * Before the clamp φ' is, in real arithmetic, a convex combination of values of the limited profiles of cells i−1, i, i+1
 * whenever the two outflows of a cell do not exceed its mass; the clamp removes rounding and makes the bound unconditional:
 * no plane leaves the range of its own values along any line of the sweep axis, ghosts included. */
ARMON_API int armon_hip_sweep_scalars_bounded(armon_ctx*, const armon_sweep_desc*, int ns, const double* const* phi_in,
                                              double* const* phi_out);
ARMON_API int armon_hip_sweep_scalars_bounded_f32(armon_ctx*, const armon_sweep_desc_f32*, int ns, const float* const* phi_in,
                                                  float* const* phi_out);

/* ---- physical diffusion: viscosity, heat conduction and scalar diffusivity (csrc/diffuse.hip) -------- */
/* No reference counterpart: the reference solves the inviscid equations. Operator-split, one or more steps per cycle. The rule:
 *
 * Coefficients. All are constants, >= 0 and finite:
 * - nu: kinematic shear viscosity. The bulk viscosity is 0.
 * - chi: diffusivity of the specific internal energy e = E − ½(u² + v²). For the perfect gas this is Fourier conduction with
 *   k = ρ·chi·c_v. It is defined the same way for Bizarrium. No EOS is evaluated.
 * - D_k: one per diffusing scalar plane.
 *
 * Shape of the step. One step of length dt reads ρ, u, v, E and the diffusing planes φ_k. It writes u', v', E', φ_k' of the REAL
 * cells into other arrays. It is out of place. ρ does not change. It reads no ghost cell. It writes no ghost cell or padding.
 *
 * Arithmetic.
 * - T is the run's data type.
 * - One IEEE operation per operation written. No contraction. The only division is dt / ρ.
 * - The host passes idx = T(1)/dx and idy = T(1)/dy.
 * - The kernel forms q4x = T(0.25)·idx, q4y = T(0.25)·idy, c43 = T(4)/T(3) and c23 = T(2)/T(3).
 *
 * Cells outside the domain. A neighbour index outside [0, n) along an axis maps as follows:
 * - On a Periodic axis: the wrapped index.
 * - Otherwise: the mirrored one, −1−i or 2n−1−i, with u and v multiplied by that side's u_factor and v_factor. These are the
 *   sweep's own factors, ±1. ρ, e and φ take factor +1.
 * - Both axes map independently. Factors multiply in a corner.
 * A wall is therefore free-slip, adiabatic and impermeable to φ. Its face carries zero tangential stress, zero work and zero heat
 * and scalar flux.
 *
 * Flux of the x-face. Take the face between cells L = (i, j) and R = (i+1, j):
 * - rf = T(0.5)·(ρ_L + ρ_R)
 * - mu = nu·rf
 * - ux = (u_R − u_L)·idx
 * - vx = (v_R − v_L)·idx
 * - uy = ((u[i,j+1] − u[i,j−1]) + (u[i+1,j+1] − u[i+1,j−1]))·q4y
 * - vy likewise from v
 * - txx = mu·(c43·ux − c23·vy)
 * - txy = mu·(uy + vx)
 * - uf = T(0.5)·(u_L + u_R)
 * - vf likewise
 * - q = (chi·rf)·((e_R − e_L)·idx)
 * - F_u = txx
 * - F_v = txy
 * - F_E = (uf·txx + vf·txy) + q
 * - F_φk = (D_k·rf)·((φ_R − φ_L)·idx)
 *
 * Flux of the y-face. This is the transpose:
 * - normal differences with idy;
 * - the transverse ones ((a[i+1,j] − a[i−1,j]) + (a[i+1,j+1] − a[i−1,j+1]))·q4x;
 * - tyy = mu·(c43·vy − c23·ux);
 * - G_u = txy, G_v = tyy, G_E = (uf·txy + vf·tyy) + q.
 *
 * Update. With k = dt/ρ:
 *   a' = a + k·((F_a(i+½) − F_a(i−½))·idx + (G_a(j+½) − G_a(j−½))·idy)
 * for a = u, v, E, φ_k.
 *
 * Consequences to preserve.
 * - A face's flux is ONE value whichever of its two cells evaluates it: "right minus left", with commutative sums only.
 * - So Σρu, Σρv, ΣρE and Σρφ telescope.
 * - A uniform state is a fixed point bit for bit.
 *
 * armon_hip_diffuse: ONE launch on the context's stream for the state and the `ns` diffusing planes, in the layout of the state
 * vectors (flat, ghosted, plain pitch nx + 2·nghost). periodic / u_factor / v_factor are indexed by ARMON_SIDE_*; the factors of
 * a periodic side are not used. With nu = chi = 0 the planes alone are read and written (ρ is read; u, v, E and their outputs
 * are not looked at and may be NULL); with ns = 0 the state alone. With rho_out given the real cells of ρ are copied too, so
 * that the caller swaps the whole set of four: 64 B per fp64 cell for the state, 16 B more per plane. All of nu, chi and
 * D[0..ns) zero: ARMON_OK, nothing launched, no pointer looked at. Refused before any launch (ARMON_ERR_INVALID_ARG, nothing
 * written; armon_hip_last_error names the argument): a NULL ctx or descriptor; a NULL array that the step reads or writes; an
 * output that is an input or another output (the same pointer: arrays that overlap in part are not detected and are the
 * caller's to avoid); a negative or non-finite nu, chi, D[k] or dt; dx or dy not finite and positive;
 * a factor of a non-periodic side other than +1 / -1; ns outside 0..ARMON_MAX_SCALARS; nx or ny < 1, nghost < 0, or a block
 * whose runs of rows outgrow a launch grid; a periodic flag on one side of an axis only. */
typedef struct armon_diffuse_desc {
    int64_t nx, ny;
    int32_t nghost, ns;
    int32_t periodic[4];
    double  u_factor[4], v_factor[4];
    double  dt, dx, dy, nu, chi, D[ARMON_MAX_SCALARS];
    const double *rho, *u, *v, *E;
    double *rho_out, *u_out, *v_out, *E_out;
    const double* phi[ARMON_MAX_SCALARS];
    double* phi_out[ARMON_MAX_SCALARS];
} armon_diffuse_desc;
/* fp32: field for field the same, with float arrays; the scalars stay double and are rounded to float inside. */
typedef struct armon_diffuse_desc_f32 {
    int64_t nx, ny;
    int32_t nghost, ns;
    int32_t periodic[4];
    double  u_factor[4], v_factor[4];
    double  dt, dx, dy, nu, chi, D[ARMON_MAX_SCALARS];
    const float *rho, *u, *v, *E;
    float *rho_out, *u_out, *v_out, *E_out;
    const float* phi[ARMON_MAX_SCALARS];
    float* phi_out[ARMON_MAX_SCALARS];
} armon_diffuse_desc_f32;
ARMON_API int armon_hip_diffuse(armon_ctx*, const armon_diffuse_desc*);
ARMON_API int armon_hip_diffuse_f32(armon_ctx*, const armon_diffuse_desc_f32*);

/* ---- mixing measures: exact binned sums and histograms of the passive scalars (csrc/mixing.hip) ------ */
/* No reference counterpart. Two passes over rho and the scalar planes, built like armon_hip_profile: every addend is rounded
 * once to a fixed-point integer, everything after that is integer addition, an unsigned minimum or an unsigned maximum, so
 * every record below is the merge of the records of the parts of its window, WORD FOR WORD, whatever the split, the launch
 * shape, the alignment path or the ghost width.
 *
 * One (plane, bin) of armon_hip_mixing: 20 words = 160 B. A sum is three signed limbs as in armon_profile_bin: its value is
 * (sum[j][0] + sum[j][1] 2^32 + sum[j][2] 2^64) 2^s_kj. NO LIMB CAN OVERFLOW WHILE FEWER THAN 2^31 CELLS ARE MERGED INTO ONE
 * BIN. phi_min / phi_max are order keys as in armon_profile_bin. */
typedef struct {
    uint64_t n;             /* cells added                                              (sum) */
    uint64_t n_bad;         /* cells refused for this plane                             (sum) */
    int64_t  sum[5][3];     /* rho, phi, phi*phi, rho*phi, rho*phi*phi: three limbs each (sum, limb by limb, no carry) */
    uint64_t phi_min, phi_max;   /* order keys                                          (min / max) */
    uint64_t reserved;      /* zero */
} armon_mixing_bin;
typedef struct {
    int32_t axis, reserved;     /* ARMON_PROFILE_X or ARMON_PROFILE_Y; reserved = 0 */
    int64_t nbins, width;       /* width: cells per bin */
    int32_t scale_exp[ARMON_MAX_SCALARS][5];   /* s_kj: quantum of sum j of plane k is 2^s_kj, -4096 <= s_kj <= 4096 */
} armon_mixing_spec;

/* Write the neutral element of the merge into bins_dev[0 .. ns * nbins): zeros, phi_min all ones, phi_max zero. Async. */
ARMON_API int armon_hip_mixing_reset(armon_ctx*, int ns, int64_t nbins, armon_mixing_bin* bins_dev);

/* MERGE the real cells [col0, col0 + wnx) x [row0, row0 + wny) of one block into bins_dev[plane][bin], plane < ns, bin < nbins.
 * Block, window, (global_col0, global_row0) and their checks are those of armon_hip_profile. phi: a HOST array of `ns` device
 * pointers, planes in the layout of the state vectors. Also refused (ARMON_ERR_INVALID_ARG, nothing written): a NULL pointer,
 * ns outside 1..ARMON_MAX_SCALARS, a NULL plane, nbins < 1, width < 1, an axis other than X or Y, a scale_exp of a plane < ns
 * outside [-4096, 4096]. `spec` and `phi` are HOST memory, read before the call returns.
 * Per cell at the global position (gx, gy) and per plane k, all arithmetic in fp64 whatever the data type (fp32 values are
 * converted first), one IEEE operation per operation written:
 *   bin    X: b = gx / width.  Y: b = gy / width.  A cell with b >= nbins is skipped and counted nowhere.
 *   terms  t0 = rho, t1 = phi, t2 = phi * phi, t3 = rho * phi, t4 = t3 * phi.
 *   Q_j    = round-half-even(t_j / 2^s_kj), an exact integer.
 *   bad    rho, phi_k or a t_j not finite, or a |Q_j| >= 2^95: the cell adds 1 to n_bad OF PLANE k and nothing else; the
 *          other planes are not affected.
 *   limbs  with a = |Q_j|: a & 0xffffffff, (a >> 32) & 0xffffffff, a >> 64, each negated when Q_j < 0, each added to its own
 *          int64. phi enters phi_min and phi_max through its order key.
 * No ghost cell is read. Integer atomics only (order-independent: the words are a function of rho, the planes, the spec and
 * the scale), no scratch, async on the context's stream with no host synchronisation. One launch per plane: the words of a
 * call with ns planes are those of ns calls with one plane each. The tuning knob PROFILE_WGS caps the workgroups of these
 * kernels and of armon_hip_scalar_pdf as it does armon_hip_profile's, and changes no result bit. */
ARMON_API int armon_hip_mixing(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho, int ns,
        const double* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
        int64_t global_row0, const armon_mixing_spec* spec, armon_mixing_bin* bins_dev);
ARMON_API int armon_hip_mixing_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho, int ns,
        const float* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
        int64_t global_row0, const armon_mixing_spec* spec, armon_mixing_bin* bins_dev);

/* Same geometry, spec and checks (scale_exp is not used): bounds_dev[k * 5 + j] = max(bounds_dev[k * 5 + j], bit pattern of the
 * largest FINITE |t_j| of plane k over the window's cells), as unsigned integers; cells past the last bin count too. */
ARMON_API int armon_hip_mixing_bounds(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho,
        int ns, const double* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
        int64_t global_row0, const armon_mixing_spec* spec, uint64_t* bounds_dev);
ARMON_API int armon_hip_mixing_bounds_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho,
        int ns, const float* const* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, int64_t global_col0,
        int64_t global_row0, const armon_mixing_spec* spec, uint64_t* bounds_dev);

/* The histogram of one plane: (nbins + 2) rows of 4 words — the cell count (uint64) and the exact sum of rho as three signed
 * limbs of quantum 2^rho_scale_exp — followed by ONE word, the count of bad cells: 4 (nbins + 2) + 1 words in all. Rows
 * 0 .. nbins - 1 are the bins, row nbins is "below", row nbins + 1 is "above". Every word merges by integer addition; the
 * neutral element is all zeros. */
typedef struct {
    double  lo, inv_w;          /* the lower edge of bin 0 and 1 / (bin width): both finite, inv_w > 0 */
    int32_t nbins;              /* 1 .. ARMON_PDF_MAX_BINS */
    int32_t rho_scale_exp;      /* -4096 .. 4096 */
} armon_pdf_spec;
#define ARMON_PDF_MAX_BINS 1024

/* Zero the 4 (nbins + 2) + 1 words of out_dev. Async. */
ARMON_API int armon_hip_scalar_pdf_reset(armon_ctx*, int nbins, uint64_t* out_dev);

/* MERGE the real cells of the window into out_dev. Geometry and its checks as armon_hip_mixing (the global position is not
 * part of the rule: no argument for it). Also refused (ARMON_ERR_INVALID_ARG, nothing written): a NULL pointer, nbins outside
 * 1..ARMON_PDF_MAX_BINS, a lo or inv_w that is not finite, inv_w <= 0, rho_scale_exp outside [-4096, 4096].
 * Per cell, in fp64 (fp32 values converted first), one IEEE operation per operation written:
 *   bad    rho or phi not finite, or |Q(rho)| >= 2^95 with Q = round-half-even(rho / 2^rho_scale_exp): the cell adds 1 to the
 *          bad word and nothing else.
 *   row    else if phi < lo: "below". Else fb = floor((phi - lo) * inv_w); if !(fb < nbins): "above"; else bin (int64)fb.
 *   adds   1 to the row's count, the limbs of Q(rho) (cut as in armon_hip_profile) to the row's three limb sums.
 * Integer atomics only, no scratch, async on the context's stream with no host synchronisation. */
ARMON_API int armon_hip_scalar_pdf(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, const double* rho,
        const double* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, const armon_pdf_spec* spec, uint64_t* out_dev);
ARMON_API int armon_hip_scalar_pdf_f32(armon_ctx*, int64_t row_length, int nghost, int64_t nx, int64_t ny, const float* rho,
        const float* phi, int64_t col0, int64_t row0, int64_t wnx, int64_t wny, const armon_pdf_spec* spec, uint64_t* out_dev);


/* ---- multi-GPU: tile-decomposed grid, halo exchange and dt reduction on the device ------------------------------ */
/* Replaces the reference's MPI path: start_exchange / finish_exchange (ref src/halo_exchange.jl:229-283), the side
 * selection of block_ghost_exchange (ref :323-354: the two sides ALONG the sweep axis, all ghost layers, no corners),
 * the MPI_Iallreduce(MIN) of the time step (ref src/solver_state.jl:89-111, src/utils.jl:126-143) and the cartesian
 * topology of init_MPI (ref src/parameters.jl:441-447: rank r at coords (r / py, r % py), non-periodic).
 *
 * A group is a px x py grid of tiles. Each local tile owns an armon_ctx (its compute stream: enqueue that tile's
 * kernels there) and a transfer stream. An exchange is pack -> (event) -> transfer -> (event) -> unpack, ordered on
 * the device only: NO host synchronisation between pack and unpack, so whatever the caller enqueues on a tile's
 * compute stream between _start and _finish (the interior of a fused sweep) overlaps with the transfers.
 *  - armon_hip_mgpu_init      : every tile lives in this process, tile r on device device_ids[r] (devices may repeat;
 *                               NULL = all on device 0). Faces travel as peer-to-peer copies (xGMI between GPUs).
 *  - armon_hip_mgpu_init_rank : one process per GPU; this process owns tile `rank` only. Faces travel as RCCL
 *                               send/recv pairs, the dt minimum as an RCCL all-reduce. `id` = ARMON_MGPU_ID_BYTES bytes
 *                               from armon_hip_mgpu_unique_id on rank 0, broadcast by the host's own launcher
 *                               (MPI_Bcast in Armon.jl, the torch.distributed store in bench.py). Collective.
 *                               `stream`: compute stream to adopt, or NULL. */
typedef struct armon_mgpu armon_mgpu;
#define ARMON_MGPU_ID_BYTES 256

ARMON_API int armon_hip_mgpu_init(int px, int py, const int* device_ids, armon_mgpu** group);
ARMON_API int armon_hip_mgpu_unique_id(void* id);
ARMON_API int armon_hip_mgpu_init_rank(int px, int py, int rank, int device_id, void* stream, const void* id,
                                       armon_mgpu** group);
/* armon_hip_mgpu_init_rank in two steps, for hosts that want to agree on readiness in between (bench.py does, over its
 * launcher's group): _prepare_rank is everything LOCAL to the process (RCCL symbols, context, streams, scratch) and may
 * fail on one rank alone; _connect is the collective ncclCommInitRank of the two communicators — every rank enters it, or
 * none (a rank that skipped it after a local failure would leave the others blocked in it). */
ARMON_API int armon_hip_mgpu_prepare_rank(int px, int py, int rank, int device_id, void* stream, armon_mgpu** group);
ARMON_API int armon_hip_mgpu_connect(armon_mgpu* group, const void* id);
ARMON_API int armon_hip_mgpu_destroy(armon_mgpu* group);
/* Periodic domains (no reference counterpart: the reference's process grid is never periodic, ref
 * src/parameters.jl:432). _set_periodic: the domain is periodic along that axis — out-of-grid neighbours wrap around, so the
 * tiles of a group or the ranks exchange across the domain's edge, and a 1 x 1 rank group is its own neighbour on every
 * side: ONE GPU executes the real ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd of armon_hip_halo_exchange_start
 * (call it before the first exchange; the caller's sweeps must then treat those sides as remote: bc_low = bc_high = 0).
 * A block that belongs to no group fills the same ghosts with armon_hip_periodic_ghosts.
 * _force_peer_copy, an aid for testing the transport: an in-process group moves its faces (and the dt scalars) with
 * hipMemcpyPeerAsync even when both tiles sit on the same device. */
ARMON_API int armon_hip_mgpu_set_periodic(armon_mgpu* group, int periodic_x, int periodic_y);
ARMON_API int armon_hip_mgpu_force_peer_copy(armon_mgpu* group, int on);
/* Test aid: from now on, with probability 1/2 each, the group's stream operations (packs, transfers, unpacks, the edge
 * join, the dt reduction) are preceded by a busy-wait kernel of up to max_delay_us on their stream — timings a single
 * GPU never produces by itself; results must not change. 0 switches it off. seed 0 = default sequence. */
ARMON_API int armon_hip_mgpu_set_chaos(armon_mgpu* group, unsigned max_delay_us, uint64_t seed);
ARMON_API int armon_hip_mgpu_n_local(armon_mgpu* group);                       /* tiles owned by this process */
ARMON_API armon_ctx* armon_hip_mgpu_ctx(armon_mgpu* group, int local_tile);    /* that tile's context (owned by the group) */
/* rank, cartesian coords and the neighbour rank per ARMON_SIDE_* (-1 = physical boundary, MPI.PROC_NULL) */
ARMON_API int armon_hip_mgpu_tile_info(armon_mgpu* group, int local_tile, int* rank, int coords[2], int neighbours[4]);

/* What one local tile exchanges: fused path (rho,u,v,E); staged path comm_vars (rho,u,v,E,p,c,g), ref
 * src/blocking/blocks.jl:50. The wire format is pack_to_array!'s (ref src/halo_exchange.jl:187-216). */
typedef struct {
    int64_t nx, ny;          /* real cells of the tile                              */
    int32_t nghost, nvars;   /* ghost layers; number of vectors (1..8)              */
    void*   vars[8];         /* device vectors of (nx+2g)*(ny+2g) elements          */
} armon_halo_desc;

/* `tiles` = one descriptor per LOCAL tile, in local tile order. _start packs and posts the transfers of the two
 * sides along `axis` of every local tile that has a neighbour there; _finish makes each compute stream wait for its
 * receives and unpacks them into the ghost cells; armon_hip_halo_exchange = _start + _finish. Physical sides are
 * left alone (mirror boundary condition: armon_hip_boundary_conditions, or bc_low/bc_high of the fused sweep). */
ARMON_API int armon_hip_halo_exchange_start(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_halo_exchange_finish(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_halo_exchange(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_halo_exchange_start_f32(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_halo_exchange_finish_f32(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_halo_exchange_f32(armon_mgpu*, int axis, const armon_halo_desc* tiles);

/* Edge stream. What follows the receive of a sweep's faces — the unpack and the LAG-wide strips next to the remote
 * sides — reads the same input state as the interior sweep and writes cells the interior does not, so it can run on the
 * tile's TRANSFER stream while the interior runs on the compute stream, instead of in a chain of small launches after
 * it (the interior reads no ghost cell and never writes the strips' cells):
 *     armon_hip_halo_exchange_start -> armon_hip_sweep(ctx, interior) -> armon_hip_halo_exchange_finish_edge
 *     -> armon_hip_sweep(edge_ctx, strip) per remote side, dt_cfl_out = edge_dt + side index, dt_accumulate = 0
 *     -> armon_hip_mgpu_edge_join(group, dt_dev or NULL)
 * _edge_ctx: the tile's context on its transfer stream (owned by the group). _edge_dt: 2 device scalars of the run's
 * precision for the strips' CFL steps. _edge_join: every compute stream waits for its tile's edge work; with dt_dev,
 * dt_dev[k] = min(dt_dev[k], the tile's two edge scalars) on the compute stream, and the edge scalars are reset.
 * Replaces the interconnect-free part of ref src/halo_exchange.jl:256-283 (finish_exchange + the boundary blocks). */
ARMON_API armon_ctx* armon_hip_mgpu_edge_ctx(armon_mgpu* group, int local_tile);
ARMON_API void* armon_hip_mgpu_edge_dt(armon_mgpu* group, int local_tile);
ARMON_API int armon_hip_halo_exchange_finish_edge(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_halo_exchange_finish_edge_f32(armon_mgpu*, int axis, const armon_halo_desc* tiles);
ARMON_API int armon_hip_mgpu_edge_join(armon_mgpu*, double* const* dt_dev);
ARMON_API int armon_hip_mgpu_edge_join_f32(armon_mgpu*, float* const* dt_dev);

/* Global minimum of one device scalar per local tile (dt_cfl_out of the fused sweep / armon_hip_dtCFL_async), in
 * place, ordered on the compute streams: afterwards every dt_dev[k] holds the minimum over ALL tiles of the group.
 * The reference consumes it one cycle later (ref src/solver_state.jl:145-166): nothing is waited for on the host. */
ARMON_API int armon_hip_dt_allreduce(armon_mgpu*, double* const* dt_dev);
ARMON_API int armon_hip_dt_allreduce_f32(armon_mgpu*, float* const* dt_dev);

/* A whole solver cycle of every LOCAL tile in one call — solver_cycle (ref src/solver.jl:288-320) on the fused path:
 * for each sweep of the cycle (ref split_axes, src/axis_splitting.jl:24-46) the halo exchange along its axis (ref
 * block_ghost_exchange, src/halo_exchange.jl:323-354), the interior of the sweep while the faces travel, the unpack and the
 * LAG-wide strips on the transfer stream, the join; after the last sweep the global minimum of the next CFL step (ref
 * src/solver_state.jl:89-111) — the calls above in the order the edge-stream protocol prescribes, enqueued natively. A
 * group of several local tiles is driven by ONE HOST THREAD PER TILE (created by the first cycle; ARMON_MGPU_THREADS=0 or
 * armon_hip_mgpu_set_threads(group, 0) keeps everything in the calling thread): eight devices fed from one thread cost
 * eight times the enqueue time of one, more than the 0.75 ms of GPU work of the tile of a 16384² grid on 8 GPUs.
 * Nothing is waited for on the host; the call returns when everything is enqueued.
 *  plan  : n_sweeps (1..3), axis[s] and dt[s] of each sweep (dt = current_dt x the splitting's factor, rounded as the run's
 *          precision rounds it), emit_p (last cycle of a run: the last sweep materialises p, ref saved_vars), emit_dt (the
 *          last sweep reduces the next CFL step and the group takes its minimum — folded, reduced and copied to dt_host on
 *          the TRANSFER streams: the compute streams go from this cycle's last sweep to the next cycle's first without
 *          waiting for it, as the reference's MPI_Iallreduce is waited for one cycle later; afterwards every tile's
 *          dt_cfl_out holds the minimum, ordered on that tile's transfer stream; 0 with cst_dt), overlap (0 = unpack and
 *          sweep in order on the compute stream), next_axis = axis of the NEXT cycle's first sweep, whose exchange is
 *          posted at the end of this call and consumed by the next one (-1 = none; a posted exchange nobody consumes is
 *          completed by armon_hip_mgpu_drain), event_slot >= 0: events event_slot + 2s / + 2s + 1 of event_ctx's pool
 *          are recorded on local tile 0's compute stream around sweep s (armon_hip_event_elapsed_ms reads them), -1 = none.
 *  tiles : per local tile the descriptors of a FULL X and a FULL Y sweep of that tile as armon_hip_sweep takes them, with
 *          *_in = the vectors that hold the state when the call is made and *_out = their partners (the same two sets in x
 *          and y); p_out / dt_cfl_out name where emit_p / emit_dt put their results; dt, bc_low / bc_high, out_lo / out_hi,
 *          dt_accumulate are set by the library (the sides from the group's topology). After the call the state is in the
 *          *_out set when n_sweeps is odd, in the *_in set when it is even.
 * Environment knobs of a group, read when it is created (measurement tools; none changes a result bit): ARMON_MGPU_THREADS=0
 * (no host threads), ARMON_MGPU_XFER_PRIORITY=normal|lowest (priority of the transfer streams; default lowest when a tile has
 * its device to itself), ARMON_MGPU_PACK=compute (halo packs in front of the interior on the compute stream, as until round
 * 4), ARMON_MGPU_TIMING=1 (host time of tile 0's steps inside the call, printed when the group is destroyed). */
typedef struct {
    int32_t n_sweeps, emit_p, emit_dt, overlap;
    int32_t axis[4];             /* [0 .. n_sweeps) used */
    double  dt[4];
    int32_t next_axis, event_slot;
    armon_ctx* event_ctx;        /* whose event pool event_slot names: a context on local tile 0's compute stream; NULL = that tile's own */
    void*   dt_host;             /* emit_dt: pinned host slot (one element of the run's precision, armon_hip_malloc_host) the   */
    int32_t dt_event_slot;       /* global minimum is copied to, and the event of local tile 0's EDGE context (armon_hip_mgpu_edge_ctx)
                                    recorded behind that copy (-1 = none): armon_hip_event_sync(edge_ctx, slot), then read *dt_host */
    int32_t reserved;
} armon_cycle_plan;
typedef struct { armon_sweep_desc x, y; } armon_tile_cycle;
typedef struct { armon_sweep_desc_f32 x, y; } armon_tile_cycle_f32;
ARMON_API int armon_hip_mgpu_cycle(armon_mgpu*, const armon_cycle_plan* plan, const armon_tile_cycle* tiles);
ARMON_API int armon_hip_mgpu_cycle_f32(armon_mgpu*, const armon_cycle_plan* plan, const armon_tile_cycle_f32* tiles);
ARMON_API int armon_hip_mgpu_drain(armon_mgpu*, const armon_tile_cycle* tiles);      /* tiles: descriptors whose *_in hold the state */
ARMON_API int armon_hip_mgpu_drain_f32(armon_mgpu*, const armon_tile_cycle_f32* tiles);
ARMON_API int armon_hip_mgpu_sync(armon_mgpu*);       /* host waits for the compute AND transfer streams of every local tile */
ARMON_API int armon_hip_mgpu_set_threads(armon_mgpu*, int on);                        /* 1 / 0; < 0 = by the environment */
/* The body force of the group's cycles (armon_hip_body_force), stored in the group: from now on every
 * armon_hip_mgpu_cycle[_f32] ends with the kick of every local tile's real cells — dt = the sum of the plan's dt[s] over the
 * sweeps along axis[0] (current_dt under every splitting of the reference), rounded to the run's precision like gx, gy —
 * after the cycle's last sweep AND the join of its strips, on the tile's compute stream: behind it in stream order come
 * the event that the packs of the exchange posted ahead wait for, so the neighbour receives kicked cells, and the next
 * cycle's sweeps. The CFL step the last sweep emits is that of the velocities before the kick. (0, 0) = no force (the
 * default): nothing is launched. Refused: a NULL group, a NaN or an infinity. The layouts of armon_cycle_plan,
 * armon_tile_cycle and armon_sweep_desc do not change. */
ARMON_API int armon_hip_mgpu_set_body_force(armon_mgpu*, double gx, double gy);

/* Host-value all-reduce over the PROCESSES of the group (the conservation sums, ref src/reductions.jl:317-320);
 * op 0 = sum, 1 = min; count <= 16; synchronous; the caller folds its own local tiles first. */
ARMON_API int armon_hip_mgpu_allreduce_host(armon_mgpu*, int op, int count, double* values);

/* border_domain(bsize, side) / ghost_domain(bsize, side) with all ghost layers (ref src/blocking/blocking.jl:141-187,
 * single_strip=false) and real_face_size (ref :210) of a tile of nx x ny real cells, 0-based; outputs nullable. */
ARMON_API int armon_hip_halo_ranges(int64_t nx, int64_t ny, int nghost, int side, armon_range* border,
                                    armon_range* ghost, int64_t* face);

#ifdef __cplusplus
}
#endif
#endif /* ARMON_HIP_H */
