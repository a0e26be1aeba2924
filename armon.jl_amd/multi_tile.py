"""Tile-decomposed runs driven through the library's own multi-GPU entry points (include/armon_hip.h:
``armon_hip_mgpu_init`` / ``armon_hip_halo_exchange_start|finish`` / ``armon_hip_dt_allreduce``).

``TileGroup`` keeps every tile of a px × py decomposition in ONE process — the shape a Julia host without MPI, or
a one-GPU rehearsal of the 8-GPU layout, uses: tile r on device ``device_ids[r]`` (all on device 0 by default), each
with its own compute and transfer stream, faces moved by peer copies ordered by events only. The cycle below is the
reference's ``solver_cycle`` (ref src/solver.jl:288-320) with ``block_ghost_exchange`` (ref src/halo_exchange.jl:
286-368) replaced by the native exchange, the interior of each fused sweep enqueued between its start and its finish
(the overlap the reference gets from its asynchronous block state machine, ref src/solver.jl:58-285), and the dt
minimum reduced on the device (ref src/solver_state.jl:89-111). The host never synchronises inside a cycle.

``NativeRcclExchanger`` is the one-process-per-GPU counterpart (``armon_hip_mgpu_init_rank``): the same native
choreography over RCCL send/recv, plugged into ``solver.overlapped_sweep`` in place of the torch.distributed
``HaloExchanger``. Both are a ``NativeGroup`` — the wrapper of an ``armon_mgpu`` handle and of its local tiles — which is
what ``solver.overlapped_sweep`` drives call by call and whose ``native_cycle`` enqueues a whole cycle in one call.
"""
import ctypes as C
import time as _time

import numpy as np

from . import _lib
from ._lib import CyclePlan, HaloDesc, TileCycle, check
from .blocking import Axis, Side, sides_along
from .parameters import PROC_NULL, ArmonParameters
from . import solver as S


def _halo_descs(params_list, grids, names):
    descs = (HaloDesc * len(grids))()
    for d, p, g in zip(descs, params_list, grids):
        d.nx, d.ny = p.N
        d.nghost, d.nvars = p.nghost, len(names)
        for k, f in enumerate(names):
            d.vars[k] = g.data[f].ptr
    return descs


def tile_cycle_descs(params_list, grids):
    """``armon_tile_cycle[n]``: per tile the descriptors of a full X and a full Y sweep from the set of vectors that holds the
    state NOW into its partner (armon_hip_mgpu_cycle fills in the steps, the sides and the cycle's outputs)."""
    tcs = (TileCycle * len(grids))()
    for tc, p, g in zip(tcs, params_list, grids):
        tc.x = S.sweep_desc(p, g, Axis.X, 0., p.cell_size(0), emit_p=True, emit_dt=True)
        tc.y = S.sweep_desc(p, g, Axis.Y, 0., p.cell_size(1), emit_p=True, emit_dt=True)
    return tcs


def cycle_plan(params, gdt, last_cycle, prefetch=True, dt_host=None):
    """``armon_cycle_plan`` of the cycle ``gdt`` is about to run (ref split_axes + update_solver_state!,
    src/axis_splitting.jl:24-46, src/solver_state.jl:339-345). ``dt_host``: pinned array of two elements, the landing zone
    of the next CFL step (slot = parity of the cycle; the event of that slot is recorded on tile 0's edge context)."""
    sweeps = S.split_axes(params.axis_splitting, gdt.cycle)
    plan = CyclePlan(n_sweeps=len(sweeps), emit_p=int(last_cycle), emit_dt=int(not params.cst_dt),
                     overlap=int(params.overlap_halo), next_axis=-1, event_slot=-1, dt_event_slot=-1)
    if dt_host is not None and not params.cst_dt:
        plan.dt_host = dt_host.ptr + (gdt.cycle & 1) * np.dtype(params.data_type).itemsize
        plan.dt_event_slot = S.DT_EVENT_SLOT + (gdt.cycle & 1)
    for k, (axis, dt_factor) in enumerate(sweeps):
        plan.axis[k] = int(axis) - 1
        plan.dt[k] = gdt.current_dt * params.T(dt_factor)
    if prefetch and not last_cycle and params.overlap_halo:
        plan.next_axis = int(S.split_axes(params.axis_splitting, gdt.cycle + 1)[0][0]) - 1
    names = ["sweep_x" if a == Axis.X else "sweep_y" for a, _ in sweeps]
    for cb in params.kernel_callbacks:        # timers that can hand out event slots (bench.py's EventTimer)
        if hasattr(cb, "reserve"):
            plan.event_slot = cb.reserve(names)
            plan.event_ctx = params.device.ctx      # the pool the timer reads (a rank's own context shares the tile's stream)
    return plan, len(sweeps)


class NativeGroup:
    """An ``armon_mgpu`` handle and its local tiles (``params``, ``grids``): all tiles of an in-process group
    (``TileGroup``) or this rank's one tile of an RCCL group (``NativeRcclExchanger``). It is the ``link`` of
    ``solver.overlapped_sweep`` (start / finish / finish_edge / edge_join / edges) and the exchanger of the staged path
    (``exchange``), and ``native_cycle`` is the one place that calls ``armon_hip_mgpu_cycle``."""

    native = True

    def _adopt(self, params, grids):
        """The local tiles of ``self.handle``: check the library's topology against theirs, fetch their edge streams."""
        L = self._L
        self.params, self.grids, self.root = params, grids, params[0]
        self.edges = []             # per tile: its transfer stream as a context, its two edge-dt scalars (device address)
        for k, p in enumerate(params):
            rank, coords, nb = C.c_int(), (C.c_int * 2)(), (C.c_int * 4)()
            check(L.armon_hip_mgpu_tile_info(self.handle, k, C.byref(rank), C.byref(coords), C.byref(nb)))
            # the library's topology is the reference's (and this package's) cartesian grid
            assert rank.value == p.rank and tuple(coords) == p.cart_coords
            assert [p.neighbours[s] for s in (Side.Left, Side.Right, Side.Bottom, Side.Top)] == list(nb)
            self.edges.append((C.c_void_p(L.armon_hip_mgpu_edge_ctx(self.handle, k)), int(L.armon_hip_mgpu_edge_dt(self.handle, k))))
        if self.root.forced:        # the body force of the run: the library's own cycle ends with its kick
            check(L.armon_hip_mgpu_set_body_force(self.handle, *self.root.gravity))
        self.dt = grids[0].dt       # tile 0 lands the global CFL step (solver.DtReadback)
        self._tcs = {}              # tile-cycle descriptors per ping-pong parity (key: where each tile's rho lives)

    def _fn(self, name):
        return getattr(self._L, "armon_hip_" + name + self.root.suffix)

    def _tile_cycles(self):
        key = tuple(g.data["rho"].ptr for g in self.grids)
        if key not in self._tcs:
            self._tcs[key] = tile_cycle_descs(self.params, self.grids)
        return self._tcs[key]

    def set_chaos(self, max_delay_us, seed=0):
        """Test aid: random busy-wait kernels in front of the group's stream operations (armon_hip_mgpu_set_chaos)."""
        check(self._L.armon_hip_mgpu_set_chaos(self.handle, int(max_delay_us), int(seed)))

    def wait(self):
        check(self._L.armon_hip_mgpu_sync(self.handle))       # compute and transfer streams of every local tile

    def drain(self):
        """Complete an exchange the last native cycle posted ahead and no cycle consumed → whether there was such a cycle."""
        usable = bool(self.handle) and S.native_cycle_usable(self.root)
        if usable:
            check(self._fn("mgpu_drain")(self.handle, self._tile_cycles()))
        return usable

    def close(self):
        if self.handle:
            self._L.armon_hip_mgpu_destroy(self.handle)
            self.handle = None

    # ---- native exchange / reduction ----------------------------------------------------------------------------
    def exchange_start(self, axis, names):
        check(self._fn("halo_exchange_start")(self.handle, int(axis) - 1, _halo_descs(self.params, self.grids, names)))

    def exchange_finish(self, axis, names):
        check(self._fn("halo_exchange_finish")(self.handle, int(axis) - 1, _halo_descs(self.params, self.grids, names)))

    def exchange_finish_edge(self, axis, names):
        """Unpack on the transfer streams (no wait on the compute streams): the strips follow there, then ``edge_join``."""
        check(self._fn("halo_exchange_finish_edge")(self.handle, int(axis) - 1, _halo_descs(self.params, self.grids, names)))

    def start(self, sides, names):
        """The exchanger interface (``halo_exchange.HaloExchanger``): ``sides`` are the two sides of one axis."""
        if not any(p.neighbours[s] != PROC_NULL for p in self.params for s in sides):
            return None
        axis = Axis.X if sides[0] in (Side.Left, Side.Right) else Axis.Y
        self.exchange_start(axis, names)
        return axis, tuple(names)

    def finish(self, handle):
        if handle is not None:
            self.exchange_finish(*handle)

    def finish_edge(self, handle):
        if handle is not None:
            self.exchange_finish_edge(*handle)

    def exchange(self, sides, names):
        self.finish(self.start(sides, names))

    def edge_join(self, with_dt):
        ptrs = (C.c_void_p * len(self.grids))(*[g.dt_scalar.ptr for g in self.grids]) if with_dt else None
        check(self._fn("mgpu_edge_join")(self.handle, ptrs))

    def dt_allreduce(self, scalars=None):
        """Global minimum of every local tile's device scalar (``grid.dt_scalar`` by default), in place."""
        scalars = [g.dt_scalar for g in self.grids] if scalars is None else scalars
        check(self._fn("dt_allreduce")(self.handle, (C.c_void_p * len(scalars))(*[a.ptr for a in scalars])))

    def native_cycle(self, gdt, last_cycle):
        """One solver cycle of every local tile in one library call (one host thread per tile inside): exchanges, sweeps,
        the global minimum of the next CFL step and its read-back, posted on tile 0's transfer stream. What is left for the
        host is to pick up the step the previous cycle posted."""
        p0, dt = self.root, self.dt
        deferred = (gdt.cycle - 1) in dt.inflight
        plan, n_sweeps = cycle_plan(p0, gdt, last_cycle, dt_host=dt.landing())
        check(self._fn("mgpu_cycle")(self.handle, C.byref(plan), self._tile_cycles()))
        if n_sweeps & 1:
            for g in self.grids:
                g.swap_state()
        if not p0.cst_dt:
            dt.inflight[gdt.cycle] = self.edges[0][0]
            if deferred:
                gdt.update_dt(dt.take(gdt.cycle - 1))


class TileGroup(NativeGroup):
    """All tiles of a ``P = (px, py)`` decomposition of one problem, in this process."""

    def __init__(self, P, device_ids=None, force_peer_copy=False, **options):
        """``periodic=(x, y)``, or a problem with ``"Periodic"`` sides: the domain is periodic along that axis — the tiles'
        neighbours wrap around (``armon_hip_mgpu_set_periodic``). ``force_peer_copy`` is a test aid for the
        transport (``armon_hip_mgpu_force_peer_copy``): ``hipMemcpyPeerAsync`` for every face and dt scalar even though the
        tiles share a device."""
        from .parameters import resolve_periodic
        self.handle = None
        periodic = resolve_periodic(options.get("test", "Sod"), options.get("periodic"))     # (refused before anything is created)
        if options.get("scalars") or getattr(options.get("test"), "scalars", None):
            _lib.solver_error("config", "passive scalars are not supported for a tile group (DESIGN.md §4.14): one block only")
        test = options.get("test")
        own = lambda key: options.get(key) if options.get(key) is not None else getattr(test, key, 0)
        if own("viscosity") != 0 or own("heat_diffusivity") != 0:      # (a diffusing scalar is a scalar: refused above)
            _lib.solver_error("config", "physical diffusion is not supported for a tile group (DESIGN.md §4.15): its stencil needs "
                                        "a corner-carrying halo of the post-sweep state, which the exchange does not have; one "
                                        "block only")
        L = _lib.lib()
        self.P = (int(P[0]), int(P[1]))
        nt = self.P[0] * self.P[1]
        ids = list(device_ids) if device_ids is not None else [0] * nt
        assert len(ids) == nt
        self.handle = C.c_void_p()
        check(L.armon_hip_mgpu_init(self.P[0], self.P[1], (C.c_int * nt)(*ids), C.byref(self.handle)))
        self._L = L
        if any(periodic):
            check(L.armon_hip_mgpu_set_periodic(self.handle, int(periodic[0]), int(periodic[1])))
        if force_peer_copy:
            check(L.armon_hip_mgpu_force_peer_copy(self.handle, 1))
        for k in ("use_MPI", "device_id", "P"):
            options.pop(k, None)
        self.params, self.grids = [], []            # (what ``close`` releases, should a tile fail to build)
        for r in range(nt):
            ctx = C.c_void_p(L.armon_hip_mgpu_ctx(self.handle, r))
            self.params.append(ArmonParameters(**options, tile_of=(r, self.P), ctx=ctx, device_id=ids[r]))
            self.grids.append(S.BlockGrid(self.params[r]))
        self._adopt(self.params, self.grids)
        self.global_dt = self.grids[0].global_dt
        for g in self.grids:
            g.global_dt = self.global_dt               # one clock for every tile (ref GlobalTimeStep is global)
        self.dt_inflight = self.dt.inflight

    def set_threads(self, on):
        """One host thread per tile inside ``armon_hip_mgpu_cycle`` (default) or everything from the calling thread."""
        check(self._L.armon_hip_mgpu_set_threads(self.handle, int(on)))

    def close(self):
        if self.handle:
            # the tile contexts belong to the group: release everything allocated through them first
            for g in self.grids:
                for a in list(g.data.values()) + (list(g.alt.values()) if g.alt else []) + [g.dt_scalar]:
                    a.free()
                g.dt.free()
            super().close()
            for p in self.params:
                if p._device is not None:
                    p._device.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- solver ---------------------------------------------------------------------------------------------------
    def init_test(self):
        for p, g in zip(self.params, self.grids):
            S.init_test(p, g)

    def conservation_vars(self):
        mass = energy = 0.
        for p, g in zip(self.params, self.grids):
            m, e = S.conservation_vars(p, g)
            mass, energy = mass + m, energy + e
        return mass, energy

    def _staged_sweep(self, axis, dt, dx):
        for p, g in zip(self.params, self.grids):
            S.update_EOS(p, g, axis)
        self.exchange(sides_along(axis), S.COMM_VARS)
        for p, g in zip(self.params, self.grids):
            for side in sides_along(axis):
                if p.neighbours[side] == PROC_NULL:
                    S.boundary_conditions(p, g, axis, side)
            S.numerical_fluxes(p, g, axis, dt, dx)
            S.cell_update(p, g, axis, dt, dx)
            S.projection_remap(p, g, axis, dt, dx)

    def _local_dt_to_device(self):
        """dtCFL of every tile into its device scalar (no host round trip), then the global minimum."""
        for p, g in zip(self.params, self.grids):
            r = p.block_size.domain_range(*p.steps_ranges[Axis.X].real_domain).to_c()
            check(p.fn("dtCFL_async")(p.device.ctx, r, p.cell_size(0), p.cell_size(1), g.ptr("u"), g.ptr("v"),
                                        g.ptr("c"), C.c_void_p(g.dt_scalar.ptr)))
        self.dt_allreduce()

    def solver_cycle(self, last_cycle=True):
        """ref src/solver.jl:288-320 over every tile."""
        p0, gdt, readback, scalar = self.root, self.global_dt, self.dt, self.grids[0].dt_scalar
        fused = p0.use_fused_sweep
        deferred = (gdt.cycle - 1) in readback.inflight
        if gdt.cycle == 0:
            for p, g in zip(self.params, self.grids):
                S.update_EOS(p, g)
        if not deferred and not p0.cst_dt:
            self._local_dt_to_device()
            readback.post(gdt.cycle, scalar)     # tile 0's scalar: already the global minimum, ordered on its stream
            gdt.update_dt(readback.take(gdt.cycle))
            if fused and gdt.cycle == 0:
                for g in self.grids:
                    g.release_scratch()          # c, g: only the EOS + dtCFL of cycle 0 needed them
        if S.native_cycle_usable(p0):
            return self.native_cycle(gdt, last_cycle)
        tiles = list(zip(self.params, self.grids))
        sweeps = S.split_axes(p0.axis_splitting, gdt.cycle)
        for k, (axis, dt_factor) in enumerate(sweeps):
            dx = p0.cell_size(int(axis) - 1)
            dt = gdt.current_dt * p0.T(dt_factor)
            if not fused:
                self._staged_sweep(axis, dt, dx)
                continue
            last = k == len(sweeps) - 1
            S.overlapped_sweep(tiles, self, axis, dt, dx, emit_p=last and last_cycle, emit_dt=last and not p0.cst_dt)
            if last:
                for p, g in tiles:               # each tile kicks its own real cells, on its compute stream (strips joined)
                    S.body_force(p, g, gdt.current_dt)
            if last and not p0.cst_dt:
                self.dt_allreduce()
                readback.post(gdt.cycle, scalar)
                if deferred:
                    gdt.update_dt(readback.take(gdt.cycle - 1))
        if not fused:
            for p, g in tiles:
                S.body_force(p, g, gdt.current_dt)

    def time_loop(self):
        """ref src/solver.jl:323-403"""
        p0, gdt = self.root, self.global_dt
        from .checkpoint import checkpoint_path
        gdt.reset()
        self.dt_inflight.clear()
        if p0.restart_from is not None:
            self.load_state(p0.restart_from)
        if p0.start_from_exact is not None:
            self.fill_exact(time=p0.start_from_exact, samples=p0.error_norms_samples)
            gdt.time = p0.T(p0.start_from_exact)     # the clock starts where the solution was taken
            if p0.check_result or p0.silent <= 1:
                p0.initial_mass, p0.initial_energy = self.conservation_vars()
        self.wait()
        t1 = _time.perf_counter_ns()
        maxtime = p0.T(p0.maxtime)
        saved_at, save_ns = -1, 0         # checkpoints are disk I/O: their time is taken out of the solve time
        compared_at, stopped = -1, False  # (and so is the time of the comparisons with a reference run's checkpoints)
        self.state_diffs = []
        profiled_at, self.profiles = -1, []   # (and the time of the profiles)
        normed_at, self.error_norms_taken = -1, []   # (and of the error norms)
        imaged_at, self.images = -1, []       # (and of the image frames)
        hist, dt_used, self.history = None, 0.0, None
        if p0.history_step != 0:
            from .history import HistoryRun
            hist = HistoryRun(self, p0)       # (the reads of its rings and its file are taken out too: hist.io_ns)
            hist.start(gdt)
        while gdt.time < maxtime and gdt.cycle < p0.maxcycle:
            self.solver_cycle(last_cycle=S.cycle_ends(p0, gdt))
            dt_used = float(gdt.current_dt)   # the step this cycle advanced by
            gdt.next_cycle()
            if hist is not None and gdt.cycle % p0.history_step == 0:
                hist.sample(gdt, dt_used)     # with the tiles at rest: the strips of a cycle are written on the transfer streams
            if p0.checkpoint_step != 0 and gdt.cycle % p0.checkpoint_step == 0:
                if hist is not None:
                    hist.flush()
                self.wait()
                t_save = _time.perf_counter_ns()
                self.save_state(checkpoint_path(p0, gdt.cycle))
                save_ns += _time.perf_counter_ns() - t_save
                saved_at = gdt.cycle
            if p0.profile_step != 0 and gdt.cycle % p0.profile_step == 0:
                from .profile import profile_run
                self.wait()
                t_save = _time.perf_counter_ns()
                profile_run(self, p0, gdt)
                save_ns += _time.perf_counter_ns() - t_save
                profiled_at = gdt.cycle
            if p0.image_step != 0 and gdt.cycle % p0.image_step == 0:
                from .derived import image_run
                self.wait()
                t_save = _time.perf_counter_ns()
                image_run(self, p0, gdt)
                save_ns += _time.perf_counter_ns() - t_save
                imaged_at = gdt.cycle
            if p0.error_norms_step != 0 and gdt.cycle % p0.error_norms_step == 0:
                from .analytic import error_norms_run
                self.wait()
                t_save = _time.perf_counter_ns()
                error_norms_run(self, p0, gdt)
                save_ns += _time.perf_counter_ns() - t_save
                normed_at = gdt.cycle
            if p0.compare_step != 0 and gdt.cycle % p0.compare_step == 0:
                from .compare import compare_run
                self.wait()
                t_save = _time.perf_counter_ns()
                stopped = compare_run(self, p0, gdt)
                save_ns += _time.perf_counter_ns() - t_save
                compared_at = gdt.cycle
                if stopped:
                    break                 # the first difference ends the run (ref @checkpoint, src/solver.jl:40-55)
        self.drain()
        self.wait()
        solve_ns = _time.perf_counter_ns() - t1 - save_ns - (hist.io_ns if hist is not None else 0)
        if hist is not None:
            hist.finish(gdt, dt_used)
        if p0.checkpoint_at_end and saved_at != gdt.cycle:
            self.save_state(checkpoint_path(p0, gdt.cycle))
        if p0.profile_at_end and profiled_at != gdt.cycle:
            from .profile import profile_run
            profile_run(self, p0, gdt)
        if p0.image_at_end and imaged_at != gdt.cycle:
            from .derived import image_run
            image_run(self, p0, gdt)
        if p0.error_norms_at_end and normed_at != gdt.cycle:
            from .analytic import error_norms_run
            error_norms_run(self, p0, gdt)
        if p0.compare_at_end and compared_at != gdt.cycle and not stopped:
            from .compare import compare_run
            compare_run(self, p0, gdt)
        return solve_ns

    def run(self):
        """``armon(params)`` for the whole group → SolverStats (``data`` = this group)."""
        self.init_test()
        solve_ns = self.time_loop()
        gdt, g = self.global_dt, self.root.global_grid
        cells = g[0] * g[1]
        return S.SolverStats(float(gdt.time), float(gdt.current_dt), gdt.cycle, solve_ns / 1e9, cells,
                             gdt.cycle * cells / max(solve_ns, 1), data=self, state_diffs=list(self.state_diffs),
                             profiles=list(self.profiles), error_norms=list(self.error_norms_taken), history=self.history,
                             images=list(self.images))

    # ---- checkpoint / restart (checkpoint.py) ---------------------------------------------------------------------
    def _tiles_at_rest(self):
        """Every tile with nothing of the group in flight: an exchange posted ahead is completed (the next cycle then posts its
        own, as at cycle 0) and all streams are idle."""
        self.drain()
        self.wait()
        return list(zip(self.params, self.grids))

    def state_digest(self, names=S.STATE_VARS):
        """``BlockGrid.state_digest`` of the whole domain: the sum mod 2^64 of the tiles' digests = the single block's."""
        from . import checkpoint
        return checkpoint.state_digest(self._tiles_at_rest(), tuple(names))

    def save_state(self, path, band_rows=None, compress=None):
        """Each tile writes its window of the GLOBAL planes: the file is byte-identical to the single block's."""
        from . import checkpoint
        return checkpoint.save(self._tiles_at_rest(), self.global_dt, self.dt, path, band_rows=band_rows, compress=compress)

    def load_state(self, path, band_rows=None):
        from . import checkpoint
        return checkpoint.load(self._tiles_at_rest(), self.global_dt, self.dt, path, band_rows=band_rows)

    def compare_state(self, ref, rtol=None, atol=0.0, names=None, limit=20, band_rows=None):
        """``BlockGrid.compare_state`` of the whole domain: the merge of the tiles' records = the single block's."""
        from . import compare
        return compare.compare_state(self._tiles_at_rest(), ref, rtol=rtol, atol=atol, names=names, limit=limit, band_rows=band_rows)

    def profile(self, kind, bins=None, width=1, centre=None, dr=None, with_p=True, scale_exp=None):
        """``BlockGrid.profile`` of the whole domain: the merge of the tiles' records = the single block's, word for word."""
        from . import profile
        return profile.profile_state(self._tiles_at_rest(), kind, bins=bins, width=width, centre=centre, dr=dr, with_p=with_p,
                                     scale_exp=scale_exp)

    def error_norms(self, reference=None, time=None, samples=1, coord_range=None, window=None, scale_exp=None):
        """``BlockGrid.error_norms`` of the whole domain: the merge of the tiles' records = the single block's, word for word.
        ``window``: ``(col0, row0, wnx, wny)`` in real cells of the GLOBAL grid; each tile takes the part it holds."""
        from . import analytic
        tiles = self._tiles_at_rest()
        return analytic.error_norms_state(tiles, reference, time=time, samples=samples, coord_range=coord_range,
                                          windows=None if window is None else analytic.tile_windows(tiles, window), scale_exp=scale_exp)

    def fill_exact(self, reference=None, time=None, samples=1, coord_range=None, window=None):
        """``BlockGrid.fill_exact`` of the whole domain: every tile fills its own real cells (of the global ``window``)."""
        from . import analytic
        tiles = self._tiles_at_rest()
        return analytic.fill_state(tiles, reference, time=time, samples=samples, coord_range=coord_range,
                                   windows=None if window is None else analytic.tile_windows(tiles, window))

    def history_sample(self, gauges=(), scale_exp=None):
        """``BlockGrid.history_sample`` of the whole domain: the merge of the tiles' records = the single block's, word for
        word; each gauge is taken from the tile that owns its cell."""
        from . import history
        return history.sample_state(self._tiles_at_rest(), gauges=gauges, scale_exp=scale_exp)

    def derive(self, quantities, factor=1, reduce="mean"):
        """``BlockGrid.derive`` of the whole domain. The tiles come to rest, ``rho, u, v, E`` are exchanged along both axes so
        that the first ghost layer of every side with a neighbour holds that tile's cells (ghost contents at a cycle boundary
        are not part of the state: every sweep refreshes what it reads), each tile runs the kernel with the bits of those sides
        set, and the coarse planes are assembled into the GLOBAL coarse grid like ``coarsen`` (same alignment rule). Central
        differences across tile edges, exact per-cell arithmetic and the fixed summation order: the planes equal the single
        block's bit for bit. → dict name → ``(cny, cnx)`` array, plus ``x``, ``y``."""
        from . import derived
        from .parameters import check_coarsen_alignment, normalize_coarsen_factor
        derived.normalize_request(quantities, reduce)          # (a bad request is refused before anything moves)
        f = normalize_coarsen_factor(factor)
        if f is None:
            _lib.solver_error("config", "derive needs a factor >= 1")
        for p in self.params:
            check_coarsen_alignment(p, f)
        tiles = self._tiles_at_rest()
        for axis in (Axis.X, Axis.Y):
            self.exchange(sides_along(axis), S.STATE_VARS)
        self.wait()
        res = derived.derive_state(tiles, quantities, factor=f, reduce=reduce)
        cnx, cny = res[next(iter(res))].shape[::-1]
        for k in ("x", "y"):
            res[k] = np.empty((cny, cnx), dtype=self.root.data_type)
        for p, g in tiles:
            x, y = g.coarse_coordinates(f)
            ox, oy = (p.N_origin[0] - 1) // f[0], (p.N_origin[1] - 1) // f[1]
            res["x"][oy:oy + x.shape[0], ox:ox + x.shape[1]] = x
            res["y"][oy:oy + y.shape[0], ox:ox + y.shape[1]] = y
        return res

    def gather(self, names=("rho", "u", "v", "E", "p")):
        """The real cells of every tile assembled into global (NY, NX) arrays on the host."""
        self.wait()
        gx, gy = self.root.global_grid
        out = {k: np.empty((gy, gx), dtype=self.root.data_type) for k in names}
        for p, g in zip(self.params, self.grids):
            ox, oy = p.N_origin[0] - 1, p.N_origin[1] - 1
            nx, ny = p.N
            for k in names:
                out[k][oy:oy + ny, ox:ox + nx] = g.real_view(g.data[k].to_host())
        return out

    def coarsen(self, factor=None, with_p=True):
        """``BlockGrid.coarsen`` for the whole group: each tile coarsens its own cells on its device, the coarse planes are
        assembled into the GLOBAL coarse grid on the host. Coarse cells are defined on the global grid, so every tile must
        start on a coarse-cell boundary ((N_origin - 1) % f == 0 along both axes: a configuration error otherwise); the
        summation order of a coarse cell does not depend on where its cells are stored, so with exact arithmetic the planes
        equal those of the same run in a single block, bit for bit. ``factor`` defaults to the ``output_coarsen`` option."""
        from .parameters import check_coarsen_alignment, coarse_shape, normalize_coarsen_factor
        factor = self.root.output_coarsen if factor is None else normalize_coarsen_factor(factor)
        if factor is None:
            _lib.solver_error("config", "coarsen needs a factor >= 1 (or the output_coarsen option)")
        for p in self.params:
            check_coarsen_alignment(p, factor)
        self.wait()
        cnx, cny = coarse_shape(self.root.global_grid, factor)
        out = {}
        for p, g in zip(self.params, self.grids):
            planes = g.coarsen(factor, with_p=with_p)
            ox, oy = (p.N_origin[0] - 1) // factor[0], (p.N_origin[1] - 1) // factor[1]
            for k, a in planes.items():
                if k not in out:
                    out[k] = np.empty((cny, cnx), dtype=a.dtype)
                out[k][oy:oy + a.shape[0], ox:ox + a.shape[1]] = a
        return out


class NativeRcclExchanger(NativeGroup):
    """One process per GPU: this rank's tile exchanges its halos and reduces dt through the library's RCCL group
    (``armon_hip_mgpu_init_rank``). Same interface as ``halo_exchange.HaloExchanger`` (start / finish / exchange /
    allreduce_min_device_async), so ``solver.overlapped_sweep`` and the staged ``block_ghost_exchange`` drive
    it unchanged. The rendezvous (128-byte RCCL ids from rank 0) travels through torch.distributed's store — the
    launcher's job, as MPI_Bcast would be for a Julia host."""

    stream_ordered = True           # everything is ordered on the device: the host never waits inside a cycle

    def __init__(self, params, grid):
        import torch.distributed as dist
        L = _lib.lib()
        self._L = L
        group = params.global_comm
        buf = C.create_string_buffer(_lib.MGPU_ID_BYTES)
        obj = [None]
        if params.rank == 0:
            # a failure here (no RCCL in the process) still has to reach the broadcast every other rank is waiting in
            try:
                check(L.armon_hip_mgpu_unique_id(buf))
                obj = [bytes(buf.raw)]
            except _lib.SolverException as e:
                obj = [str(e)]
        dist.broadcast_object_list(obj, src=0, group=group)
        if not isinstance(obj[0], bytes):
            raise _lib.SolverException("cpp", f"rank 0 could not create the RCCL ids: {obj[0]}")
        ident = C.create_string_buffer(obj[0], _lib.MGPU_ID_BYTES)
        # Local part first (RCCL symbols, context, streams, scratch: it can fail on one rank alone), then the ranks agree
        # over the launcher's group, and only then the collective ncclCommInitRank — entered by every rank or by none: a
        # rank that skipped it after a local failure would leave the others blocked in it for ever.
        self.handle, err = C.c_void_p(), None
        try:
            dev = params.device                 # the tile's kernels keep running on the context the run already uses
            check(L.armon_hip_mgpu_prepare_rank(params.proc_dims[0], params.proc_dims[1], params.rank, params.device_id,
                                                C.c_void_p(dev.stream), C.byref(self.handle)))
            if any(params.periodic):
                check(L.armon_hip_mgpu_set_periodic(self.handle, int(params.periodic[0]), int(params.periodic[1])))
        except Exception as e:           # ANY local failure must still reach the all_gather every other rank is waiting in
            err = e
        ready = [None] * dist.get_world_size(group)
        dist.all_gather_object(ready, err is None, group=group)
        if not all(ready):
            self.close()
            raise _lib.SolverException("cpp", f"native RCCL group: local initialisation failed on rank(s) "
                                              f"{[r for r, ok in enumerate(ready) if not ok]}" + (f": {err}" if err else ""))
        try:
            check(L.armon_hip_mgpu_connect(self.handle, ident))
        except BaseException:
            self.close()                 # the prepared handle (context, streams, scratch) does not outlive a failed connect
            raise
        # the group made its own context on that same stream; sweeps stay on params.device (same stream → same order)
        self._adopt([params], [grid])

    def allreduce_min_device_async(self, scalar):
        self.dt_allreduce([scalar])

    def drain(self):
        """End of a run: complete the exchange posted ahead, and let the transfer stream finish (the last reduction and its
        read-back are still on it; ``params.wait()`` only covers the compute stream)."""
        if super().drain():
            self.wait()

    def allreduce_host(self, values, op):
        v = (C.c_double * len(values))(*values)
        check(self._L.armon_hip_mgpu_allreduce_host(self.handle, 0 if op == "sum" else 1, len(values), v))
        return list(v)
