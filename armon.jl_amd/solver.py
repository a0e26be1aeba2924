"""Solver driver of the HIP backend: ``armon(params)``, ``time_loop``, ``solver_cycle`` and the dt state.

Mirrors ref src/solver.jl:288-516 (synchronous cycle — the path a device backend uses),
src/solver_state.jl:58-166 (GlobalTimeStep), src/axis_splitting.jl:24-46, and the per-block kernel
wrappers of src/kernels.jl:151-230, src/riemann_schemes.jl:46-120, src/projection_schemes.jl:44-157,
src/halo_exchange.jl:32-36,286-368, src/reductions.jl:89-110,164-199,301-323. Every kernel call goes
through the C ABI of libarmon_hip.so; nothing here computes on the host.
"""
import ctypes as C
import math
import time as _time
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import BlockDataPtrs, FIELDS, SweepDesc, check, solver_error
from .blocking import Axis, Side, first_side, last_side, sides_along
from .parameters import LIMITERS, PROC_NULL, PROJECTIONS, SCHEMES
from .problem import SCALAR_PREFIX

MAIN_VARS = ("x", "y", "rho", "u", "v", "E", "p", "c", "g", "us", "ps")   # ref src/blocking/blocks.jl:47
SAVED_VARS = ("x", "y", "rho", "u", "v", "p")                              # ref :49
COMM_VARS = ("rho", "u", "v", "E", "p", "c", "g")                          # ref :50
STATE_VARS = ("rho", "u", "v", "E")


@dataclass
class SolverStats:   # ref src/solver.jl:13-23
    final_time: float
    last_dt: float
    cycles: int
    solve_time: float          # seconds
    cell_count: int
    giga_cells_per_sec: float
    data: object = None
    timer: object = None
    grid_log: object = None
    state_diffs: list = field(default_factory=list)     # (cycle, compare.StateDiff) of compare_step / compare_at_end
    profiles: list = field(default_factory=list)        # (cycle, profile.Profile) of profile_step / profile_at_end
    error_norms: list = field(default_factory=list)     # (cycle, time, analytic.ErrorNorms or None: no solution at that time) of error_norms_step / error_norms_at_end
    history: object = None                               # history.History of history_step
    images: list = field(default_factory=list)          # paths of the frames of image_step / image_at_end
    scalars: tuple = ()                                  # names of the run's passive scalars (read with stats.data.scalar(name))
    scalar_transport: str = "remap"                      # the rule the sweeps carried them with
    diffusion_steps: int = 0                             # launches of armon_hip_diffuse: the sub-steps of every cycle
    mixing: list = field(default_factory=list)          # (cycle, time, {name: mixing.MixingProfile}, {name: mixing.ScalarPDF} or None) of mixing_step / mixing_at_end

    def __str__(self):   # ref src/solver.jl:26-35
        return (f"Solver stats:\n - final time:  {self.final_time}\n - last Δt:     {self.last_dt}\n"
                f" - cycles:      {self.cycles}\n - performance: {self.giga_cells_per_sec} ×10⁹ cell-cycles/sec "
                f"({self.solve_time} sec, {self.cell_count} cells)")


class GlobalTimeStep:
    """ref src/solver_state.jl:30-166 — cycle/time/dt with the reference's one-cycle lag. All arithmetic is
    done in the run's data type T (numpy scalars), like the reference's ``GlobalTimeStep{T}``."""

    def __init__(self, params):
        self.params = params
        self.reset()

    def reset(self):   # ref :58-68
        p = self.params
        T = p.T
        self.cycle = 0
        self.time = T(0.)
        self.current_dt = T(p.Dt) if p.cst_dt else T(0.)
        self.next_cycle_dt = T(math.inf)

    def update_dt(self, new_dt):
        """ref update_dt!, :102-142 (``new_dt`` = global minimum of the local CFL time steps)."""
        p = self.params
        T = p.T
        new_dt = T(new_dt)
        previous_dt = self.current_dt
        if not math.isfinite(new_dt) or new_dt <= 0:
            solver_error("time", f"Invalid time step for cycle {self.cycle}: {new_dt}")
        elif previous_dt == 0:
            new_dt = T(p.cfl) * new_dt
        else:
            # convert(T, min(cfl·new_dt, 1.05·previous_dt)) with the 1.05 product in Float64 (ref :129)
            new_dt = T(min(float(T(p.cfl) * new_dt), 1.05 * float(previous_dt)))
        self.next_cycle_dt = new_dt
        if self.current_dt == 0:
            self.current_dt = self.next_cycle_dt

    def next_cycle(self):
        """ref next_cycle!, :145-166"""
        p = self.params
        T = p.T
        self.cycle += 1
        self.time = T(self.time + self.current_dt)
        if p.cst_dt:
            self.current_dt = self.next_cycle_dt = T(p.Dt)
            return
        self.current_dt = self.next_cycle_dt
        self.next_cycle_dt = T(math.inf)


def split_axes(splitting, cycle):
    """ref src/axis_splitting.jl:24-46 → sequence of (axis, dt_factor)."""
    even = cycle % 2 == 0
    if splitting == "Sequential":
        return ((Axis.X, 1.0), (Axis.Y, 1.0))
    if splitting in ("Godunov", "SequentialSym"):
        return ((Axis.X, 1.0), (Axis.Y, 1.0)) if even else ((Axis.Y, 1.0), (Axis.X, 1.0))
    if splitting == "Strang":
        return (((Axis.X, 0.5), (Axis.Y, 1.0), (Axis.X, 0.5)) if even
                else ((Axis.Y, 0.5), (Axis.X, 1.0), (Axis.Y, 0.5)))
    if splitting == "X_only":
        return ((Axis.X, 1.0),)
    if splitting == "Y_only":
        return ((Axis.Y, 1.0),)
    solver_error("config", f"Unknown splitting method: '{splitting}'")


# what the fused path touches in every run: the saved variables (ref saved_vars, src/blocking/blocks.jl:49) and the state
FUSED_FIELDS = ("x", "y", "rho", "u", "v", "E", "p")


class _Fields(dict):
    """The 16 ``BlockData`` vectors by name. On the staged path all of them exist from the start, as in the reference (ref
    src/blocking/blocks.jl:36-44). On the fused path only the seven of ``FUSED_FIELDS`` do — ``us, ps, work_1..4, mask`` are
    never touched by a fused run, ``c, g`` only by the EOS + dtCFL of cycle 0 — and any other is allocated on first access,
    holding what ``init_test`` would have left in it (zeros; 0 / 1 for ``mask``): a 16384² block keeps 11 + the 8 transient
    spares of the placement search instead of 20 + 8 vectors (config 5's global grid on one GPU: 172 -> 95 GB), while the
    ``BlockData`` the C ABI sees stays 16 pointers (NULL = not in ``vars_to_zero``)."""

    def __init__(self, grid, names):
        super().__init__()
        import weakref
        self._grid_ref = weakref.ref(grid)     # no reference cycle: a dropped grid must release its vectors at once (86 GB blocks follow each other in the tests)
        for f in names:
            # the state vectors are interchangeable with their ping-pong partners (placement): all of them hold the pair's
            # line-pitched intermediate when the block's cycles run through it
            self[f] = grid.params.device.empty(grid.size.n_cells, grid.params.data_type,
                                               capacity=grid.pair_cells if f in STATE_VARS else None)

    def __missing__(self, key):
        if key not in FIELDS:
            raise KeyError(key)
        grid = self._grid_ref()
        a = grid.params.device.zeros(grid.size.n_cells, grid.params.data_type)
        if key == "mask" and grid.initialised:
            g = grid.size.ghosts
            nx, ny = grid.size.real_size
            m = np.zeros((ny + 2 * g, nx + 2 * g), dtype=grid.params.data_type)
            m[g:g + ny, g:g + nx] = 1
            a.copy_from_host(m.ravel())
        self[key] = a
        grid.lazy.add(key)
        return a


def pair_usable(params):
    """The X and the Y sweep of a cycle can go through ``armon_hip_sweep_pair`` — the state between them in rows of whole
    128-B lines, which the Y march loads non-temporally — when the cycle is the library's from end to end: fused fp64
    sweeps, Sequential splitting (X then Y, every cycle), no remote side (a neighbour's ghost rows would have to arrive in
    the intermediate layout), and a block large enough for the placement of its vectors to be measured
    (``placement_min_bytes`` per vector: smaller ones gain nothing from either and keep the plain layout). Decided once per block (its vectors are allocated with room for that layout); ``pair_cycle``
    decides cycle by cycle."""
    return bool(params.use_fused_sweep and np.dtype(params.data_type).itemsize == 8 and params.axis_splitting == "Sequential"
                and not params.scalar_names   # the scalar sweep reads the pre-sweep state: the pair's Y sweep overwrites the pre-X one
                and not params.use_MPI and all(n == PROC_NULL for n in params.neighbours.values())
                and int(getattr(params, "x_kernel", 0)) == 0
                and not params.wrap[1]        # the pair's contract: physical Y sides (an X-periodic block keeps the pair)
                and params.block_size.n_cells * np.dtype(params.data_type).itemsize >= params.placement_min_bytes)


class BlockGrid:
    """One block per GPU (ref BlockGrid with use_cache_blocking=false, src/blocking/block_grid.jl:352-355):
    the 16 ``BlockData`` vectors (ref src/blocking/blocks.jl:18-44) in HBM, plus the 4 ping-pong state
    vectors the fused sweep writes to."""

    def __init__(self, params):
        self.params = params
        self.size = params.block_size
        dev = params.device
        n = self.size.n_cells
        dt_ = params.data_type
        self.initialised = False               # init_test has run (a vector created later is given its initial content)
        self.lazy = set()                      # fused path: the vectors created on first access
        # elements per state vector when the cycles run through armon_hip_sweep_pair (about 1 MB more per vector at 16384²)
        self.pair_cells = self.size.line_cells(np.dtype(dt_).itemsize) if pair_usable(params) else None
        self.data = _Fields(self, FUSED_FIELDS if params.use_fused_sweep else FIELDS)
        self.alt = {f: dev.empty(n, dt_, capacity=self.pair_cells) for f in STATE_VARS} if params.use_fused_sweep else None
        # passive scalars: plane "s:<name>" and its ping-pong partner, 2·ns more vectors; none without scalars
        self.scalar_planes = tuple(SCALAR_PREFIX + name for name in params.scalar_names)
        for f in self.scalar_planes:
            self.data[f] = dev.zeros(n, dt_)
            self.alt[f] = dev.zeros(n, dt_)
        self.placement = None                  # report of tune_placement (bench / tests)
        self.pair_cycles = 0                   # host-driven cycles that went through armon_hip_sweep_pair (a report, like placement)
        self.diffusion_steps = 0               # launches of armon_hip_diffuse (a report, likewise)
        self.global_dt = GlobalTimeStep(params)
        self.dt_scalar = dev.zeros(2, dt_)     # device scalar written by the fused dt reduction
        self.dt = DtReadback(params)           # deferred read-back of dt_scalar
        self.dt_inflight = self.dt.inflight    # (the name the drivers clear between runs)
        self.comm = None                       # set by halo_exchange.setup when use_MPI
        self.halo_prefetch = None              # (axis, handle) of an exchange posted ahead of its sweep
        self._coarse_xy = {}                   # (fx, fy) -> coordinates of the coarse cells (coarse_coordinates)
        self.state_diffs = []                  # (cycle, StateDiff) of the run's compare_step / compare_at_end
        self.profiles = []                     # (cycle, Profile) of the run's profile_step / profile_at_end
        self.error_norms_taken = []            # (cycle, time, ErrorNorms) of the run's error_norms_step / error_norms_at_end
        self.history = None                    # History of the run's history_step
        self.images = []                       # paths of the frames of the run's image_step / image_at_end
        self.mixing_samples = []               # (cycle, time, profiles, pdfs) of the run's mixing_step / mixing_at_end

    def ptr(self, name):
        return C.c_void_p(self.data[name].ptr)

    def block_data_ptrs(self):
        """``armon_block_data``: the vectors that exist (NULL for those the fused path has not needed yet)."""
        bd = BlockDataPtrs()
        for f in FIELDS:
            if f in self.data:
                setattr(bd, f, self.data[f].ptr)
        return bd

    def release_scratch(self, names=("c", "g")):
        """Fused path: free vectors that were only created on the way (``c, g`` by the EOS + dtCFL of cycle 0)."""
        for f in names:
            if f in self.lazy and f in self.data:
                self.params.wait()
                self.data.pop(f).free()
                self.lazy.discard(f)

    def swap_state(self):
        """After a fused sweep the fresh state lives in ``alt``: exchange the roles."""
        for f in STATE_VARS:
            self.data[f], self.alt[f] = self.alt[f], self.data[f]

    def swap_scalars(self):
        """After a scalar sweep the fresh planes live in ``alt``: exchange the roles."""
        for f in self.scalar_planes:
            self.data[f], self.alt[f] = self.alt[f], self.data[f]

    def scalar(self, name):
        """The real cells of the passive scalar ``name`` on the host → ``(ny, nx)`` array."""
        if name not in self.params.scalar_names:
            solver_error("config", f"no scalar {name!r}: this run carries {self.params.scalar_names}")
        self.params.wait()
        return self.real_view(self.data[SCALAR_PREFIX + name].to_host()).copy()

    def tune_placement(self, min_bytes=None, spare=None, keep_state=True):
        """Pick a good PHYSICAL placement for the 8 vectors a fused sweep streams (4 read + 4 written).

        On MI355X the same kernels on the same virtual layout run 10-20 % apart depending on where the 8
        vectors sit in HBM relative to each other: vectors allocated back to back end up at a REGULAR
        physical spacing, and for many spacings the 8 streams then keep meeting on the same channels/banks
        (tools/probes/probe_skew.hip, probe_pairs.hip: 2.93-3.77 ms for the same copy as a function of the
        spacing; random picks of 8 among 24 such vectors: 75 % at 2.71-2.79 ms, the back-to-back groups 2.94-3.08).
        Nothing visible from user space predicts it, so it is measured, natively: ``spare`` extra vectors are
        allocated, up to ``placement_tries`` assignments of the 8 roles to vectors of the pool are timed with one X
        and one Y sweep (the first one being the back-to-back assignment), the fastest is kept and the unused
        vectors are freed.

        ``keep_state=False`` (what ``init_test`` does, BEFORE it writes the initial condition):
        ``armon_hip_choose_placement`` — the vectors hold nothing yet, candidates are timed on a uniform state, the
        search may stop after 12 draws once two of them lie within 1 % of the best and 7 % under the worst; transient
        memory = the 8 ``spare`` vectors only (17 GB at 16384²). The pool is deliberately small: among 12-16 vectors
        allocated one after the other about half of the random draws land on the fast level, among 32 one in twenty
        (profiles/r02_placement_pool_sizes.txt). A pool is either slow for EVERY assignment or fast for most of them
        (profiles/r02_placement_what_it_is_not.txt), so a round is short — ``placement_tries`` = 24 draws at most, 12 when two of them already lie within 0.4 % of the best — and a round
        that found nothing is followed by a fresh batch of spares, up to ``placement_rounds`` = 8 times.
        ``keep_state=True``: ``armon_hip_tune_placement`` moves a LIVE state around (4 more vectors park it meanwhile). ~20 ms per try, outside any timed region.
        Returns the report also stored in ``self.placement``."""
        params, dev = self.params, self.params.device
        tries = params.placement_tries
        nbytes = self.data["rho"].nbytes
        if min_bytes is None:
            min_bytes = params.placement_min_bytes
        if spare is None:
            spare = 8
        if self.alt is None or tries <= 1 or nbytes < min_bytes:
            return None
        free, _total = dev.memory_info()
        spare = int(min(spare, (free * 0.8) // max(nbytes, 1) - (4 if keep_state else 0)))
        if spare < 1:
            return None
        dx = params.cell_size(0)
        dt = 1e-3 * dx                    # any small step: the arithmetic does not depend on the data
        n, dt_ = self.data["rho"].n, self.data["rho"].dtype
        pool = [self.data[f] for f in STATE_VARS] + [self.alt[f] for f in STATE_VARS]
        # every vector of the pool can end up in any role: the spares are as large as the grid's own, and the library sees
        # the whole allocation — it times the draws with armon_hip_sweep_pair when they hold its intermediate
        cap = min(v.capacity_bytes for v in pool) // dt_.itemsize
        cap_bytes = cap * dt_.itemsize
        try:
            for _ in range(spare):
                pool.append(dev.empty(n, dt_, capacity=cap))
        except _lib.SolverException:          # not enough memory after all: keep the placement we have
            for v in pool[8:]:
                v.free()
            return None
        d_x = sweep_desc(params, self, Axis.X, dt, dx)
        d_y = sweep_desc(params, self, Axis.Y, dt, params.cell_size(1), emit_dt=True)     # as in a cycle
        # A search can come back empty-handed: in about one process in four none of the draws of a 16-vector pool
        # reaches the fast level (profiles/r02_placement_pool_sizes.txt). The fast level is recognisable on its own —
        # an X + Y pair then streams its 16 vectors' worth of bytes at >= 0.93 of the 6.29 TB/s this part sustains —
        # so when the best draw stays below that, a fresh batch of spares is allocated NEXT TO the losers (freeing them
        # first would hand back the same memory) and the search is repeated with the best assignment so far as its
        # first draw, at most `placement_rounds` times. (Arithmetic-bound sweeps — exact flavour, Bizarrium — may never
        # reach the mark: they just use their rounds.)
        rounds = max(1, params.placement_rounds) if not keep_state else 1
        # (fp32 sweeps top out at 0.89-0.91 of that rate, so their mark sits at 0.88: the search must be able to stop)
        fast_frac = 0.88 if np.dtype(params.data_type).itemsize == 4 else 0.93
        fast_ms = 2 * 8 * nbytes / (fast_frac * 6.29e12) * 1e3
        losers, all_times, report_rounds = [], [], 0
        best = pool[:8]                           # what the grid uses if nothing better is found
        while True:
            report_rounds += 1
            ptrs = (C.c_void_p * len(pool))(*[v.ptr for v in pool])
            picks, times, done = (C.c_int * 8)(), (C.c_double * tries)(), C.c_int(tries)
            try:
                if keep_state:
                    check(params.fn("tune_placement")(dev.ctx, C.byref(d_x), C.byref(d_y), ptrs, len(pool), cap_bytes, tries,
                                                      C.byref(picks), times))
                else:
                    check(params.fn("choose_placement")(dev.ctx, C.byref(d_x), C.byref(d_y), ptrs, len(pool), cap_bytes,
                                                        tries, 0.004, C.byref(picks), times, C.byref(done)))
            except _lib.SolverException:          # e.g. no room for the 4 transient vectors: nothing was moved in THIS round
                # pool[:8] is the assignment this round started from — the grid's own vectors in round 1, the best of the
                # previous rounds afterwards (the grid's original vectors may then be among the losers): install it before
                # anything is freed, so that the grid never points at a released vector
                for k, f in enumerate(STATE_VARS):
                    self.data[f], self.alt[f] = best[k], best[4 + k]
                for v in pool[8:] + losers:
                    v.free()
                return None
            picks, times = list(picks), list(times)[:done.value]
            all_times.append([round(t, 3) for t in times])
            best = [pool[k] for k in picks]
            losers += [v for i, v in enumerate(pool) if i not in set(picks)]
            if min(times) <= fast_ms or report_rounds >= rounds:
                break
            free, _total = dev.memory_info()
            if free < (spare + 2) * nbytes:
                break
            try:
                pool = best + [dev.empty(n, dt_, capacity=cap) for _ in range(spare)]
            except _lib.SolverException:
                break
        for k, f in enumerate(STATE_VARS):
            self.data[f], self.alt[f] = best[k], best[4 + k]
        for v in losers:
            v.free()
        flat = [t for r in all_times for t in r]
        self.placement = {"tries": len(flat), "max_tries": tries, "pool": 8 + spare, "rounds": report_rounds,
                          "x_plus_y_ms": all_times[0] if report_rounds == 1 else all_times,
                          "chosen_ms": round(min(all_times[-1]), 3), "fast_level_ms": round(fast_ms, 3),
                          "transient_GB": round((report_rounds * spare + (4 if keep_state else 0)) * nbytes / 1e9, 2)}
        return self.placement

    def device_to_host(self, names=MAIN_VARS):
        """ref device_to_host!, src/blocking/blocks.jl:121-131"""
        self.params.wait()
        return {f: self.data[f].to_host() for f in names}

    def gather(self, names, start, stride, count):
        """``count`` elements of each vector of ``names`` (at most 8), from flat index ``start`` on, ``stride`` apart, picked
        on the device (armon_hip_gather_strided) → dict name → numpy array of ``count``. Only those elements cross PCIe.
        Any of the 16 ``BlockData`` names is accepted; on the fused path one that does not exist yet is created on this
        access, like everywhere else (``_Fields``)."""
        params, dev = self.params, self.params.device
        names = tuple(names)
        out = dev.empty(max(len(names) * count, 1), params.data_type)
        try:
            vars_ = (C.c_void_p * len(names))(*[self.ptr(f) for f in names])
            check(params.fn("gather_strided")(dev.ctx, self.size.n_cells, len(names), vars_, int(start), int(stride),
                                              int(count), C.c_void_p(out.ptr)))
            host = out.to_host()[:len(names) * count].reshape(len(names), count)
        finally:
            out.free()
        return {f: host[k] for k, f in enumerate(names)}

    def coarse_coordinates(self, factor):
        """``(x, y)`` of ``coarsen``: the STORED coordinates of the first cell each coarse cell covers, taken from the block's
        ``x`` and ``y`` vectors with the gather kernel (one row of ``x``, one column of ``y``), as ``(cny, cnx)`` arrays. They
        do not change during a run: fetched once per factor and kept (read-only)."""
        from .parameters import coarse_shape
        if factor not in self._coarse_xy:
            fx, fy = factor
            nx, ny = self.size.real_size
            g, pitch = self.size.ghosts, self.size.size[0]
            cnx, cny = coarse_shape((nx, ny), factor)
            first = g * pitch + g
            xs = self.gather(("x",), first, min(fx, nx), cnx)["x"]
            ys = self.gather(("y",), first, min(fy, ny) * pitch, cny)["y"]
            x, y = np.broadcast_to(xs[None, :], (cny, cnx)).copy(), np.broadcast_to(ys[:, None], (cny, cnx)).copy()
            x.flags.writeable = y.flags.writeable = False
            self._coarse_xy[factor] = (x, y)
        return self._coarse_xy[factor]

    def coarsen(self, factor, with_p=True):
        """In-situ reduced output: the state block-averaged on the device by ``factor = f | (fx, fy)``
        (armon_hip_coarsen: ρ and p volume-averaged, u, v, E mass-weighted, real cells only) → dict of ``(cny, cnx)`` numpy
        arrays ``rho, u, v, E`` (+ ``p`` when ``with_p``) and ``x, y``. ``x, y`` are the STORED coordinates of the first cell
        each coarse cell covers, taken with the gather kernel, not recomputed on the host (``coarse_coordinates``). Only the
        coarse planes cross PCIe. On the fused path ``p`` is what the last sweep that was asked for it left
        (``solver_cycle(last_cycle=True)``). A factor other than (power of two <= 64, <= 64) goes through device scratch
        that stays with the context: see armon_hip_coarsen in include/armon_hip.h for its size."""
        from .parameters import coarse_shape, normalize_coarsen_factor
        params, dev = self.params, self.params.device
        factor = normalize_coarsen_factor(factor)
        if factor is None:
            solver_error("config", "coarsen needs a factor >= 1")
        fx, fy = factor
        nx, ny = self.size.real_size
        cnx, cny = coarse_shape((nx, ny), factor)
        names = STATE_VARS + (("p",) if with_p else ())
        out = dev.empty(len(names) * cnx * cny, params.data_type)
        try:
            check(params.fn("coarsen")(dev.ctx, self.size.size[0], self.size.ghosts, nx, ny, fx, fy,
                                       *[self.ptr(f) for f in STATE_VARS], self.ptr("p") if with_p else None,
                                       C.c_void_p(out.ptr)))
            planes = out.to_host().reshape(len(names), cny, cnx)
        finally:
            out.free()
        res = {f: planes[k] for k, f in enumerate(names)}
        res["x"], res["y"] = self.coarse_coordinates(factor)
        return res

    def state_digest(self, names=STATE_VARS):
        """64-bit digest of the real cells of each vector of ``names`` (at most 8), computed on the device
        (armon_hip_state_pack without a destination; checkpoint.py states the formula) → tuple of ints. A function of the
        values and their GLOBAL positions only: ghost cells, ghost width and decomposition do not enter, and the digests of
        the tiles of a group add up (mod 2^64) to the single block's."""
        from . import checkpoint
        return checkpoint.state_digest([(self.params, self)], tuple(names))

    def save_state(self, path, band_rows=None, compress=None):
        """Write a checkpoint of this block (checkpoint.py) → its header."""
        from . import checkpoint
        return checkpoint.save([(self.params, self)], self.global_dt, self.dt, path, band_rows=band_rows, compress=compress)

    def load_state(self, path, band_rows=None):
        """Load the state, the clock and the pending CFL step of a checkpoint over this (initialised) block → its header."""
        from . import checkpoint
        return checkpoint.load([(self.params, self)], self.global_dt, self.dt, path, band_rows=band_rows)

    def host_to_device(self, host):
        for f, a in host.items():
            self.data[f].copy_from_host(a)
        if "x" in host or "y" in host:
            self._coarse_xy.clear()

    def compare_state(self, ref, rtol=None, atol=0.0, names=None, limit=20, band_rows=None):
        """What separates this block's state from ``ref`` — a checkpoint's path, or a ``BlockGrid`` / ``TileGroup`` of the same
        global grid and data type — computed on the device (compare.py) → ``compare.StateDiff``."""
        from . import compare
        return compare.compare_state([(self.params, self)], ref, rtol=rtol, atol=atol, names=names, limit=limit, band_rows=band_rows)

    def profile(self, kind, bins=None, width=1, centre=None, dr=None, with_p=True, scale_exp=None):
        """The exact 1-D profile of this block's state along ``kind`` = ``"x" | "y" | "r"``, computed on the device
        (profile.py states the rule and the arguments) → ``profile.Profile``."""
        from . import profile
        self.params.wait()
        return profile.profile_state([(self.params, self)], kind, bins=bins, width=width, centre=centre, dr=dr, with_p=with_p,
                                     scale_exp=scale_exp)

    def mixing(self, axis="y", width=1, scalars=None, scale_exp=None, bins=None):
        """The mixing measures of this block's passive scalars along ``axis`` = ``"x" | "y"`` in bins of ``width`` cells,
        computed on the device (mixing.py states the rule and the arguments) → dict name → ``mixing.MixingProfile``."""
        from . import mixing
        self.params.wait()
        return mixing.mixing_state([(self.params, self)], axis, width=width, scalars=scalars, scale_exp=scale_exp, bins=bins)

    def scalar_pdf(self, name, bins=64, range=(0., 1.), window=None):
        """The histogram of the passive scalar ``name`` over ``bins`` equal bins of ``range = (lo, hi)``, with the exact mass
        of every bin, computed on the device (mixing.py) → ``mixing.ScalarPDF``. ``window``: ``(col0, row0, wnx, wny)`` of the
        real cells to take instead of all of them."""
        from . import mixing
        self.params.wait()
        return mixing.pdf_state([(self.params, self)], name, bins=bins, range=range, windows=None if window is None else [window])

    def derive(self, quantities, factor=1, reduce="mean"):
        """Derived flow fields of this block's state — names of ``derived.QUANTITIES`` (rho, p, e, speed, mach, grad_rho,
        vorticity, divergence) — computed on the device and reduced over the coarse cells of ``coarsen(factor)``
        (armon_hip_derive; derived.py states the rule) → dict name → ``(cny, cnx)`` array, plus ``x``, ``y`` from
        ``coarse_coordinates``. ``reduce``: ``"mean" | "max" | "min"``, or a dict quantity → name. The block is the whole
        domain: one-sided differences at its edges, where no ghost cell is read; central ones across a periodic edge
        (DESIGN.md §4.13). Only the coarse planes cross PCIe."""
        from . import derived
        from .parameters import normalize_coarsen_factor
        self.params.wait()
        # across a periodic edge the differences are central: the first ghost layer of a periodic axis is filled from the
        # opposite border (one layer, the four state vectors) and its two sides count as sides with a neighbour
        bits = 0
        for axis, sides in ((Axis.X, derived.LEFT | derived.RIGHT), (Axis.Y, derived.BOTTOM | derived.TOP)):
            if self.params.wrap[int(axis) - 1]:
                periodic_ghosts(self.params, self, axis, STATE_VARS, layers=1)
                bits |= sides
        res = derived.derive_state([(self.params, self)], quantities, factor=factor, reduce=reduce, neighbours=[bits])
        res["x"], res["y"] = self.coarse_coordinates(normalize_coarsen_factor(factor))
        return res

    def error_norms(self, reference=None, time=None, samples=1, coord_range=None, window=None, scale_exp=None):
        """The distance of this block's state from an exact solution, reduced on the device (analytic.py states the rule and the
        arguments) → ``analytic.ErrorNorms``. ``reference=None``: the test case's own solution at ``time``."""
        from . import analytic
        self.params.wait()
        return analytic.error_norms_state([(self.params, self)], reference, time=time, samples=samples, coord_range=coord_range,
                                          windows=None if window is None else [tuple(window)], scale_exp=scale_exp)

    def fill_exact(self, reference=None, time=None, samples=1, coord_range=None, window=None):
        """Write an exact solution (default: the test case's at ``time``) into rho, u, v, E of this block's real cells."""
        from . import analytic
        self.params.wait()
        return analytic.fill_state([(self.params, self)], reference, time=time, samples=samples, coord_range=coord_range,
                                   windows=None if window is None else [tuple(window)])

    def history_sample(self, gauges=(), scale_exp=None):
        """One sample of the run history of this block's state, reduced on the device (history.py states the rule) →
        ``(history.HistoryRecord, gauge values (gauges, 5))``. ``gauges``: ``(x, y)`` points; ``scale_exp=None``: the default
        scale of this state."""
        from . import history
        self.params.wait()
        return history.sample_state([(self.params, self)], gauges=gauges, scale_exp=scale_exp)

    def real_view(self, a):
        g = self.size.ghosts
        nx, ny = self.size.real_size
        return a.reshape(self.size.size[1], self.size.size[0])[g:g + ny, g:g + nx]

    def memory_required(self):
        """Bytes of device memory the block's vectors take (ref memory_required, src/blocking/block_grid.jl): the 16 of
        ``BlockData`` on the staged path; 7 + 4 ping-pong partners on the fused one (+ any created on first access)."""
        n = self.size.n_cells * np.dtype(self.params.data_type).itemsize
        # (+ the padding of the 8 state vectors that hold the line-pitched intermediate of armon_hip_sweep_pair)
        pad = sum(v.capacity_bytes - v.nbytes for v in list(self.data.values()) + (list(self.alt.values()) if self.alt else []))
        return n * (len(self.data) + (len(self.alt) if self.alt else 0)) + pad


# ---- per-block kernel wrappers -----------------------------------------------------------------

class _KernelSection:
    """Kernel profiling callbacks — ref ``kernel_start``/``kernel_end`` wrapped around every kernel launch
    when profiling is enabled (ref src/generic_kernel.jl:869-876,892-908, src/profiling.jl:6-68).
    ``params.kernel_callbacks`` = list of objects with ``start(name)`` / ``end(name)``."""
    __slots__ = ("cbs", "name")

    def __init__(self, params, name):
        self.cbs = params.kernel_callbacks
        self.name = name

    def __enter__(self):
        for cb in self.cbs:
            cb.start(self.name)

    def __exit__(self, *exc):
        for cb in self.cbs:
            cb.end(self.name)
        return False


def _k(params, name):
    return _KernelSection(params, name)


def _range(params, corners):
    return params.block_size.domain_range(*corners).to_c()


def init_test(params, grid, tune=True):
    """ref src/kernels.jl:176-207 (+ the measured choice of the HBM placement of the vectors, made BEFORE they are
    written; ``tune=False`` to skip it, e.g. when re-initialising a grid that has been placed already)"""
    if tune and grid.placement is None:
        if params.use_fused_sweep:
            grid.tune_placement(keep_state=False)
        else:
            tune_staged_placement(params, grid)
    _init_test_kernel(params, grid)
    if grid.scalar_planes:
        from .problem import init_scalars
        init_scalars(params, grid)
    grid.initialised = True


def tune_staged_placement(params, grid, min_bytes=None):
    """The staged path's counterpart of ``BlockGrid.tune_placement``: the 16 ``BlockData`` vectors have the same size,
    so ANY assignment of the 16 allocations to the 16 fields is a valid layout, and which one is taken moves the staged
    kernels by 5-20 % (advection_second_order 3.25 ... 4.0 ms at 16384², tools/staged_placement_probe.py). Up to 12 random
    assignments — of 16 among the 16 vectors and 8 spares that are freed afterwards — are timed with one staged cycle (X then Y: EOS, boundary conditions, fluxes, cell update, advection,
    projection) on the initial condition, the fastest is kept. ≈40 ms per try, before any timed region."""
    import random
    tries = params.placement_tries
    nbytes = grid.data["rho"].nbytes
    if min_bytes is None:
        min_bytes = params.placement_min_bytes
    # a tile with a remote side (an MPI rank, or a tile of an in-process group: use_MPI is False there and grid.comm is
    # None) cannot run the timing cycle below on its own — its ghost exchange needs the neighbours
    if tries <= 1 or nbytes < min_bytes or params.use_MPI or any(n != PROC_NULL for n in params.neighbours.values()):
        return None
    dev = params.device
    vectors = [grid.data[f] for f in FIELDS]
    free, _total = dev.memory_info()
    try:        # 8 spare vectors widen the choice (freed afterwards): 16 of 24 allocations
        n_spare = int(min(8, (free * 0.5) // max(nbytes, 1)))
        vectors += [dev.empty(vectors[0].n, vectors[0].dtype) for _ in range(max(n_spare, 0))]
    except _lib.SolverException:
        pass
    tries = min(12, params.placement_tries)
    rng = random.Random(0x5EED)
    dx = params.cell_size(0)
    dt = params.T(0.2) * dx
    times, perms = [], []
    callbacks, params.kernel_callbacks = params.kernel_callbacks, []
    for t in range(tries):
        perm = list(range(len(FIELDS))) if t == 0 else rng.sample(range(len(vectors)), len(FIELDS))
        for f, k in zip(FIELDS, perm):
            grid.data[f] = vectors[k]
        _init_test_kernel(params, grid)
        update_EOS(params, grid)
        dev.event_record(1002)
        for axis in (Axis.X, Axis.Y):
            update_EOS(params, grid, axis)
            block_ghost_exchange(params, grid, axis)
            numerical_fluxes(params, grid, axis, dt, params.cell_size(int(axis) - 1))
            cell_update(params, grid, axis, dt, params.cell_size(int(axis) - 1))
            projection_remap(params, grid, axis, dt, params.cell_size(int(axis) - 1))
        dev.event_record(1003)
        times.append(dev.event_elapsed_ms(1002, 1003))
        perms.append(perm)
    params.kernel_callbacks = callbacks
    k = times.index(min(times))
    for f, i in zip(FIELDS, perms[k]):
        grid.data[f] = vectors[i]
    for i, v in enumerate(vectors):
        if i not in perms[k]:
            v.free()
    grid.placement = {"staged": True, "tries": tries, "pool": len(vectors), "cycle_ms": [round(t, 3) for t in times], "chosen": k,
                      "chosen_ms": round(times[k], 3)}
    return grid.placement


def _init_test_kernel(params, grid):
    bs = params.block_size
    full = params.steps_ranges[Axis.X].full_domain
    gpos = (C.c_int64 * 2)(params.N_origin[0] - 1, params.N_origin[1] - 1)
    gN = (C.c_int64 * 2)(*params.global_grid)
    real = C.c_float if params.data_type == np.float32 else C.c_double
    origin = (real * 2)(*params.origin)
    dX = (real * 2)(params.cell_size(0), params.cell_size(1))
    bd = grid.block_data_ptrs()
    check(params.fn("init_test")(params.device.ctx, _range(params, full), params.test.tag,
                                   bs.size[0], bs.size[1], bs.ghosts, C.byref(gpos), C.byref(gN),
                                   C.byref(origin), C.byref(dX), params.test.r, C.byref(bd)))
    if getattr(params.test, "is_problem", False):
        # a user-defined problem (problem.py): init_test above wrote x, y, mask and the zeroed work vectors; rho, u, v, E are
        # overwritten from the problem's regions (armon_hip_init_regions) or arrays
        from .problem import init_state
        init_state(params, grid)


def update_EOS(params, grid, axis=Axis.X):
    """ref src/kernels.jl:151-173"""
    r = _range(params, params.steps_ranges[axis].EOS)
    p = grid.ptr
    if params.test.eos == "bizarrium":
        with _k(params, "bizarrium_EOS"):
            check(params.fn("bizarrium_EOS")(params.device.ctx, r, p("rho"), p("u"), p("v"), p("E"),
                                               p("p"), p("c"), p("g")))
    else:
        with _k(params, "perfect_gas_EOS"):
            check(params.fn("perfect_gas_EOS")(params.device.ctx, r, params.test.gamma, p("rho"), p("E"),
                                                 p("u"), p("v"), p("p"), p("c"), p("g")))


def boundary_conditions(params, grid, axis, side):
    """ref src/halo_exchange.jl:32-36"""
    bs = params.block_size
    uf, vf = params.test.boundary_condition(side)
    domain = bs.border_domain(side).to_c()
    incr = bs.stride_along(axis)
    if side in (Side.Left, Side.Bottom):
        incr = -incr
    p = grid.ptr
    check(params.fn("boundary_conditions")(params.device.ctx, domain, incr, bs.ghosts, uf, vf,
                                             p("rho"), p("u"), p("v"), p("p"), p("c"), p("g"), p("E")))


def periodic_ghosts(params, grid, axis, names, layers=None):
    """``armon_hip_periodic_ghosts`` (the rule in include/armon_hip.h): the ghosts of ``axis`` of the vectors
    ``names`` (at most 8) of ``grid``'s current state take the real cells of the block's opposite border, ``layers`` deep
    (default: all ``nghost``), in one launch on the compute stream."""
    bs = params.block_size
    nx, ny = bs.real_size
    vars_ = (C.c_void_p * len(names))(*[grid.data[f].ptr for f in names])
    with _k(params, "periodic_ghosts"):
        check(params.fn("periodic_ghosts")(params.device.ctx, 0 if axis == Axis.X else 1, bs.size[0], bs.ghosts,
                                           bs.ghosts if layers is None else int(layers), nx, ny, len(names), vars_))


def block_ghost_exchange(params, grid, axis):
    """ref src/halo_exchange.jl:286-368: physical boundary → mirror BC; process boundary → exchange; a periodic axis of a lone
    block → the ghosts of both sides from the opposite border (where the oracle's ``periodic_ghosts`` stands)."""
    remote = [s for s in sides_along(axis) if params.neighbours[s] != PROC_NULL]
    if remote:
        from .halo_exchange import exchange_sides
        exchange_sides(params, grid, axis, remote, COMM_VARS)
    if params.wrap[int(axis) - 1]:
        periodic_ghosts(params, grid, axis, COMM_VARS)
        return
    for side in sides_along(axis):
        if params.neighbours[side] == PROC_NULL:
            boundary_conditions(params, grid, axis, side)


def numerical_fluxes(params, grid, axis, dt, dx):
    """ref src/riemann_schemes.jl:46-52,107-113"""
    r = _range(params, params.steps_ranges[axis].fluxes)
    s = params.block_size.stride_along(axis)
    p = grid.ptr
    ua = p("u") if axis == Axis.X else p("v")
    if params.riemann_scheme == "GAD":
        with _k(params, "acoustic_GAD"):
            check(params.fn("acoustic_GAD")(params.device.ctx, r, s, dt, dx, p("us"), p("ps"), p("rho"), ua,
                                              p("p"), p("c"), LIMITERS[params.riemann_limiter]))
    else:
        with _k(params, "acoustic"):
            check(params.fn("acoustic")(params.device.ctx, r, s, p("us"), p("ps"), p("rho"), ua, p("p"), p("c")))


def cell_update(params, grid, axis, dt, dx):
    """ref src/kernels.jl:217-223"""
    r = _range(params, params.steps_ranges[axis].cell_update)
    s = params.block_size.stride_along(axis)
    p = grid.ptr
    ua = p("u") if axis == Axis.X else p("v")
    with _k(params, "cell_update"):
        check(params.fn("cell_update")(params.device.ctx, r, s, dx, dt, p("us"), p("ps"), p("rho"), ua, p("E")))


def projection_remap(params, grid, axis, dt, dx):
    """ref src/projection_schemes.jl:44-157: advection_fluxes! then euler_projection!"""
    s = params.block_size.stride_along(axis)
    p = grid.ptr
    ra = _range(params, params.steps_ranges[axis].advection)
    w = (p("work_1"), p("work_2"), p("work_3"), p("work_4"))
    if params.projection_scheme == "euler_2nd":
        with _k(params, "advection_second_order"):
            check(params.fn("advection_second_order")(params.device.ctx, ra, s, dx, dt, p("us"), p("rho"),
                                                        p("u"), p("v"), p("E"), *w))
    else:
        with _k(params, "advection_first_order"):
            check(params.fn("advection_first_order")(params.device.ctx, ra, s, dt, p("us"), p("rho"),
                                                       p("u"), p("v"), p("E"), *w))
    rp = _range(params, params.steps_ranges[axis].projection)
    with _k(params, "euler_projection"):
        check(params.fn("euler_projection")(params.device.ctx, rp, s, dx, dt, p("us"), p("rho"), p("u"),
                                              p("v"), p("E"), *w))


def body_force(params, grid, dt):
    """The kick that ends a cycle under a body force (``params.gravity``; DESIGN.md §4.12, the rule in include/armon_hip.h):
    ``armon_hip_body_force`` over the real cells of ``grid``'s current state with the cycle's full step ``dt``, on the compute
    stream. Without a force nothing is launched."""
    if not params.forced:
        return
    r = _range(params, params.steps_ranges[Axis.X].real_domain)
    gx, gy = params.gravity
    p = grid.ptr
    with _k(params, "body_force"):
        check(params.fn("body_force")(params.device.ctx, r, float(dt), gx, gy, p("u") if gx != 0 else None,
                                      p("v") if gy != 0 else None, p("E")))


def diffusion_substeps(params, dt):
    """How many equal explicit steps a cycle of step ``dt`` applies its physical diffusion in:
    ``n = max(1, ceil(float(dt)·2·κ·(1/dx² + 1/dy²)/σ))`` with κ the largest of 4·nu/3, chi and the scalars' D, and σ =
    ``diffusion_number``; each step has the length ``T(dt)/T(n)``. More than ``diffusion_max_substeps`` is an error of the
    category ``time`` that names the three numbers. 0 when nothing diffuses."""
    if not params.diffusive:
        return 0
    dx, dy = float(params.cell_size(0)), float(params.cell_size(1))
    kappa = max(4. * params.viscosity / 3., params.heat_diffusivity, *params.scalar_diffusivities)
    number = float(dt) * 2. * kappa * (1. / (dx * dx) + 1. / (dy * dy))
    n = max(1, math.ceil(number / params.diffusion_number))
    if n > params.diffusion_max_substeps:
        solver_error("time", f"a cycle of step dt = {float(dt)!r} has the diffusion number {number!r}: it needs {n} sub-steps at "
                             f"diffusion_number = {params.diffusion_number!r}, more than diffusion_max_substeps = "
                             f"{params.diffusion_max_substeps}")
    return n


def diffuse_desc(params, grid, dt):
    """The ``armon_diffuse_desc`` of one step of length ``dt`` of ``grid``'s current state and its diffusing planes into their
    ping-pong partners. A state that does not diffuse (nu = chi = 0) is left where it is: its arrays are not given."""
    d = _lib.DiffuseDesc()
    d.nx, d.ny = params.N
    d.nghost = params.nghost
    for k, side in enumerate((Side.Left, Side.Right, Side.Bottom, Side.Top)):          # the ARMON_SIDE_* order
        d.periodic[k] = int(params.wrap[k // 2])
        d.u_factor[k], d.v_factor[k] = params.test.boundary_condition(side)
    d.dt, d.dx, d.dy = float(dt), params.cell_size(0), params.cell_size(1)
    d.nu, d.chi = params.viscosity, params.heat_diffusivity
    d.rho = grid.data["rho"].ptr
    if params.viscosity != 0 or params.heat_diffusivity != 0:
        d.u, d.v, d.E = (grid.data[f].ptr for f in ("u", "v", "E"))
        d.rho_out, d.u_out, d.v_out, d.E_out = (grid.alt[f].ptr for f in STATE_VARS)
    planes = diffusing_planes(params, grid)
    d.ns = len(planes)
    for k, (f, D) in enumerate(planes):
        d.D[k], d.phi[k], d.phi_out[k] = D, grid.data[f].ptr, grid.alt[f].ptr
    return d


def diffusing_planes(params, grid):
    """``(plane, D)`` of the scalars with a diffusivity, in plane order."""
    return [(f, D) for f, D in zip(grid.scalar_planes, params.scalar_diffusivities) if D != 0]


def diffuse(params, grid, dt):
    """The physical diffusion of a cycle of step ``dt`` (``params.viscosity``, ``heat_diffusivity``, the scalars' own;
    DESIGN.md §4.15, the rule in include/armon_hip.h): ``diffusion_substeps`` launches of ``armon_hip_diffuse`` on the compute
    stream, each followed by the swap of what it wrote with its ping-pong partner — the whole set of four state vectors (the
    step copies ρ, so that the two placement-tuned sets stay together) and the diffusing planes. After the cycle's last sweep,
    before the kick of a body force. Without diffusion nothing is launched."""
    if not params.diffusive:
        return
    n = diffusion_substeps(params, dt)
    T = params.T
    step = float(T(dt) / T(n))
    state = params.viscosity != 0 or params.heat_diffusivity != 0
    for _ in range(n):
        d = diffuse_desc(params, grid, step)
        with _k(params, "diffuse"):
            check(params.fn("diffuse")(params.device.ctx, C.byref(d)))
        grid.diffusion_steps += 1
        if state:
            grid.swap_state()
        for f, _D in diffusing_planes(params, grid):
            grid.data[f], grid.alt[f] = grid.alt[f], grid.data[f]


def local_time_step(params, grid):
    """ref src/reductions.jl:89-110 (dx, dy are the GLOBAL cell sizes, :92)"""
    r = _range(params, params.steps_ranges[Axis.X].real_domain)
    dx, dy = params.cell_size(0), params.cell_size(1)
    out = (C.c_float if params.data_type == np.float32 else C.c_double)()
    p = grid.ptr
    with _k(params, "dtCFL"):
        check(params.fn("dtCFL")(params.device.ctx, r, dx, dy, p("u"), p("v"), p("c"), C.byref(out)))
    return out.value


def conservation_vars(params, grid):
    """ref src/reductions.jl:262-323 → (total_mass, total_energy), summed over ranks when use_MPI"""
    r = _range(params, params.steps_ranges[Axis.X].real_domain)
    ds = params.cell_size(0) * params.cell_size(1)
    out = ((C.c_float if params.data_type == np.float32 else C.c_double) * 2)()
    check(params.fn("conservation_vars")(params.device.ctx, r, ds, grid.ptr("rho"), grid.ptr("E"), C.byref(out)))
    mass, energy = out[0], out[1]
    if params.use_MPI:
        from .halo_exchange import allreduce_sum
        mass, energy = allreduce_sum(params, (mass, energy))
    return mass, energy


def global_min(params, local_dt):
    """MPI_Iallreduce(MIN) of ref src/solver_state.jl:107-111, src/utils.jl:126-143"""
    if params.use_MPI:
        from .halo_exchange import allreduce_min
        return allreduce_min(params, local_dt)
    return local_dt


# ---- fused sweep -----------------------------------------------------------------------------------

def sweep_lag(params):
    """Cells a fused sweep reads past the cells it writes: 2 + [GAD] + [euler_2nd]."""
    return 2 + (params.riemann_scheme == "GAD") + (params.projection_scheme == "euler_2nd")


def fused_sweep(params, grid, axis, dt, dx, emit_p=False, emit_c=False, emit_dt=False,
                out_range=None, dt_accumulate=False, swap=True, ctx=None, dt_out=None):
    """One directional sweep as a single kernel launch (armon_hip_sweep). The halo cells of process
    boundaries must already hold the neighbour's (ρ,u,v,E). ``emit_dt``: also reduce the CFL time step
    of the resulting state into ``grid.dt_scalar`` (device) — or into ``dt_out``. ``ctx``: another context of the same
    device to launch on (the tile's edge stream, multi_gpu.hip); such launches are not seen by the kernel callbacks,
    whose events live on the compute stream."""
    d = sweep_desc(params, grid, axis, dt, dx, emit_p, emit_c, emit_dt, out_range, dt_accumulate)
    if emit_dt and dt_out is not None:
        d.dt_cfl_out = dt_out
    if params.wrap[int(axis) - 1]:
        # a lone block's periodic axis: the four vectors the sweep reads get their ghosts first, on the same stream
        periodic_ghosts(params, grid, axis, STATE_VARS)
    if ctx is not None:
        check(params.fn("sweep")(ctx, C.byref(d)))
    else:
        with _k(params, "sweep_x" if axis == Axis.X else "sweep_y"):
            check(params.fn("sweep")(params.device.ctx, C.byref(d)))
        if grid.scalar_planes:
            scalar_sweep(params, grid, axis, d)
    if swap:
        grid.swap_state()


SCALAR_SWEEPS = {"remap": "sweep_scalars", "bounded": "sweep_scalars_bounded"}     # the entry point of a transport rule


def scalar_sweep(params, grid, axis, d):
    """The passive scalars through the sweep ``d`` describes (``armon_hip_sweep_scalars``, DESIGN.md §4.14, or with
    ``scalar_transport="bounded"`` ``armon_hip_sweep_scalars_bounded``, §4.17 — same arguments, same launch): enqueued behind
    ``armon_hip_sweep(d)``, whose input — the pre-sweep state — is still intact, and before ``swap_state``; then the planes'
    own ping-pong partners take their place. On a periodic axis the planes get their ghosts first, like the state."""
    if params.wrap[int(axis) - 1]:
        periodic_ghosts(params, grid, axis, grid.scalar_planes)
    ns = len(grid.scalar_planes)
    phi_in = (C.c_void_p * ns)(*[grid.data[f].ptr for f in grid.scalar_planes])
    phi_out = (C.c_void_p * ns)(*[grid.alt[f].ptr for f in grid.scalar_planes])
    with _k(params, "scalars_x" if axis == Axis.X else "scalars_y"):
        check(params.fn(SCALAR_SWEEPS[params.scalar_transport])(params.device.ctx, C.byref(d), ns, phi_in, phi_out))
    grid.swap_scalars()


def pair_cycle(params, grid):
    """This cycle's X and Y sweeps go through ``armon_hip_sweep_pair``: ``pair_usable``, no kernel callbacks to wrap around
    the single sweeps, and vectors that hold its intermediate (a grid whose vectors were replaced by smaller ones falls back
    to the two plain sweeps)."""
    return (grid.pair_cells is not None and not params.kernel_callbacks and pair_usable(params)
            and min(grid.alt[f].capacity_bytes for f in STATE_VARS) >= grid.pair_cells * np.dtype(params.data_type).itemsize)


def fused_pair(params, grid, d_x, d_y):
    """``armon_hip_sweep_pair``: ``d_x`` sweeps the current state into the alternate vectors, ``d_y`` sweeps it back."""
    mid = min(v.capacity_bytes for v in list(grid.alt.values()) + [grid.data[f] for f in STATE_VARS])
    check(params.fn("sweep_pair")(params.device.ctx, C.byref(d_x), C.byref(d_y), mid))


def sweep_desc(params, grid, axis, dt, dx, emit_p=False, emit_c=False, emit_dt=False, out_range=None,
               dt_accumulate=False):
    """The ``armon_sweep_desc`` of one sweep of ``grid``'s current state into its alternate arrays."""
    d = SweepDesc()
    d.axis = 0 if axis == Axis.X else 1
    d.scheme = SCHEMES[params.riemann_scheme]
    d.limiter = LIMITERS[params.riemann_limiter]
    d.projection = PROJECTIONS[params.projection_scheme]
    d.eos = 1 if params.test.eos == "bizarrium" else 0
    d.nghost = params.nghost
    lo, hi = first_side(axis), last_side(axis)
    # a periodic axis of a lone block: its ghosts hold the opposite border's cells (periodic_ghosts), like a remote side's
    wrapped = params.wrap[int(axis) - 1]
    d.bc_low = int(params.neighbours[lo] == PROC_NULL and not wrapped)
    d.bc_high = int(params.neighbours[hi] == PROC_NULL and not wrapped)
    d.exact = int(params.exact_arithmetic)
    d.x_kernel = int(getattr(params, "x_kernel", 0))
    d.nx, d.ny = params.N
    d.dt, d.dx, d.gamma = dt, dx, params.test.gamma
    d.u_factor_low, d.v_factor_low = params.test.boundary_condition(lo)
    d.u_factor_high, d.v_factor_high = params.test.boundary_condition(hi)
    d.rho_in, d.u_in, d.v_in, d.E_in = (grid.data[f].ptr for f in STATE_VARS)
    d.rho_out, d.u_out, d.v_out, d.E_out = (grid.alt[f].ptr for f in STATE_VARS)
    d.p_out = grid.data["p"].ptr if emit_p else None
    d.c_out = grid.data["c"].ptr if emit_c else None
    if emit_dt:
        d.dt_cfl_out = grid.dt_scalar.ptr
        d.cfl_dx = params.cell_size(0)
        d.cfl_dy = params.cell_size(1)
        d.dt_accumulate = int(dt_accumulate)
    if out_range is not None:
        d.out_lo, d.out_hi = out_range
    return d


def overlapped_sweep(tiles, link, axis, dt, dx, prefetched=None, **emit):
    """One fused sweep of every ``(params, grid)`` of ``tiles`` — this rank's tile, or all tiles of an in-process group — with
    the halo exchange of (ρ,u,v,E) along ``axis`` running while the interiors are computed: post the halos (or take the
    handle ``prefetched`` at the end of the previous cycle), sweep what reads no ghost cell (the cells at least LAG away from
    the remote sides; everything for a tile without one), finish the exchange, sweep the LAG-wide strips next to the remote
    sides, swap (ref src/solver.jl:58-285 gets the same overlap from its async block state machine).
    ``link`` moves the halos: ``start(sides, names)`` → handle or None, ``finish(handle)``, and for the library's groups
    ``edges`` (per tile its transfer stream as a context and its two edge-dt scalars; None for torch's ``HaloExchanger``),
    ``finish_edge(handle)`` and ``edge_join(with_dt)``: unpack and strips then run on each tile's transfer stream, concurrent
    with the interiors. That form needs every tile with a remote side to overlap — a tile too small to have an interior, or
    ``overlap_halo=False``, sweeps after the unpack on its compute stream, so then the whole group takes the in-order form."""
    p0 = tiles[0][0]
    lag = sweep_lag(p0)
    i_ax = int(axis) - 1
    handle = prefetched if prefetched is not None else link.start(sides_along(axis), STATE_VARS)
    late = []
    for k, (p, g) in enumerate(tiles):
        lo_r = p.neighbours[first_side(axis)] != PROC_NULL
        hi_r = p.neighbours[last_side(axis)] != PROC_NULL
        n = p.N[i_ax]
        if not (lo_r or hi_r):
            fused_sweep(p, g, axis, dt, dx, swap=False, **emit)
        elif n < 2 * lag + 1 or not p.overlap_halo:
            late.append((k, p, g, None))
        else:
            lo, hi = (lag if lo_r else 0), (n - lag if hi_r else n)
            fused_sweep(p, g, axis, dt, dx, out_range=(lo, hi), swap=False, **emit)
            late.append((k, p, g, ((0, lo), (hi, n))))
    on_edge = bool(late) and link.edges is not None and p0.edge_stream and all(strips is not None for *_, strips in late)
    if on_edge:
        link.finish_edge(handle)
    else:
        link.finish(handle)
    sz = np.dtype(p0.data_type).itemsize
    for k, p, g, strips in late:
        if strips is None:
            fused_sweep(p, g, axis, dt, dx, swap=False, **emit)
            continue
        for side, rng in enumerate(strips):
            if rng[0] == rng[1]:
                continue
            if on_edge:
                ctx, edge_dt = link.edges[k]
                fused_sweep(p, g, axis, dt, dx, out_range=rng, swap=False, ctx=ctx, dt_out=edge_dt + side * sz, **emit)
            else:
                fused_sweep(p, g, axis, dt, dx, out_range=rng, swap=False, dt_accumulate=True, **emit)
    if on_edge:
        link.edge_join(bool(emit.get("emit_dt")))
    for _, g in tiles:
        g.swap_state()


def rank_sweep(params, grid, axis, dt, dx, **emit):
    """``overlapped_sweep`` of this rank's tile over ``grid.comm``, with the exchange ``prefetch_halo`` may have posted."""
    handle = None
    if grid.halo_prefetch is not None and grid.halo_prefetch[0] == axis:
        handle, grid.halo_prefetch = grid.halo_prefetch[1], None
    else:
        drain_halo(grid)
    overlapped_sweep([(params, grid)], grid.comm, axis, dt, dx, prefetched=handle, **emit)


def prefetch_halo(params, grid):
    """Post the halo exchange of the NEXT cycle's first sweep right after this cycle's last sweep: it depends on
    the state only, not on the next dt, so it travels while the dt reduction is folded, all-reduced and read
    back by the host, and the next cycle's interior sweep can start as soon as its dt is known."""
    if not (params.use_MPI and params.use_fused_sweep) or grid.comm is None or not params.overlap_halo:
        return
    axis = split_axes(params.axis_splitting, grid.global_dt.cycle + 1)[0][0]
    remote = [s for s in sides_along(axis) if params.neighbours[s] != PROC_NULL]
    if not remote or params.N[int(axis) - 1] < 2 * sweep_lag(params) + 1:
        return
    drain_halo(grid)
    grid.halo_prefetch = (axis, grid.comm.start(sides_along(axis), STATE_VARS))


def drain_halo(grid):
    """Complete a prefetched exchange nobody consumed (end of a run, change of plan)."""
    if getattr(grid.comm, "native", False):
        grid.comm.drain()                        # what the library's own cycle posted ahead
    if grid.halo_prefetch is not None:
        grid.comm.finish(grid.halo_prefetch[1])
        grid.halo_prefetch = None


# ---- cycle / time loop ---------------------------------------------------------------------------------

def next_time_step(params, grid):
    """ref src/reductions.jl:164-199 (grid form): CFL step of the current state with the dtCFL kernel, global
    minimum, ``update_dt!``. Synchronous; the fused path only needs it on its first cycle (see below)."""
    gdt = grid.global_dt
    if params.cst_dt:
        return
    gdt.update_dt(global_min(params, local_time_step(params, grid)))


# The reference consumes a cycle's CFL reduction in the NEXT cycle (one-cycle lag of GlobalTimeStep,
# ref src/solver_state.jl:89-99,145-166: the MPI_Iallreduce started by cycle n is waited for by cycle n+1).
# The fused path uses that slack: the last sweep of cycle n-1 reduces L(n), the CFL step of the state cycle n
# starts from; its read-back is only POSTED then (all-reduce on the device scalar, asynchronous copy into a pinned
# slot, event), cycle n's sweeps are launched with the dt already known, and L(n) is picked up afterwards for
# ``update_dt!`` -> cycle n+1. The host never drains the stream: it runs at most one cycle ahead of the GPU.
DT_EVENT_SLOT = 1012       # event-pool slots 1012, 1013: one per parity of the posting cycle


class DtReadback:
    """The deferred read-back of a CFL step: the pinned landing zone (one slot per parity of the posting cycle) and, per
    posting cycle still in flight, the context its event (slot ``DT_EVENT_SLOT`` + parity) was recorded in — the compute
    context of the block, or the transfer stream of tile 0 when the library's own cycle posted it."""

    def __init__(self, params):
        self.params, self.host, self.inflight = params, None, {}

    def landing(self):
        if self.host is None:
            self.host = self.params.device.pinned(2, self.params.data_type)
        return self.host

    def post(self, cycle, scalar):
        """After the last sweep of ``cycle`` reduced the next cycle's L into ``scalar`` (already the global minimum, or
        all-reduced on the host by the taker): asynchronous copy into the slot + event, on the compute stream."""
        dev = self.params.device
        self.landing().copy_from_device_async(scalar, n=1, dst_offset=cycle & 1)
        dev.event_record(DT_EVENT_SLOT + (cycle & 1))
        self.inflight[cycle] = dev.ctx

    def take(self, cycle):
        """The CFL step posted by ``cycle`` (blocks only if the GPU has not got there yet)."""
        check(self.params.device._L.armon_hip_event_sync(self.inflight.pop(cycle), DT_EVENT_SLOT + (cycle & 1)))
        return float(self.host.array[cycle & 1])

    def prime(self, cycle, value):
        """Make ``value`` the CFL step posted by ``cycle``, already landed (a restart, or a checkpoint that took it to store
        it): the pinned slot holds it and the slot's event, recorded now on the compute stream, is what ``take`` waits for."""
        dev = self.params.device
        self.landing().array[cycle & 1] = value
        dev.event_record(DT_EVENT_SLOT + (cycle & 1))
        self.inflight[cycle] = dev.ctx

    def free(self):
        if self.host is not None:
            self.host.free()
            self.host = None


def post_dt_readback(params, grid):
    """After the last sweep of the current cycle (which reduced the next cycle's L into ``grid.dt_scalar``)."""
    if getattr(grid.comm, "stream_ordered", False):
        grid.comm.allreduce_min_device_async(grid.dt_scalar)      # RCCL, in place, ordered on the stream
    grid.dt.post(grid.global_dt.cycle, grid.dt_scalar)


def take_dt_readback(params, grid, posted_in_cycle):
    """Global CFL step posted by ``posted_in_cycle``."""
    local_dt = grid.dt.take(posted_in_cycle)
    if getattr(grid.comm, "stream_ordered", False):
        return local_dt                                           # already the minimum over the ranks
    return global_min(params, local_dt)


def native_cycle_usable(params):
    """The one-call cycle of the library's groups (armon_hip_mgpu_cycle) has two forms of a sweep with remote sides:
    interior + edge stream (overlap), or in order."""
    return params.use_fused_sweep and params.native_cycle and (not params.overlap_halo or params.edge_stream)


def _checkpoint(params, grid, label, axis=Axis.X):
    """ref @checkpoint, src/solver.jl:40-55 → src/io.jl:185-227 (compare / is_ref options)"""
    if not params.compare:
        return False
    from .io import step_checkpoint
    return step_checkpoint(params, grid, label, axis.name)


def solver_cycle(params, grid, last_cycle=True):
    """ref src/solver.jl:288-320 — returns True when a step comparison (``compare``) found a difference.
    ``last_cycle`` (fused path only): materialise p (the reference's saved_vars hold the EOS of the state
    before the last sweep) after this cycle."""
    gdt = grid.global_dt
    deferred = (gdt.cycle - 1) in grid.dt_inflight      # fused path, cycle >= 1: this cycle's dt is already known
    if gdt.cycle == 0:
        if _checkpoint(params, grid, "init_test"):
            return True
        update_EOS(params, grid)
        if _checkpoint(params, grid, "EOS_init"):
            return True
    if not deferred:
        next_time_step(params, grid)
        if params.use_fused_sweep and gdt.cycle == 0:
            grid.release_scratch()               # c, g: only the EOS + dtCFL of cycle 0 needed them
    if _checkpoint(params, grid, "time_step"):
        return True
    if params.use_MPI and getattr(grid.comm, "native", False) and native_cycle_usable(params):
        # the library's own group: exchanges, sweeps and the all-reduce of the next CFL step in ONE call
        # (armon_hip_mgpu_cycle); what is left for the host is the read-back of that scalar, one cycle late
        grid.comm.native_cycle(gdt, last_cycle)
        return False
    sweeps = split_axes(params.axis_splitting, gdt.cycle)
    if params.use_fused_sweep and pair_cycle(params, grid):
        # the cycle is the library's from end to end: X then Y through armon_hip_sweep_pair, the state between them in rows of
        # whole lines; the Y sweep emits what a cycle's last sweep emits below
        dt = gdt.current_dt
        d_x = sweep_desc(params, grid, Axis.X, dt * params.T(sweeps[0][1]), params.cell_size(0))
        grid.swap_state()
        d_y = sweep_desc(params, grid, Axis.Y, dt * params.T(sweeps[1][1]), params.cell_size(1), emit_p=last_cycle,
                         emit_dt=not params.cst_dt)
        grid.swap_state()
        if params.wrap[0]:
            # X-periodic: the X ghosts of the caller's set (the plain pitch), then the pair with the X descriptor's bc_* = 0
            periodic_ghosts(params, grid, Axis.X, STATE_VARS)
        fused_pair(params, grid, d_x, d_y)
        grid.pair_cycles += 1
        if not params.cst_dt:
            post_dt_readback(params, grid)       # (the Y sweep's own CFL step: that of the velocities before diffusion and kick)
        diffuse(params, grid, dt)
        body_force(params, grid, dt)
        if not params.cst_dt:
            if deferred:
                gdt.update_dt(take_dt_readback(params, grid, gdt.cycle - 1))
        return False
    for k, (axis, dt_factor) in enumerate(sweeps):
        # update_solver_state!: ref src/solver_state.jl:339-345
        i_ax = int(axis) - 1
        dx = params.cell_size(i_ax)
        dt = gdt.current_dt * params.T(dt_factor)
        if params.use_fused_sweep:
            # The last sweep of a cycle also reduces the next cycle's CFL step (post-sweep u, v with its
            # own pre-sweep c: what the reference's dtCFL_kernel reads) and, on the final
            # cycle, materialises the pre-sweep p that the reference leaves in memory.
            last = k == len(sweeps) - 1
            sweep = rank_sweep if params.use_MPI else fused_sweep
            sweep(params, grid, axis, dt, dx, emit_p=last and last_cycle, emit_dt=last and not params.cst_dt)
            if last:
                # physical diffusion, then the kick of a body force: after the cycle's last sweep (whose strips, if any, the
                # compute stream has joined), before the halo of the next cycle is packed from the real cells they change.
                # The sweep's emitted CFL step is that of the velocities before either.
                diffuse(params, grid, gdt.current_dt)
                body_force(params, grid, gdt.current_dt)
            if last and not last_cycle:
                prefetch_halo(params, grid)
            if last and not params.cst_dt:
                post_dt_readback(params, grid)
                if deferred:
                    gdt.update_dt(take_dt_readback(params, grid, gdt.cycle - 1))
        else:
            update_EOS(params, grid, axis)
            if _checkpoint(params, grid, "EOS", axis):
                return True
            block_ghost_exchange(params, grid, axis)
            if _checkpoint(params, grid, "boundary_conditions", axis):
                return True
            numerical_fluxes(params, grid, axis, dt, dx)
            if _checkpoint(params, grid, "numerical_fluxes", axis):
                return True
            cell_update(params, grid, axis, dt, dx)
            if _checkpoint(params, grid, "cell_update", axis):
                return True
            projection_remap(params, grid, axis, dt, dx)
            if _checkpoint(params, grid, "projection_remap", axis):
                return True
    if not params.use_fused_sweep:
        body_force(params, grid, gdt.current_dt)     # staged path: the same kick, after the last projection
    return False


# ---- graph replay of the cycle (device-resident time step) ----------------------------------------------------------------
GRAPH_BATCH = 8            # cycles enqueued between two looks at the device state
GRAPH_EVENT_SLOT = 1014    # event-pool slots 1014, 1015


def graph_cycles_usable(params):
    """The cycle can be captured once and replayed when nothing on the host has to happen inside it: one block, fused
    sweeps, no per-cycle output (conservation print-outs, animation frames, step comparisons)."""
    if not (params.use_fused_sweep and params.graph_cycles):
        return False
    if params.checkpoint_step != 0 or params.checkpoint_at_end or params.restart_from is not None:
        return False                    # checkpoints are written, and a restart is primed, between host-driven cycles
    if params.state_compare or params.compare_dir is not None:
        return False                    # and so is a state compared with a reference run's checkpoint
    if params.state_profile:
        return False                    # and a profile taken
    if params.exact_solution:
        return False                    # and error norms taken, or a start from the exact solution
    if params.history_step != 0:
        return False                    # and a history sample enqueued behind a cycle
    if params.state_image:
        return False                    # and an image frame rendered
    if params.state_mixing:
        return False                    # and a mixing sample taken
    if params.forced:
        return False                    # and the kick of a body force enqueued behind every cycle (not part of the captured graph)
    if params.diffusive:
        return False                    # and the diffusion steps enqueued behind every cycle (host-driven only)
    if params.scalar_names:
        return False                    # and the scalar sweep enqueued behind every sweep (host-driven only)
    if params.use_MPI or any(n != PROC_NULL for n in params.neighbours.values()):
        return False
    if any(params.wrap):
        return False                    # and the ghosts of a lone block's periodic axes filled before its sweeps (out of scope)
    if not params.device.owns_ctx:     # a tile context of a group: its stream is the group's, not ours to capture
        return False
    return params.silent > 1 and params.animation_step == 0 and not params.compare and not params.kernel_callbacks


def _graph_sweep_descs(params, grid, cycle_parity, state_ptr):
    """Descriptors of one cycle's sweeps with the time step read from the device state (dt = the split factor)."""
    descs = []
    sweeps = split_axes(params.axis_splitting, cycle_parity)
    for k, (axis, dt_factor) in enumerate(sweeps):
        last = k == len(sweeps) - 1
        d = sweep_desc(params, grid, axis, float(params.T(dt_factor)), params.cell_size(int(axis) - 1),
                       emit_p=last, emit_dt=last and not params.cst_dt)
        d.dt_state = state_ptr
        descs.append(d)
        grid.swap_state()
    return descs


def time_loop_graph(params, grid, _after_handover=None):
    """The time loop with the dt state machine on the device and each cycle replayed from a hipGraph
    (include/armon_hip.h: armon_dt_state, armon_hip_dt_state_step, armon_hip_graph_*). Cycles 0 and 1 run host-driven as
    in ``time_loop`` — cycle 0 needs the staged dtCFL kernel, and everything a capture records must have run once —, then the
    device owns (cycle, time, current_dt): a cycle is ONE host call, the host reads the state back every GRAPH_BATCH
    cycles without stopping the stream. Same bits, same cycle count, same final time as the host-driven loop (tests)."""
    dev, gdt, T = params.device, grid.global_dt, params.T
    gdt.reset()
    grid.dt_inflight.clear()
    params.wait()
    t1 = _time.perf_counter_ns()
    maxtime = T(params.maxtime)

    # host-driven start: cycles 0 and 1 (the second one consumes the first deferred CFL step)
    while gdt.time < maxtime and gdt.cycle < params.maxcycle and gdt.cycle < 2:
        if solver_cycle(params, grid, last_cycle=cycle_ends(params, gdt)):
            break
        gdt.next_cycle()
    n_parities = 1 if params.axis_splitting in ("Sequential", "X_only", "Y_only") else 2
    swaps_per_cycle = len(split_axes(params.axis_splitting, 0))
    if gdt.time < maxtime and gdt.cycle < params.maxcycle:
        # hand the state machine over: the CFL step of the state cycle `gdt.cycle` starts from was posted by the previous one
        L_prev = 0.0
        if not params.cst_dt:
            L_prev = take_dt_readback(params, grid, gdt.cycle - 1)
        # auto_step: the fold of the last sweep's dt reduction steps the state machine itself (one kernel less per cycle);
        # with a constant time step there is no reduction to ride on and the step stays a kernel of its own
        auto = not params.cst_dt
        st = _lib.DtState(current_dt=float(gdt.current_dt), time=float(gdt.time), L_prev=float(L_prev), cycle=gdt.cycle,
                          done=0, invalid=0, emit_p=int(cycle_ends(params, gdt)), auto_step=int(auto), cst_dt=int(params.cst_dt),
                          maxcycle=params.maxcycle, cfl=float(params.cfl), maxtime=float(params.maxtime), Dt=float(params.Dt))
        state = dev.empty(C.sizeof(_lib.DtState) // 8, np.float64)
        host_state = dev.pinned(C.sizeof(_lib.DtState) // 8 * 2, np.float64)
        check(dev._L.armon_hip_memcpy(dev.ctx, C.c_void_p(state.ptr), C.byref(st), C.sizeof(st), 1))
        step = params.fn("dt_state_step")
        L_new = C.c_void_p(grid.dt_scalar.ptr)
        # the step kernel runs once outside any capture, on a state that is already `done` (a no-op)
        dummy = dev.empty(C.sizeof(_lib.DtState) // 8, np.float64)
        over = _lib.DtState(done=1)
        check(dev._L.armon_hip_memcpy(dev.ctx, C.c_void_p(dummy.ptr), C.byref(over), C.sizeof(over), 1))
        check(step(dev.ctx, C.c_void_p(dummy.ptr), L_new, float(params.cfl), float(params.maxtime), params.maxcycle,
                   int(params.cst_dt), float(params.Dt)))
        params.wait()
        dummy.free()

        def enqueue_cycle(parity):
            descs = _graph_sweep_descs(params, grid, parity, state.ptr)
            if pair_cycle(params, grid):          # the same two kernels and the fold, the intermediate in rows of whole lines
                fused_pair(params, grid, *descs)
            else:
                for d in descs:
                    check(params.fn("sweep")(dev.ctx, C.byref(d)))
            if not auto:
                check(step(dev.ctx, C.c_void_p(state.ptr), L_new, float(params.cfl), float(params.maxtime), params.maxcycle,
                           int(params.cst_dt), float(params.Dt)))

        # One graph per cycle parity, and per parity of the ping-pong (a cycle of an odd number of sweeps leaves the state in
        # the other set of vectors): captured lazily, keyed by (parity of the cycle, which set holds the state).
        graphs, origin = {}, grid.data["rho"].ptr

        def launch_cycle(cycle):
            key = (cycle % n_parities, grid.data["rho"].ptr == origin)
            if key not in graphs:
                check(dev._L.armon_hip_graph_begin(dev.ctx))
                held, g = grid.data["rho"].ptr, C.c_void_p()
                try:
                    enqueue_cycle(cycle)
                except BaseException:
                    # leave no capture open, no graph behind and the ping-pong where it was: a caller that catches the
                    # error finds the state it had before this cycle
                    if dev._L.armon_hip_graph_end(dev.ctx, C.byref(g)) == 0 and g:
                        dev._L.armon_hip_graph_destroy(g)
                    if grid.data["rho"].ptr != held:
                        grid.swap_state()
                    raise
                check(dev._L.armon_hip_graph_end(dev.ctx, C.byref(g)))
                graphs[key] = g
                # the capture only recorded the cycle: undo its ping-pong bookkeeping, then replay it for real below
                for _ in range(swaps_per_cycle):
                    grid.swap_state()
            check(dev._L.armon_hip_graph_launch(dev.ctx, graphs[key]))
            for _ in range(swaps_per_cycle):
                grid.swap_state()

        def read_state(slot):
            check(dev._L.armon_hip_memcpy_async(dev.ctx, C.c_void_p(host_state.ptr + slot * C.sizeof(_lib.DtState)),
                                               C.c_void_p(state.ptr), C.sizeof(_lib.DtState), 2))
            dev.event_record(GRAPH_EVENT_SLOT + slot)

        def state_at(slot):
            dev.event_sync(GRAPH_EVENT_SLOT + slot)
            return _lib.DtState.from_buffer_copy(bytes(host_state.array.view(np.uint8)[slot * C.sizeof(_lib.DtState):
                                                                                       (slot + 1) * C.sizeof(_lib.DtState)]))

        # Replay. The host does not know which cycle is the last one: it enqueues batches and looks at the state of the
        # PREVIOUS batch while the current one runs; cycles enqueued past the end are no-ops on the device (`done`), but
        # the ping-pong bookkeeping above assumed they ran, so the final state's set is recomputed from the cycle count.
        if _after_handover is not None:        # test hook: the device owns the time step from here on
            _after_handover(params, grid)
        cycle, batch, final = gdt.cycle, 0, None
        start_cycle, start_in_origin = gdt.cycle, grid.data["rho"].ptr == origin
        try:
            while final is None:
                for _ in range(GRAPH_BATCH):
                    launch_cycle(cycle)
                    cycle += 1
                read_state(batch & 1)
                if batch > 0:
                    prev = state_at((batch - 1) & 1)
                    if prev.done:
                        final = prev
                batch += 1
                if final is None and cycle - start_cycle > params.maxcycle + 2 * GRAPH_BATCH:
                    # every cycle the run could hold has been enqueued and the device still does not say `done`: the state
                    # machine is not stepping (it cannot happen with the kernels as they are; it must not pass for a result)
                    last = state_at((batch - 1) & 1)
                    if not last.done:
                        solver_error("time", f"the device-resident time loop did not finish within maxcycle = {params.maxcycle} "
                                             f"cycles (device state: cycle {last.cycle}, time {last.time}, dt {last.current_dt})")
                    final = last
            last = state_at((batch - 1) & 1)
            final = last if last.done else final
        except BaseException:
            params.wait()                 # no copy into the pinned slots is in flight any more
            host_state.free()
            raise
        finally:
            params.wait()
            for g in graphs.values():
                dev._L.armon_hip_graph_destroy(g)
            state.free()
        if final.invalid:
            host_state.free()
            solver_error("time", f"Invalid time step for cycle {final.invalid_cycle}: {final.invalid_value}")
        # where the state really is: cycles [start_cycle, final.cycle) ran, the later ones were no-ops
        ran = final.cycle - start_cycle
        in_origin = start_in_origin if (ran * swaps_per_cycle) % 2 == 0 else not start_in_origin
        if (grid.data["rho"].ptr == origin) != in_origin:
            grid.swap_state()
        gdt.cycle, gdt.time, gdt.current_dt = int(final.cycle), T(final.time), T(final.current_dt)
        grid.graph_report = {"graphs": len(graphs), "cycles_replayed": int(ran), "cycles_enqueued": cycle - start_cycle}
        host_state.free()
    params.wait()
    return report_run(params, gdt, _time.perf_counter_ns() - t1)


def cycle_ends(params, gdt):
    """Whether the cycle ``gdt`` is about to run ends the run (it then materialises p). With a variable time step the cycle's
    dt is only known after ``next_time_step`` on cycle 0 (``current_dt == 0``): be conservative there."""
    return (gdt.cycle + 1 >= params.maxcycle or (not params.cst_dt and gdt.current_dt == 0)
            or params.T(gdt.time + gdt.current_dt) >= params.T(params.maxtime))


def report_run(params, gdt, solve_time):
    """The run summary of ref src/solver.jl:385-403 → (time, dt, cycles, cells_per_ns, solve_time_ns)."""
    cells = params.N[0] * params.N[1]
    grind_time = solve_time / max(gdt.cycle * cells, 1)
    if params.is_root and params.silent < 3:
        print(" ")
        print(f"Total time:  {solve_time / 1e9:.5f} sec")
        print(f"Grind time:  {grind_time / 1e3:.5f} µs/cell/cycle")
        print(f"Cells/sec:   {1 / grind_time * 1e3:.5f} Mega cells/sec")
        print(f"Cycles:      {gdt.cycle}")
        print(f"Last cycle:  {gdt.time:.18f} sec, Δt={gdt.current_dt:.18f} sec")
    return float(gdt.time), float(gdt.current_dt), gdt.cycle, 1 / grind_time, solve_time


def time_loop(params, grid):
    """ref src/solver.jl:323-403 → (time, dt, cycles, cells_per_ns, solve_time_ns)"""
    if graph_cycles_usable(params):
        return time_loop_graph(params, grid)
    grid.global_dt.reset()
    grid.dt_inflight.clear()
    gdt = grid.global_dt
    if params.restart_from is not None:
        grid.load_state(params.restart_from)
    if params.start_from_exact is not None:
        grid.fill_exact(time=params.start_from_exact, samples=params.error_norms_samples)
        gdt.time = params.T(params.start_from_exact)     # the clock starts where the solution was taken
        if params.check_result or params.silent <= 1:
            params.initial_mass, params.initial_energy = conservation_vars(params, grid)
    params.wait()
    t1 = _time.perf_counter_ns()
    maxtime = params.T(params.maxtime)
    saved_at, save_ns = -1, 0             # checkpoints are disk I/O: their time is taken out of the solve time
    compared_at, stopped = -1, False      # (and so is the time of the comparisons with a reference run's checkpoints)
    grid.state_diffs = []
    profiled_at, grid.profiles = -1, []   # (and the time of the profiles)
    normed_at, grid.error_norms_taken = -1, []   # (and of the error norms)
    imaged_at, grid.images = -1, []       # (and of the image frames)
    mixed_at, grid.mixing_samples = -1, []   # (and of the mixing samples; a restart starts a new series)
    hist, dt_used, grid.history = None, 0.0, None
    if params.history_step != 0:
        from .history import HistoryRun
        hist = HistoryRun(grid, params)   # (the reads of its ring and its file are taken out too: hist.io_ns)
        hist.start(gdt)                   # the row of the initial state, unless the run continues another
    while gdt.time < maxtime and gdt.cycle < params.maxcycle:
        ends = cycle_ends(params, gdt)
        # animation frames (ref :373-378) are written after next_cycle! when (cycle - 1) % animation_step == 0; the fused
        # path only materialises p (a saved var) on request, so a cycle that ends with a frame asks for it like the last one
        frame_due = params.animation_step != 0 and gdt.cycle % params.animation_step == 0
        if solver_cycle(params, grid, last_cycle=ends or frame_due):
            break
        dt_used = float(gdt.current_dt)   # the step this cycle advanced by
        gdt.next_cycle()
        if hist is not None and gdt.cycle % params.history_step == 0:
            hist.sample(gdt, dt_used)     # enqueued behind the cycle: no wait
        if frame_due:
            from .io import write_animation_frame
            params.wait()
            write_animation_frame(params, grid)
        if params.silent <= 1:
            params.wait()
            mass, energy = conservation_vars(params, grid)
            if params.is_root:
                dM = abs(params.initial_mass - mass) / params.initial_mass * 100
                dE = abs(params.initial_energy - energy) / params.initial_energy * 100
                print(f"Cycle {gdt.cycle:4d}: dt = {gdt.current_dt:.18f}, t = {gdt.time:.18f}, "
                      f"|ΔM| = {dM:#8.6g}%, |ΔE| = {dE:#8.6g}%")
        if params.checkpoint_step != 0 and gdt.cycle % params.checkpoint_step == 0:
            from .checkpoint import checkpoint_path
            if hist is not None:
                hist.flush()              # a restart from this checkpoint finds every row up to it in the file
            params.wait()
            t_save = _time.perf_counter_ns()
            grid.save_state(checkpoint_path(params, gdt.cycle))
            save_ns += _time.perf_counter_ns() - t_save
            saved_at = gdt.cycle
        if params.profile_step != 0 and gdt.cycle % params.profile_step == 0:
            from .profile import profile_run
            params.wait()
            t_save = _time.perf_counter_ns()
            profile_run(grid, params, gdt)
            save_ns += _time.perf_counter_ns() - t_save
            profiled_at = gdt.cycle
        if params.mixing_step != 0 and gdt.cycle % params.mixing_step == 0:
            from .mixing import mixing_run
            params.wait()
            t_save = _time.perf_counter_ns()
            mixing_run(grid, params, gdt)
            save_ns += _time.perf_counter_ns() - t_save
            mixed_at = gdt.cycle
        if params.image_step != 0 and gdt.cycle % params.image_step == 0:
            from .derived import image_run
            params.wait()
            t_save = _time.perf_counter_ns()
            image_run(grid, params, gdt)
            save_ns += _time.perf_counter_ns() - t_save
            imaged_at = gdt.cycle
        if params.error_norms_step != 0 and gdt.cycle % params.error_norms_step == 0:
            from .analytic import error_norms_run
            params.wait()
            t_save = _time.perf_counter_ns()
            error_norms_run(grid, params, gdt)
            save_ns += _time.perf_counter_ns() - t_save
            normed_at = gdt.cycle
        if params.compare_step != 0 and gdt.cycle % params.compare_step == 0:
            from .compare import compare_run
            params.wait()
            t_save = _time.perf_counter_ns()
            stopped = compare_run(grid, params, gdt)
            save_ns += _time.perf_counter_ns() - t_save
            compared_at = gdt.cycle
            if stopped:
                break                     # the first difference ends the run (ref @checkpoint, src/solver.jl:40-55)
    drain_halo(grid)
    params.wait()   # "Last fence"
    solve_ns = _time.perf_counter_ns() - t1 - save_ns - (hist.io_ns if hist is not None else 0)
    if hist is not None:
        hist.finish(gdt, dt_used)
    if params.checkpoint_at_end and saved_at != gdt.cycle:
        from .checkpoint import checkpoint_path
        grid.save_state(checkpoint_path(params, gdt.cycle))
    if params.profile_at_end and profiled_at != gdt.cycle:
        from .profile import profile_run
        profile_run(grid, params, gdt)
    if params.mixing_at_end and mixed_at != gdt.cycle:
        from .mixing import mixing_run
        mixing_run(grid, params, gdt)
    if params.image_at_end and imaged_at != gdt.cycle:
        from .derived import image_run
        image_run(grid, params, gdt)
    if params.error_norms_at_end and normed_at != gdt.cycle:
        from .analytic import error_norms_run
        error_norms_run(grid, params, gdt)
    if params.compare_at_end and compared_at != gdt.cycle and not stopped:
        from .compare import compare_run
        compare_run(grid, params, gdt)
    return report_run(params, gdt, solve_ns)


def armon(params):
    """ref src/solver.jl:411-516 — main entry point, returns SolverStats."""
    if params.is_root and params.silent < 3:
        print(params)
    if params.animation_step != 0:
        from .io import prepare_animation_dir
        prepare_animation_dir(params)
    grid = BlockGrid(params)
    if params.use_MPI:
        from .halo_exchange import setup
        setup(params, grid)
    init_test(params, grid)
    if params.check_result or params.silent <= 1:
        params.initial_mass, params.initial_energy = conservation_vars(params, grid)
    final_time, dt, cycles, cells_per_ns, solve_time = time_loop(params, grid)
    if params.check_result and params.test.conservative:
        mass, energy = conservation_vars(params, grid)
        if params.is_root:
            dM = abs(params.initial_mass - mass)
            dE = abs(params.initial_energy - energy)
            if not (dM <= 1e-12 and dE <= 1e-12):   # ref src/solver.jl:484-501 (comparison_tolerance)
                solver_error("check", f"mass or energy are not conserved: |ΔM| = {dM}, |ΔE| = {dE}")
    if params.write_output:
        from .io import write_sub_domain_file
        write_sub_domain_file(params, grid, params.output_file, coarse=params.output_coarsen is not None)
    if params.write_slices:
        from .io import write_slices_files
        write_slices_files(params, grid, params.output_file)
    stats = SolverStats(final_time, dt, cycles, solve_time / 1e9, params.N[0] * params.N[1], cells_per_ns)
    stats.state_diffs = list(grid.state_diffs)
    stats.profiles = list(grid.profiles)
    stats.error_norms = list(grid.error_norms_taken)
    stats.history = grid.history
    stats.images = list(grid.images)
    stats.mixing = list(grid.mixing_samples)
    stats.scalars = tuple(params.scalar_names)
    stats.scalar_transport = params.scalar_transport
    stats.diffusion_steps = grid.diffusion_steps
    if params.return_data:
        stats.data = grid
    return stats
