"""``ArmonParameters`` — the reference's configuration surface (ref src/parameters.jl) for the HIP backend.

Same keyword names, defaults and validation as ``ArmonParameters(; kwargs...)``: every ``init_*`` step
consumes its own options and anything left over is an error (ref src/parameters.jl:349-372). Options
that only steer the reference's CPU machinery (threads, NUMA, cache blocking, logging) are accepted and
recorded so that a reference script runs unchanged, but have no effect on the device path.
"""
import numbers

import numpy as np

from ._lib import solver_error
from .blocking import Axis, BlockSize, Side, compute_steps_ranges
from .test_cases import default_domain_origin, default_domain_size

SCHEMES = {"Godunov": 0, "GAD": 1}                       # ref src/riemann_schemes.jl:5-6
SCHEME_STENCIL = {"Godunov": 1, "GAD": 2}                # ref :17-18
PROJECTIONS = {"euler": 0, "euler_2nd": 1}               # ref src/projection_schemes.jl:4-5
PROJECTION_STENCIL = {"euler": 1, "euler_2nd": 2}        # ref :11-12
LIMITERS = {"no_limiter": 0, "minmod": 1, "superbee": 2}  # ref src/limiters.jl:10-12
SPLITTINGS = ("Sequential", "Godunov", "SequentialSym", "Strang", "X_only", "Y_only")  # ref src/axis_splitting.jl:7-12

PROC_NULL = -1


class ArmonParameters:
    def __init__(self, *, data_type=np.float64, N=(10, 10), **options):
        self.data_type = np.dtype(data_type)
        if self.data_type not in (np.dtype(np.float64), np.dtype(np.float32)):
            solver_error("config", f"unsupported data_type {data_type}: Float64 or Float32")
        self.T = self.data_type.type          # scalar constructor: host-side arithmetic is done in T, like the reference
        self.suffix = "_f32" if self.data_type == np.float32 else ""
        if len(N) != 2:
            solver_error("config", "only 2-D domains are supported")
        self.N = tuple(int(n) for n in N)
        options = self._get_device(**options)
        options = self._init_scheme(**options)
        options = self._init_test(**options)
        options = self._init_MPI(**options)
        options = self._init_device(**options)
        options = self._init_profiling(**options)
        options = self._init_indexing(**options)
        options = self._init_output(**options)
        options = self._init_backend(**options)
        if options:   # ref src/parameters.jl:369-372
            names = ", ".join(f"'{k}'" for k in options)
            raise ValueError(f"{len(options)} unconsumed options:\n{names}")

    # ref src/parameters.jl:392-405 — this backend IS the device: use_gpu defaults to True here
    def _get_device(self, device="HIP_native", use_gpu=True, use_kokkos=False, **options):
        if use_kokkos:
            solver_error("config", "use_kokkos is not available in the HIP backend")
        if not use_gpu:
            solver_error("config", "the HIP backend has no CPU path (use_gpu=false)")
        if str(device) not in ("HIP_native", "ROCM"):
            solver_error("config", f"Unknown device: '{device}' (this backend provides :HIP_native)")
        self.device_name = str(device)
        self.use_gpu = True
        self.use_kokkos = False
        return options

    # ref src/parameters.jl:577-630
    def _init_scheme(self, scheme="GAD", projection="euler_2nd", riemann_limiter="minmod",
                     axis_splitting="Sequential", nghost=4, cst_dt=False, Dt=0.,
                     dt_on_even_cycles=False, **options):
        scheme, projection = str(scheme), str(projection)
        riemann_limiter, axis_splitting = str(riemann_limiter), str(axis_splitting)
        if projection not in PROJECTIONS:
            solver_error("config", f"Unknown scheme: '{projection}'")
        if scheme not in SCHEMES:
            solver_error("config", f"Unknown scheme: '{scheme}'")
        if axis_splitting not in SPLITTINGS:
            solver_error("config", f"Unknown splitting method: '{axis_splitting}'")
        if riemann_limiter not in LIMITERS:
            solver_error("config", f"Unknown limiter name: '{riemann_limiter}'")
        # The reference asks for stencil(scheme)·stencil(projection) ghosts (ref src/parameters.jl:609-613),
        # but its own step ranges (ref :1005-1014) compute fluxes up to interface N+w+1, whose stencil
        # reads cell N+w+stencil(scheme): with fewer than w+stencil(scheme) ghost layers that read leaves
        # the block (undefined behaviour under @inbounds in the reference, a memory fault on a GPU).
        # Both rules agree for the default GAD + euler_2nd (4); the stricter one is enforced here.
        min_nghost = max(SCHEME_STENCIL[scheme] * PROJECTION_STENCIL[projection],
                         SCHEME_STENCIL[scheme] + PROJECTION_STENCIL[projection])
        if nghost < min_nghost:
            solver_error("config", "Not enough ghost cells for the riemann solver and projection, "
                                   f"at least {min_nghost} are needed, got {nghost}")
        if cst_dt and Dt == 0:
            solver_error("config", "Dt == 0 with constant step enabled")
        if dt_on_even_cycles:
            # ref src/reductions.jl:165-170 skips update_dt! on odd cycles, after which next_cycle!
            # (ref src/solver_state.jl:158-161) rejects the Ready state: unusable in the sync solver.
            solver_error("config", "dt_on_even_cycles is not supported by the synchronous solver cycle")
        self.nghost = int(nghost)
        self.riemann_scheme = scheme
        self.projection_scheme = projection
        self.riemann_limiter = riemann_limiter
        self.axis_splitting = axis_splitting
        self.cst_dt = bool(cst_dt)
        self.Dt = float(Dt)
        self.dt_on_even_cycles = False
        return options

    # ref src/parameters.jl:632-670
    def _init_test(self, test="Sod", domain_size=None, origin=None, cfl=0., maxtime=0.,
                   maxcycle=500_000, gravity=None, scalars=None, viscosity=None, heat_diffusivity=None, diffusion_number=0.5,
                   diffusion_max_substeps=64, scalar_transport=None, **options):
        """``test``: the name of a built-in case, or a ``problem.Problem`` — a user-defined initial state, gamma, EOS and
        boundary types — which is bound here to the run's data type and cell size (``Problem.bind``).
        ``gravity=(gx, gy)``: a uniform body force, applied on the device as a kick at the end of every cycle (DESIGN.md
        §4.12); it overrides a problem's own, as ``domain_size`` and ``cfl`` do, and works with a built-in case too. The
        values are rounded to the data type; ``params.test.gravity`` holds what the device receives.
        ``scalars``: a list of ``problem.Scalar`` (or a dict name → ``(NY, NX)`` array) — passive fields carried through the
        fused sweeps, added after a problem's own; at most 4 in all. ``params.scalars`` holds them bound
        to the data type, ``params.scalar_names`` their names in plane order.
        ``viscosity=nu``, ``heat_diffusivity=chi``: physical diffusion (the rule in include/armon_hip.h) — a
        constant kinematic shear viscosity and a constant diffusivity of the specific internal energy, both >= 0, applied on
        the device after the cycle's last sweep and before the kick of a body force; they override a problem's own, as
        ``gravity`` does, and a scalar diffuses with its own ``Scalar(..., diffusivity=D)``. ``params.diffusive`` says whether
        anything diffuses. A cycle of step dt applies ``solver.diffusion_substeps(params, dt)`` equal explicit steps:
        ``diffusion_number`` = sigma in (0, 1] bounds dt·2·kappa·(1/dx² + 1/dy²) of one of them (kappa the largest of 4 nu / 3,
        chi and the D), and more than ``diffusion_max_substeps`` of them in a cycle is an error of the category ``time``.
        ``scalar_transport``: ``"remap"`` (the default: φ is remapped as ρ·φ and divided by the new ρ) or
        ``"bounded"`` (φ is transported per unit mass and stays within the range of its own values); it
        overrides a problem's own, as ``viscosity`` does. ``"bounded"`` needs at least one scalar. The bound covers the
        transport: a diffusing scalar diffuses after the sweeps as before."""
        from .problem import Problem, bind_case, check_scalar_transport
        problem = test if isinstance(test, Problem) else None
        name = str(test)
        if domain_size is None:
            domain_size = problem.domain_size if problem is not None else default_domain_size(name)
        self.domain_size = tuple(float(d) for d in domain_size)
        if origin is None:
            origin = problem.origin if problem is not None else default_domain_origin(name)
        self.origin = tuple(float(o) for o in origin)
        T = self.T
        dX = (T(self.domain_size[0]) / T(self.N[0]), T(self.domain_size[1]) / T(self.N[1]))
        if problem is not None:
            self.test = problem.bind(dX, T, self.N, gravity=gravity, scalars=scalars, viscosity=viscosity,
                                     heat_diffusivity=heat_diffusivity)
        else:
            self.test = bind_case(name, dX, T, gravity=(0., 0.) if gravity is None else gravity, scalars=scalars,
                                  global_grid=self.N, viscosity=viscosity, heat_diffusivity=heat_diffusivity)
        self.scalars = tuple(self.test.scalars)
        self.scalar_names = tuple(sc.name for sc in self.scalars)
        if scalar_transport is None:
            scalar_transport = problem.scalar_transport if problem is not None else "remap"
        self.scalar_transport = check_scalar_transport(scalar_transport)
        if self.scalar_transport != "remap" and not self.scalars:
            solver_error("config", f"scalar_transport = {self.scalar_transport!r} needs at least one passive scalar (scalars=...)")
        self.gravity = self.test.gravity
        self.forced = self.gravity != (0., 0.)
        self.viscosity, self.heat_diffusivity = self.test.viscosity, self.test.heat_diffusivity
        self.scalar_diffusivities = tuple(sc.diffusivity for sc in self.scalars)
        self.diffusive = self.viscosity != 0 or self.heat_diffusivity != 0 or any(D != 0 for D in self.scalar_diffusivities)
        if isinstance(diffusion_number, (bool, np.bool_)) or not isinstance(diffusion_number, (numbers.Real, np.floating)) \
                or not 0 < diffusion_number <= 1:
            solver_error("config", f"diffusion_number must be a number in (0, 1], got {diffusion_number!r}")
        self.diffusion_number = float(diffusion_number)
        if isinstance(diffusion_max_substeps, (bool, np.bool_)) or not isinstance(diffusion_max_substeps, (numbers.Integral, np.integer)) \
                or diffusion_max_substeps < 1:
            solver_error("config", f"diffusion_max_substeps must be an integer >= 1, got {diffusion_max_substeps!r}")
        self.diffusion_max_substeps = int(diffusion_max_substeps)
        self.maxcycle = int(maxcycle)
        self.cfl = float(cfl) if cfl != 0 else self.test.cfl
        self.maxtime = float(maxtime) if maxtime != 0 else self.test.maxtime
        return options

    # ref src/parameters.jl:408-467. The MPI transport is replaced by torch.distributed (RCCL on GPUs,
    # gloo in CPU tests): `use_MPI=True` needs an initialised process group, `global_comm` may carry a
    # torch ProcessGroup. Default is False here because a single process owns a single GPU.
    def _init_MPI(self, use_MPI=False, P=(1, 1), reorder_grid=True, global_comm=None, gpu_aware=True,
                  tile_of=None, periodic=None, **options):
        """``tile_of=(rank, (px, py))``: this parameter set describes ONE tile of a px×py grid whose tiles all live in
        this process (``multi_tile.TileGroup`` over ``armon_hip_mgpu_init``): same partition and neighbours as an MPI
        rank of the reference, no process group involved. ``periodic=(x, y)``: the domain is periodic along that axis
        (the reference's domain never is, ref src/parameters.jl:432). A problem with ``"Periodic"`` sides
        sets it; given with a built-in case it overrides the case's sides on that axis. On one block the ghosts of a
        periodic axis are filled from the block's own opposite border (``armon_hip_periodic_ghosts``; ``wrap`` records the
        axes, the neighbours stay ``PROC_NULL``); in a tile group or a native rank the neighbours wrap around along that
        axis (``armon_hip_mgpu_set_periodic``), so a tile can be its own neighbour; only the library's native exchange
        supports it."""
        if tile_of is not None:
            P = tile_of[1]
        self.periodic = resolve_periodic(self.test, periodic)
        if len(P) != len(self.N):
            solver_error("config", f"Mismatched dimensions: expected a grid of {len(self.N)} processes, got: {len(P)}")
        self.use_MPI = bool(use_MPI)
        self.reorder_grid = reorder_grid
        self.gpu_aware = gpu_aware
        self.global_comm = global_comm
        if self.use_MPI and getattr(self.test, "arrays", None) is not None:
            solver_error("config", "Problem.from_arrays is not supported for ranks of a process group (use_MPI=true): "
                                   "one block or an in-process tile group only")
        if self.use_MPI:
            import torch.distributed as dist
            if not dist.is_initialized():
                solver_error("config", "'use_MPI=true' but the process group has not yet been initialized")
            self.rank = dist.get_rank(global_comm)
            self.proc_size = dist.get_world_size(global_comm)
            self.proc_dims = tuple(int(p) for p in P)
            if self.proc_dims[0] * self.proc_dims[1] != self.proc_size:
                solver_error("config", f"could not create a {P[0]}×{P[1]} cartesian topology "
                                       f"using {self.proc_size} processes")
            self.cart_coords = cart_coords(self.rank, self.proc_dims)
            self.neighbours = cart_neighbours(self.cart_coords, self.proc_dims, self.periodic)
        elif tile_of is not None:
            self.proc_dims = tuple(int(p) for p in P)
            self.rank = int(tile_of[0])
            self.proc_size = self.proc_dims[0] * self.proc_dims[1]
            if not 0 <= self.rank < self.proc_size:
                solver_error("config", f"tile {self.rank} is not part of a {P[0]}×{P[1]} grid")
            self.cart_coords = cart_coords(self.rank, self.proc_dims)
            self.neighbours = cart_neighbours(self.cart_coords, self.proc_dims, self.periodic)
        else:
            self.rank = 0
            self.proc_size = 1
            self.proc_dims = (1, 1)
            self.cart_coords = (0, 0)
            self.neighbours = {s: PROC_NULL for s in Side}
        # the axes along which this block is its own neighbour: a lone block's periodic axes (a tile's or a rank's periodic
        # sides have a neighbour in the topology instead)
        lone = not self.use_MPI and tile_of is None
        self.wrap = self.periodic if lone else (False, False)
        self.root_rank = 0
        self.is_root = self.rank == self.root_rank
        return options

    # ref src/parameters.jl:470-530 — CPU machinery knobs: accepted, inert on the device path.
    def _init_device(self, use_threading=True, use_simd=True, block_size=None, use_cache_blocking=False,
                     async_cycle=False, use_two_step_reduction=False, workload_distribution="simple",
                     distrib_params=None, numa_aware=False, lock_memory=False, busy_wait_limit=100,
                     **options):
        if use_cache_blocking:
            # ref src/blocking/block_grid.jl:352-355: without cache blocking the grid is one block.
            solver_error("config", "use_cache_blocking is a CPU cache optimisation; the HIP backend keeps one block per GPU")
        if async_cycle:
            solver_error("config", "async_cycle (CPU thread state machine) is replaced by HIP streams here")
        self.use_threading, self.use_simd = use_threading, use_simd
        self.use_cache_blocking, self.async_cycle = False, False
        # ref src/reductions.jl:70-78,276-284: "two steps" = per-cell values into a temporary array, then a plain reduce of
        # it, for GPU backends whose one-step mapreduce misbehaves. Every reduction of this backend already IS two-step
        # (one partial per workgroup, then a fold kernel; reductions.hip) and deterministic, so both settings select the
        # same, compliant behaviour: the option is satisfied, not dropped.
        self.use_two_step_reduction = bool(use_two_step_reduction)
        self.kernel_block_size = block_size
        return options

    # ref src/parameters.jl:532-575
    def _init_profiling(self, profiling=(), measure_time=True, time_async=True, log_blocks=False,
                        estimated_blk_log_size=0, **options):
        self.profiling = tuple(profiling)
        self.kernel_callbacks = []      # ref register_kernel_callback, src/profiling.jl:30-68
        self.measure_time = measure_time
        self.time_async = time_async
        return options

    # ref src/parameters.jl:673-697
    def _init_indexing(self, **options):
        self.global_grid = self.N
        P, cc, g = self.proc_dims, self.cart_coords, self.global_grid
        self.N = tuple(g[d] // P[d] + (g[d] % P[d] if cc[d] == P[d] - 1 else 0) for d in range(2))
        if any(P[d] > 1 and self.N[d] < self.nghost for d in range(2)):
            solver_error("config", f"domain {g} is too small to be split by {P} processes while keeping "
                                   f"more than {self.nghost} cells along each axis")
        self.N_origin = tuple(cc[d] * (g[d] // P[d]) + 1 for d in range(2))
        self.block_size = BlockSize((self.N[0] + 2 * self.nghost, self.N[1] + 2 * self.nghost), self.nghost)
        w = PROJECTION_STENCIL[self.projection_scheme]
        self.steps_ranges = {ax: compute_steps_ranges(ax, self.nghost, w) for ax in (Axis.X, Axis.Y)}
        return options

    # ref src/parameters.jl:700-748
    def _init_output(self, silent=0, output_dir=".", output_file="output", write_output=False,
                     write_ghosts=False, write_slices=False, output_precision=None, animation_step=0,
                     compare=False, is_ref=False, comparison_tolerance=1e-10, check_result=False,
                     return_data=False, checkpoint_step=0, checkpoint_file="checkpoint", checkpoint_at_end=False,
                     restart_from=None, compare_step=0, compare_dir=None, compare_file="checkpoint", compare_at_end=False,
                     comparison_atol=0.0, comparison_time_atol=0.0, profile_step=0, profile_kind="x", profile_bins=None,
                     profile_width=1, profile_centre=None, profile_dr=None, profile_file="profile", profile_at_end=False,
                     error_norms_step=0, error_norms_at_end=False, error_norms_samples=1, error_norms_file="error_norms",
                     start_from_exact=None, history_step=0, history_file="history", history_gauges=(), history_capacity=256,
                     history_scale_exp=None, image_step=0, image_at_end=False, image_quantity="grad_rho", image_reduce=None,
                     image_coarsen=None, image_transfer=None, image_range=None, image_file="image", checkpoint_compress=False,
                     mixing_step=0, mixing_at_end=False, mixing_axis="y", mixing_bin_width=1, mixing_scalars=None,
                     mixing_pdf_bins=0, mixing_pdf_range=(0., 1.), mixing_file="mixing", **options):
        """``checkpoint_step=k``: a checkpoint every k completed cycles (0 = off) as
        ``<output_dir>/<checkpoint_file>_<cycle:06d>.ckpt``; ``checkpoint_at_end``: one when the run stops;
        ``restart_from=path``: continue the run of that file, bit for bit (checkpoint.py; no reference counterpart);
        ``checkpoint_compress``: checkpoints are written packed — file version 2, every band of every plane encoded on the
        device with a lossless codec (csrc/plane_codec.hip) — instead of as dense planes; reading takes either.
        ``compare_step=k``: after every k completed cycles (0 = off) the state is compared on the device with
        ``<compare_dir>/<compare_file>_<cycle:06d>.ckpt`` — the checkpoints of a reference run — within ``comparison_tolerance``
        (relative) and ``comparison_atol`` (a number, or a dict plane → number); the file's time is compared with the run's
        within ``comparison_tolerance`` and ``comparison_time_atol``; ``compare_at_end``: with the file of the final cycle;
        the first difference is reported and stops the run (compare.py; the text ``compare`` / ``is_ref`` path is untouched by
        these).
        ``profile_step=k``: after every k completed cycles (0 = off) the exact profile of the state (profile.py) along
        ``profile_kind`` = ``"x" | "y" | "r"`` is written to ``<output_dir>/<profile_file>_<cycle:06d>.txt``;
        ``profile_bins``, ``profile_width``, ``profile_centre``, ``profile_dr``: the arguments of ``profile.profile_state``
        (None = its defaults); ``profile_at_end``: one when the run stops.
        ``error_norms_step=k``: after every k completed cycles (0 = off) the state's distance from the exact solution of the
        test case at the run's time (analytic.py) is written to ``<output_dir>/<error_norms_file>_<cycle:06d>.txt`` and listed
        in ``SolverStats.error_norms``; ``error_norms_samples``: 1, 2 or 4 points per cell and axis for the cell means of the
        solution; ``error_norms_at_end``: one when the run stops. ``start_from_exact=t0``: the state is filled with the exact
        solution at ``t0 > 0`` and the clock starts there, so that a convergence study skips the start-up error of the jump.
        ``history_step=k``: the run history (history.py) — a row of exact global sums, extrema with their cells and gauge
        values for the initial state, after every k completed cycles (0 = off) and for the cycle the run stops at, in
        ``<output_dir>/<history_file>.txt`` and in ``SolverStats.history``; a single block enqueues each sample behind its
        cycle and never waits for it. ``history_gauges=[(x, y), ...]``: at most 64 points inside the domain whose cell's rho, u,
        v, E, p are recorded with every row; ``history_capacity``: the slots of the device-resident ring, read back when it is
        full (1 .. 65536); ``history_scale_exp``: six exponents instead of the default scale (``history.default_scale``). With
        ``restart_from`` an existing file whose header matches keeps its rows up to the checkpoint's cycle and is appended
        to. None of ``history_file``, ``history_gauges``, ``history_capacity``, ``history_scale_exp`` has an effect while
        ``history_step`` is 0, but each is checked.
        ``image_step=k``: after every k completed cycles (0 = off) a greyscale PNG frame of each derived field of
        ``image_quantity`` (a name of ``derived.QUANTITIES`` or a list of them), computed and reduced on the device
        (derived.py), is written to ``<output_dir>/<image_file>_<quantity>_<cycle:06d>.png`` and listed in
        ``SolverStats.images``; ``image_at_end``: one when the run stops. ``image_reduce``: ``"mean" | "max" | "min"`` or a
        dict quantity → name (None: max for ``grad_rho``, mean otherwise); ``image_coarsen``: the factor ``f | (fx, fy)``
        (None: ``output_coarsen`` if set, else the smallest power of two that brings the longer side to at most 2048
        pixels); ``image_transfer``: ``"linear" | "log" | "schlieren"`` or a dict quantity → name (None: schlieren for
        ``grad_rho``, linear otherwise); ``image_range=(lo, hi)``: the values of black and white (None: the frame's own
        finite minimum and maximum).
        ``mixing_step=k``: after every k completed cycles (0 = off) the mixing measures of the run's passive scalars
        (mixing.py) — per scalar the exact profile of rho, φ, φ², ρφ, ρφ² along ``mixing_axis`` = ``"x" | "y"`` in bins of
        ``mixing_bin_width`` cells, and with ``mixing_pdf_bins`` > 0 the histogram of φ over ``mixing_pdf_range = (lo, hi)``
        with the mass of every bin — are written to ``<output_dir>/<mixing_file>_<cycle:06d>.txt``, their whole-record
        measures (content, min, max, integral width, mixedness, extents) to one line of the time series
        ``<output_dir>/<mixing_file>.txt``, and listed in ``SolverStats.mixing``; ``mixing_scalars``: the names to take
        (None = all); ``mixing_at_end``: one sample when the run stops. A restart starts a new series. One block only."""
        self.compare, self.is_ref = bool(compare), bool(is_ref)
        if isinstance(checkpoint_step, bool) or not isinstance(checkpoint_step, (numbers.Integral, np.integer)) or checkpoint_step < 0:
            solver_error("config", f"checkpoint_step must be an integer >= 0, got {checkpoint_step!r}")
        self.checkpoint_step = int(checkpoint_step)
        self.checkpoint_file = str(checkpoint_file)
        if not self.checkpoint_file or "/" in self.checkpoint_file:
            solver_error("config", f"checkpoint_file is a file name inside output_dir, got {checkpoint_file!r}")
        self.checkpoint_at_end = bool(checkpoint_at_end)
        if not isinstance(checkpoint_compress, (bool, np.bool_)):
            solver_error("config", f"checkpoint_compress must be true or false, got {checkpoint_compress!r}")
        self.checkpoint_compress = bool(checkpoint_compress)
        self.restart_from = None if restart_from is None else str(restart_from)
        if self.restart_from is not None and (self.compare or self.is_ref):
            solver_error("config", "restart_from cannot be combined with compare / is_ref: the step files of a reference "
                                   "run start at cycle 0")
        if self.use_MPI and (self.checkpoint_step or self.checkpoint_at_end or self.restart_from is not None):
            solver_error("config", "checkpoint / restart is not supported for ranks of a process group (use_MPI=true): "
                                   "one block or an in-process tile group only")
        self.comparison_tolerance = float(comparison_tolerance)
        if isinstance(compare_step, bool) or not isinstance(compare_step, (numbers.Integral, np.integer)) or compare_step < 0:
            solver_error("config", f"compare_step must be an integer >= 0, got {compare_step!r}")
        self.compare_step = int(compare_step)
        self.compare_dir = None if compare_dir is None else str(compare_dir)
        self.compare_file = str(compare_file)
        if not self.compare_file or "/" in self.compare_file:
            solver_error("config", f"compare_file is a file name inside compare_dir, got {compare_file!r}")
        self.compare_at_end = bool(compare_at_end)
        atols = list(comparison_atol.values()) if isinstance(comparison_atol, dict) else [comparison_atol]
        if not all(isinstance(v, (numbers.Real, np.floating)) and not isinstance(v, bool) and v >= 0 for v in atols):
            solver_error("config", f"comparison_atol must be a number >= 0 (or a dict plane -> number), got {comparison_atol!r}")
        self.comparison_atol = ({str(k): float(v) for k, v in comparison_atol.items()} if isinstance(comparison_atol, dict)
                                else float(comparison_atol))
        if isinstance(comparison_time_atol, bool) or not isinstance(comparison_time_atol, (numbers.Real, np.floating)) \
                or not comparison_time_atol >= 0:
            solver_error("config", f"comparison_time_atol must be a number >= 0, got {comparison_time_atol!r}")
        self.comparison_time_atol = float(comparison_time_atol)
        self.state_compare = self.compare_step != 0 or self.compare_at_end      # any comparison with checkpoints during the run
        if (self.state_compare or self.compare_dir is not None) and (self.compare or self.is_ref):
            solver_error("config", "compare_step / compare_at_end / compare_dir cannot be combined with compare / is_ref: "
                                   "one compares with checkpoints on the device, the other with text files per sub-step")
        if (self.state_compare or self.compare_dir is not None) and self.use_MPI:
            solver_error("config", "compare_step / compare_at_end are not supported for ranks of a process group (use_MPI=true): "
                                   "one block or an in-process tile group only")
        if self.state_compare and self.compare_dir is None:
            solver_error("config", "compare_step / compare_at_end need compare_dir: the directory of the reference run's checkpoints")
        if isinstance(profile_step, bool) or not isinstance(profile_step, (numbers.Integral, np.integer)) or profile_step < 0:
            solver_error("config", f"profile_step must be an integer >= 0, got {profile_step!r}")
        self.profile_step = int(profile_step)
        self.profile_at_end = bool(profile_at_end)
        self.profile_kind = str(profile_kind)
        if self.profile_kind not in ("x", "y", "r"):
            solver_error("config", f"unknown profile_kind {profile_kind!r}: 'x', 'y' or 'r'")
        if isinstance(profile_width, bool) or not isinstance(profile_width, (numbers.Integral, np.integer)) or profile_width < 1:
            solver_error("config", f"profile_width must be an integer >= 1, got {profile_width!r}")
        self.profile_width = int(profile_width)
        if profile_bins is not None and (isinstance(profile_bins, bool) or not isinstance(profile_bins, (numbers.Integral, np.integer))
                                         or profile_bins < 1):
            solver_error("config", f"profile_bins must be an integer >= 1, got {profile_bins!r}")
        self.profile_bins = None if profile_bins is None else int(profile_bins)
        if profile_dr is not None and (isinstance(profile_dr, bool) or not isinstance(profile_dr, (numbers.Real, np.floating))
                                       or not (0 < profile_dr < float("inf"))):
            solver_error("config", f"profile_dr must be a finite number > 0, got {profile_dr!r}")
        self.profile_dr = None if profile_dr is None else float(profile_dr)
        if profile_centre is not None and (len(profile_centre) != 2 or not all(np.isfinite(float(c)) for c in profile_centre)):
            solver_error("config", f"profile_centre takes two finite coordinates, got {profile_centre!r}")
        self.profile_centre = None if profile_centre is None else tuple(float(c) for c in profile_centre)
        self.profile_file = str(profile_file)
        if not self.profile_file or "/" in self.profile_file:
            solver_error("config", f"profile_file is a file name inside output_dir, got {profile_file!r}")
        self.state_profile = self.profile_step != 0 or self.profile_at_end      # any profile taken during the run
        if self.state_profile and self.use_MPI:
            solver_error("config", "profile_step / profile_at_end are not supported for ranks of a process group (use_MPI=true): "
                                   "one block or an in-process tile group only")
        if isinstance(mixing_step, bool) or not isinstance(mixing_step, (numbers.Integral, np.integer)) or mixing_step < 0:
            solver_error("config", f"mixing_step must be an integer >= 0, got {mixing_step!r}")
        self.mixing_step = int(mixing_step)
        if not isinstance(mixing_at_end, (bool, np.bool_)):
            solver_error("config", f"mixing_at_end must be True or False, got {mixing_at_end!r}")
        self.mixing_at_end = bool(mixing_at_end)
        if mixing_axis not in ("x", "y"):
            solver_error("config", f"unknown mixing_axis {mixing_axis!r}: 'x' or 'y'")
        self.mixing_axis = str(mixing_axis)
        if isinstance(mixing_bin_width, bool) or not isinstance(mixing_bin_width, (numbers.Integral, np.integer)) or mixing_bin_width < 1:
            solver_error("config", f"mixing_bin_width must be an integer >= 1, got {mixing_bin_width!r}")
        self.mixing_bin_width = int(mixing_bin_width)
        if isinstance(mixing_pdf_bins, bool) or not isinstance(mixing_pdf_bins, (numbers.Integral, np.integer)) \
                or not 0 <= mixing_pdf_bins <= 1024:
            solver_error("config", f"mixing_pdf_bins must be an integer in [0, 1024], got {mixing_pdf_bins!r}")
        self.mixing_pdf_bins = int(mixing_pdf_bins)
        try:
            good = len(mixing_pdf_range) == 2 and not any(isinstance(c, bool) for c in mixing_pdf_range) and \
                all(np.isfinite(float(c)) for c in mixing_pdf_range) and float(mixing_pdf_range[0]) < float(mixing_pdf_range[1])
        except (TypeError, ValueError):
            good = False
        if not good:
            solver_error("config", f"mixing_pdf_range takes two finite values lo < hi, got {mixing_pdf_range!r}")
        self.mixing_pdf_range = (float(mixing_pdf_range[0]), float(mixing_pdf_range[1]))
        if not isinstance(mixing_file, str) or not mixing_file or "/" in mixing_file:
            solver_error("config", f"mixing_file is a file name inside output_dir, got {mixing_file!r}")
        self.mixing_file = mixing_file
        if mixing_scalars is not None:
            if isinstance(mixing_scalars, str) or not all(isinstance(s, str) for s in mixing_scalars) or len(mixing_scalars) == 0 \
                    or len(set(mixing_scalars)) != len(tuple(mixing_scalars)):
                solver_error("config", f"mixing_scalars takes a list of distinct scalar names (None for all), got {mixing_scalars!r}")
            for s in mixing_scalars:
                if s not in self.scalar_names:
                    solver_error("config", f"mixing_scalars: no scalar {s!r}: this run carries {self.scalar_names}")
        self.mixing_scalars = None if mixing_scalars is None else tuple(mixing_scalars)
        self.state_mixing = self.mixing_step != 0 or self.mixing_at_end         # any mixing sample taken during the run
        if self.state_mixing and not self.scalar_names:
            solver_error("config", "mixing_step / mixing_at_end need passive scalars: this run carries none")
        if self.state_mixing and self.use_MPI:
            solver_error("config", "mixing_step / mixing_at_end are not supported for ranks of a process group (use_MPI=true): "
                                   "one block only")
        if isinstance(error_norms_step, bool) or not isinstance(error_norms_step, (numbers.Integral, np.integer)) or error_norms_step < 0:
            solver_error("config", f"error_norms_step must be an integer >= 0, got {error_norms_step!r}")
        self.error_norms_step = int(error_norms_step)
        self.error_norms_at_end = bool(error_norms_at_end)
        if isinstance(error_norms_samples, bool) or error_norms_samples not in (1, 2, 4):
            solver_error("config", f"error_norms_samples must be 1, 2 or 4, got {error_norms_samples!r}")
        self.error_norms_samples = int(error_norms_samples)
        self.error_norms_file = str(error_norms_file)
        if not self.error_norms_file or "/" in self.error_norms_file:
            solver_error("config", f"error_norms_file is a file name inside output_dir, got {error_norms_file!r}")
        if start_from_exact is not None and (isinstance(start_from_exact, bool) or not isinstance(start_from_exact, (numbers.Real, np.floating))
                                             or not (0 < start_from_exact < float("inf"))):
            solver_error("config", f"start_from_exact must be a finite time > 0, got {start_from_exact!r}")
        self.start_from_exact = None if start_from_exact is None else float(start_from_exact)
        self.state_error_norms = self.error_norms_step != 0 or self.error_norms_at_end     # any error norms taken during the run
        self.exact_solution = self.state_error_norms or self.start_from_exact is not None
        if self.exact_solution and self.use_MPI:
            solver_error("config", "error_norms_step / error_norms_at_end / start_from_exact are not supported for ranks of a process "
                                   "group (use_MPI=true): one block or an in-process tile group only")
        if self.start_from_exact is not None and (self.compare or self.is_ref):
            solver_error("config", "start_from_exact cannot be combined with compare / is_ref: the step files of a reference run "
                                   "start from the initial state at cycle 0")
        if self.start_from_exact is not None and self.restart_from is not None:
            solver_error("config", "start_from_exact cannot be combined with restart_from: both set the initial state and the clock")
        if self.exact_solution:
            from .analytic import has_closed_form
            if not has_closed_form(self.test, self.periodic):
                solver_error("config", f"error_norms_step / error_norms_at_end / start_from_exact need a test case with an exact "
                                       f"solution: {self.test.name} has no closed form")
        if isinstance(history_step, bool) or not isinstance(history_step, (numbers.Integral, np.integer)) or history_step < 0:
            solver_error("config", f"history_step must be an integer >= 0, got {history_step!r}")
        self.history_step = int(history_step)
        self.history_file = str(history_file)
        if not self.history_file or "/" in self.history_file:
            solver_error("config", f"history_file is a file name inside output_dir, got {history_file!r}")
        if isinstance(history_capacity, bool) or not isinstance(history_capacity, (numbers.Integral, np.integer)) \
                or not 1 <= history_capacity <= 65536:
            solver_error("config", f"history_capacity must be an integer in [1, 65536], got {history_capacity!r}")
        self.history_capacity = int(history_capacity)
        from . import history as _history
        try:
            points = [tuple(pt) for pt in history_gauges]
            good = all(len(pt) == 2 and not any(isinstance(c, bool) for c in pt) and all(np.isfinite(float(c)) for c in pt) for pt in points)
        except (TypeError, ValueError):
            good = False
        if not good:
            solver_error("config", f"history_gauges takes a list of (x, y) points, got {history_gauges!r}")
        if len(points) > _history.MAX_GAUGES:
            solver_error("config", f"history_gauges: {len(points)} points, at most {_history.MAX_GAUGES}")
        self.history_gauges = tuple((float(x), float(y)) for x, y in points)
        _history.gauge_cells(self, self.history_gauges)         # a point outside the domain is refused here, not in the run
        self.history_scale_exp = None if history_scale_exp is None else _history.check_scale(history_scale_exp)
        if self.history_step != 0 and self.use_MPI:
            solver_error("config", "history_step is not supported for ranks of a process group (use_MPI=true): "
                                   "one block or an in-process tile group only")
        from . import derived as _derived
        if isinstance(image_step, bool) or not isinstance(image_step, (numbers.Integral, np.integer)) or image_step < 0:
            solver_error("config", f"image_step must be an integer >= 0, got {image_step!r}")
        self.image_step = int(image_step)
        if not isinstance(image_at_end, (bool, np.bool_)):
            solver_error("config", f"image_at_end must be True or False, got {image_at_end!r}")
        self.image_at_end = bool(image_at_end)
        if not isinstance(image_quantity, (str, tuple, list)) or not all(isinstance(q, str) for q in image_quantity):
            solver_error("config", f"image_quantity takes a name or a list of names of {_derived.QUANTITIES}, got {image_quantity!r}")
        if image_reduce is not None and not isinstance(image_reduce, (str, dict)):
            solver_error("config", f"image_reduce takes a name of {_derived.REDUCTIONS} or a dict quantity -> name, got {image_reduce!r}")
        names = (image_quantity,) if isinstance(image_quantity, str) else tuple(image_quantity)
        default_reduce = {q: "max" if q == "grad_rho" else "mean" for q in names}
        if isinstance(image_reduce, dict):
            image_reduce = {**{q: m for q, m in default_reduce.items() if q not in image_reduce}, **image_reduce}
        self.image_quantity, modes = _derived.normalize_request(names, default_reduce if image_reduce is None else image_reduce,
                                                                scalars=self.scalar_names)
        self.image_reduce = dict(zip(self.image_quantity, modes))
        if image_transfer is None:
            image_transfer = {}
        elif isinstance(image_transfer, str):
            image_transfer = {q: image_transfer for q in self.image_quantity}
        elif not isinstance(image_transfer, dict):
            solver_error("config", f"image_transfer takes a name of {_derived.TRANSFERS} or a dict quantity -> name, got {image_transfer!r}")
        for q, t in image_transfer.items():
            if q not in self.image_quantity or t not in _derived.TRANSFERS:
                solver_error("config", f"image_transfer: {q!r} -> {t!r}: a quantity of image_quantity and one of {_derived.TRANSFERS}")
        self.image_transfer = {q: image_transfer.get(q, "schlieren" if q == "grad_rho" else "linear") for q in self.image_quantity}
        if image_range is not None:
            try:
                good = len(image_range) == 2 and not any(isinstance(c, bool) for c in image_range) and \
                    all(np.isfinite(float(c)) for c in image_range) and float(image_range[0]) < float(image_range[1])
            except (TypeError, ValueError):
                good = False
            if not good:
                solver_error("config", f"image_range takes two finite values lo < hi, got {image_range!r}")
        self.image_range = None if image_range is None else (float(image_range[0]), float(image_range[1]))
        self._image_coarsen = None if image_coarsen is None else normalize_coarsen_factor(image_coarsen)
        if image_coarsen is not None and self._image_coarsen is None:
            solver_error("config", f"image_coarsen takes factors >= 1 (None for the default), got {image_coarsen!r}")
        if not isinstance(image_file, str) or not image_file or "/" in image_file:
            solver_error("config", f"image_file is a file name inside output_dir, got {image_file!r}")
        self.image_file = image_file
        self.state_image = self.image_step != 0 or self.image_at_end        # any frame taken during the run
        if self.state_image and self.use_MPI:
            solver_error("config", "image_step / image_at_end are not supported for ranks of a process group (use_MPI=true): "
                                   "one block or an in-process tile group only")
        self.silent = silent
        self.output_dir, self.output_file = output_dir, output_file
        self.write_output, self.write_ghosts = write_output, write_ghosts
        self.write_slices = bool(write_slices)          # 3 more files at the end of armon(): io.write_slices_files
        self.animation_step = int(animation_step)       # a frame every `animation_step` cycles: solver.time_loop
        if self.animation_step < 0:
            solver_error("config", f"animation_step must be >= 0, got {animation_step}")
        self.output_precision = 17 if output_precision is None else int(output_precision)
        self.check_result = check_result
        self.return_data = return_data
        self.initial_mass = 0.
        self.initial_energy = 0.
        return options

    # ref src/parameters.jl:766-778 — backend specific options (like ext/ArmonKokkos.jl:83-87)
    def _init_backend(self, device_id=None, use_fused_sweep=True, exact_arithmetic=False, stream=None,
                      placement_tries=24, stream_ordered_halo=True, ctx=None, native_halo=True, overlap_halo=True, edge_stream=True,
                      placement_min_bytes=256 << 20, placement_rounds=8, graph_cycles=False, native_cycle=True,
                      output_coarsen=0, **options):
        """``device_id``: GPU ordinal (default LOCAL_RANK or 0). ``use_fused_sweep``: run each sweep as
        the fused HIP kernel instead of the 5 staged kernels. ``exact_arithmetic=True``: IEEE division/sqrt
        and no FMA contraction in the fused sweep — bit-identical to the staged path and to the CPU oracle, every bit,
        subnormal values included (quotients that can fall below the normal range take the IEEE expansion; the
        unguarded form of rounds 1-3, one subnormal unit off in 1 run of 800, is the build flag -DARMON_LOOSE_SUBNORMAL);
        the default tuned arithmetic (shared 1-ulp reciprocals, FMAs) stays within the reference's own
        golden-file tolerance (atol 1e-13, rtol 4 eps on the Sod family). ``placement_tries``: how many
        placements of the state vectors in HBM ``init_test`` may try (0/1 = take the first; see
        ``BlockGrid.tune_placement``). ``output_coarsen=0 | f | (fx, fy)``: in-situ reduced output — ``write_output`` and
        the animation frames write the state block-averaged on the device by these factors (``BlockGrid.coarsen``,
        ``io.write_coarse_file``) instead of every cell; 0 = the full grid, as the reference does."""
        import os
        self.output_coarsen = normalize_coarsen_factor(output_coarsen)
        if self.output_coarsen is not None:
            if self.write_ghosts:
                solver_error("config", "output_coarsen averages real cells only: it cannot be combined with write_ghosts")
            check_coarsen_alignment(self, self.output_coarsen)
        # the factor of the image frames (image_coarsen, consumed by _init_output): its default needs output_coarsen
        from .derived import default_image_factor
        self.image_factor = self._image_coarsen or self.output_coarsen or default_image_factor(self.global_grid)
        if self.state_image:
            check_coarsen_alignment(self, self.image_factor)
        if device_id is None:
            device_id = int(os.environ.get("LOCAL_RANK", "0")) if self.use_MPI else 0
        self.device_id = int(device_id)
        self._stream = stream
        self._ctx = ctx         # an existing armon_ctx to adopt (a tile context owned by an armon_mgpu group)
        self.native_halo = bool(native_halo)    # N>1 over RCCL: halo exchange / dt all-reduce by the library itself
        self.overlap_halo = bool(overlap_halo)  # sweep the interior while the halos travel
        self.edge_stream = bool(edge_stream)    # native groups: unpack + boundary strips on the transfer stream, concurrent with the interior
        self._device = None     # created on first use, so that configuration errors need no GPU
        # per-step dumps / comparisons need the intermediate states: only the staged path has them
        self.use_fused_sweep = bool(use_fused_sweep) and not self.compare
        if self.scalars and not self.use_fused_sweep:
            solver_error("config", "passive scalars are carried by the fused sweeps only: use_fused_sweep=False (the staged path, "
                                   "which compare / is_ref select too) cannot be combined with scalars")
        if self.scalars and self.use_MPI:
            solver_error("config", "passive scalars are not supported for ranks of a process group (use_MPI=true): one block only")
        if self.diffusive and not self.use_fused_sweep:
            solver_error("config", "physical diffusion (viscosity, heat_diffusivity, a scalar's diffusivity) runs behind the fused "
                                   "sweeps only: use_fused_sweep=False (the staged path, which compare / is_ref select too) cannot "
                                   "be combined with it")
        if self.diffusive and self.use_MPI:
            solver_error("config", "physical diffusion is not supported for ranks of a process group (use_MPI=true): one block only")
        self.exact_arithmetic = bool(exact_arithmetic)
        self.placement_tries = int(placement_tries)
        self.placement_min_bytes = int(placement_min_bytes)     # vectors smaller than this are not worth placing
        self.placement_rounds = int(placement_rounds)           # batches of spares a search may go through
        # dt state machine on the device + each cycle replayed from a hipGraph (solver.time_loop_graph): one host call per
        # cycle instead of one per kernel plus a scalar read-back — what small grids are bound by
        self.graph_cycles = bool(graph_cycles)
        # tile groups / RCCL ranks: a whole cycle (exchanges, sweeps, dt minimum) enqueued by ONE library call
        # (armon_hip_mgpu_cycle) instead of call by call from this host mirror
        self.native_cycle = bool(native_cycle)
        self.stream_ordered_halo = bool(stream_ordered_halo)   # RCCL: order the exchange on the stream, no host syncs
        self.shared_stream = False
        self.backend_options = dict(device_id=device_id, use_fused_sweep=self.use_fused_sweep,
                                    exact_arithmetic=self.exact_arithmetic)
        return options

    # ---- hooks ---------------------------------------------------------------------------------
    @property
    def device(self):
        """``create_device(Val(:HIP_native))`` (ref src/parameters.jl:751-755): context on first use."""
        if self._device is None:
            from .device import HIPDevice
            if self._ctx is not None:
                self._device = HIPDevice.adopt(self._ctx, self.device_id)
                return self._device
            stream = self._stream
            if stream is None and self.use_MPI and self.stream_ordered_halo:
                stream = self._torch_stream_for_rccl()
            self._device = HIPDevice(self.device_id, stream)
        return self._device

    def _torch_stream_for_rccl(self):
        """With the RCCL backend every kernel of this rank runs on ONE torch stream (made current): torch's
        point-to-point ops then order themselves after the pack kernels and the unpack kernels after the
        receives on the device, and the halo exchange needs no host synchronisation at all."""
        try:
            import torch
            import torch.distributed as dist
            if not (dist.is_initialized() and dist.get_backend(self.global_comm) == "nccl"):
                return None
            torch.cuda.set_device(self.device_id)
            self._torch_stream = torch.cuda.Stream(device=self.device_id)
            torch.cuda.set_stream(self._torch_stream)
            self.shared_stream = True
            return self._torch_stream.cuda_stream
        except ImportError:
            return None

    def fn(self, name):
        """The C-ABI entry point ``armon_hip_<name>`` for this run's data_type (``_f32`` suffix for Float32)."""
        from . import _lib
        L = self._device._L if self._device is not None else _lib.lib()      # the library this run's context came from
        return getattr(L, "armon_hip_" + name + self.suffix)

    def cell_size(self, i_ax):
        """Global cell size along an axis, computed in T (ref src/solver_state.jl:341, src/reductions.jl:92)."""
        return self.T(self.domain_size[i_ax]) / self.T(self.global_grid[i_ax])

    def wait(self):
        """``Base.wait(params)`` (ref src/parameters.jl:1031-1038)."""
        self.device.wait()

    def device_memory_info(self):
        return self.device.memory_info()

    def data_type_size(self):
        return self.data_type.itemsize

    def __repr__(self):   # ref print_parameters, src/parameters.jl:805-918 (abridged)
        return (f"ArmonParameters(test={self.test.name}, N={self.N} of {self.global_grid}, "
                f"scheme={self.riemann_scheme}, limiter={self.riemann_limiter}, "
                f"projection={self.projection_scheme}, splitting={self.axis_splitting}, "
                f"nghost={self.nghost}, cfl={self.cfl}, maxtime={self.maxtime}, maxcycle={self.maxcycle}, "
                f"P={self.proc_dims}, coords={self.cart_coords}, device_id={self.device_id})")


def resolve_periodic(test, periodic=None):
    """The periodic axes ``(x, y)`` of a run: ``test`` — a built-in case's name, a ``Problem`` or a bound one — gives its own
    through ``"Periodic"`` sides (both sides of an axis together); ``periodic=None`` takes them. An explicit ``periodic``
    overrides the sides of a test that has no periodic side of its own (a built-in case, a problem with walls or free flow);
    against a problem that has some it must say the same, anything else is a configuration error."""
    from .boundaries import periodic_axes
    from .test_cases import _known
    boundaries = _known(test)["boundaries"] if isinstance(test, str) else test.boundaries
    own = periodic_axes(boundaries)
    if periodic is None:
        return own
    try:
        px, py = periodic
        good = all(isinstance(v, (bool, np.bool_)) or v in (0, 1) for v in (px, py))
    except (TypeError, ValueError):
        good = False
    if not good:
        solver_error("config", f"periodic takes two booleans (x, y), got {periodic!r}")
    given = (bool(px), bool(py))
    if any(own) and given != own:
        solver_error("config", f"periodic = {given} contradicts the problem's boundaries {tuple(boundaries)}, which are "
                               f"periodic along (x, y) = {own}")
    return given


def cart_coords(rank, dims):
    """MPI_Cart_coords for a non-periodic row-major grid (last dimension varies fastest)."""
    return (rank // dims[1], rank % dims[1])


def cart_rank(coords, dims, periodic=(False, False)):
    coords = tuple(c % dims[d] if periodic[d] else c for d, c in enumerate(coords))
    if not all(0 <= coords[d] < dims[d] for d in range(2)):
        return PROC_NULL
    return coords[0] * dims[1] + coords[1]


def cart_neighbours(coords, dims, periodic=(False, False)):
    """ref src/parameters.jl:441-447 (MPI.Cart_shift along dim 0 = X, dim 1 = Y); ``periodic``: the axes along which the grid wraps
    around, see ``_init_MPI``."""
    cx, cy = coords
    return {
        Side.Left: cart_rank((cx - 1, cy), dims, periodic),
        Side.Right: cart_rank((cx + 1, cy), dims, periodic),
        Side.Bottom: cart_rank((cx, cy - 1), dims, periodic),
        Side.Top: cart_rank((cx, cy + 1), dims, periodic),
    }


def normalize_coarsen_factor(factor):
    """``0 | f | (fx, fy)`` -> ``None`` (no coarsening) or a pair of integers >= 1; anything else is a configuration error."""
    def integer(f):
        if isinstance(f, bool) or not isinstance(f, (numbers.Integral, np.integer)):
            solver_error("config", f"coarsening factors must be integers, got {f!r}")
        return int(f)

    if isinstance(factor, (tuple, list)):
        if len(factor) != 2:
            solver_error("config", f"a coarsening factor is an integer or a pair (fx, fy), got {factor!r}")
        fx, fy = integer(factor[0]), integer(factor[1])
        if fx < 1 or fy < 1:
            solver_error("config", f"coarsening factors must be >= 1 along both axes, got {factor!r}")
        return fx, fy
    f = integer(factor)
    if f < 0:
        solver_error("config", f"coarsening factors must be >= 1 (or 0 for none), got {f}")
    return None if f == 0 else (f, f)


def coarse_shape(N, factor):
    """``(cnx, cny) = (ceil(nx / fx), ceil(ny / fy))``: the coarse grid of an nx x ny block (the last coarse row / column
    is partial when the factor does not divide the grid)."""
    fx, fy = factor
    return (-(-int(N[0]) // fx), -(-int(N[1]) // fy))


def check_coarsen_alignment(params, factor):
    """Coarse cells are defined on the GLOBAL grid: a tile can only coarsen its own cells when its first real cell starts a
    coarse cell along both axes, (N_origin - 1) % f == 0."""
    for d, name in enumerate("xy"):
        if (params.N_origin[d] - 1) % factor[d] != 0:
            solver_error("config", f"coarsening factor {factor[d]} along {name} does not respect the tile boundaries: tile "
                                   f"{params.cart_coords} of {params.proc_dims} starts at global cell {params.N_origin[d] - 1}, "
                                   "which is not a multiple of the factor (coarse cells may not straddle tiles)")


def memory_required(N, nghost=4, data_type=np.float64, fused=True, transient=False):
    """Device bytes for one block (ref ``memory_required``, src/blocking/block_grid.jl): the 16 ``BlockData`` vectors on the
    staged path; on the fused path the 7 it touches (x, y, rho, u, v, E, p) + 4 ping-pong partners of the state — the
    other nine (us, ps, work_1..4, mask; c, g after the first cycle) are only allocated when something reads them.
    ``transient=True``: the peak instead — + c, g during cycle 0, or the 8 spare vectors of the placement search of
    ``init_test`` (blocks whose vectors reach 256 MiB), whichever is larger."""
    n = (N[0] + 2 * nghost) * (N[1] + 2 * nghost) * np.dtype(data_type).itemsize
    if not fused:
        return n * 16
    spares = 8 if n >= (256 << 20) else 2
    return n * (11 + (spares if transient else 0))


def proc_grid_for(world):
    """Process grid used by the benchmarks: 1→(1,1), 2→(2,1), 4→(2,2), 8→(4,2) (BASELINE.json configs);
    otherwise the most square px ≥ py factorisation."""
    py = int(world ** 0.5)
    while world % py:
        py -= 1
    return (world // py, py)
