"""Body forces on the GPU (csrc/body_force.hip): the kick against its numpy restatement
(tests/body_force_restated.py), forced runs against the CPU — the oracle's sweeps (tests/sweep_reference.py) alternated with the
restated kick —, and everything the project guarantees with the force switched on: tiles, restarts, the graph fallback.

"Equals" always means bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import body_force_restated as BF
from sweep_reference import rand_state, reference_sweep

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
DTYPES = ("float64", "float32")
N = (24, 20)
FORCE = (0.7, -1.3)


def A():
    import armon_amd
    return armon_amd


@pytest.fixture(scope="module")
def dev():
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------
WINDOWS = [(5, 3), (64, 1), (130, 7), (3, 70000)]            # (3, 70000): more rows than a launch grid's y extent
G_VALUE = 9.81


def real_range(nx, ny, g):
    from armon_amd._lib import Range
    row = nx + 2 * g
    return Range(g * row + g, row, ny, 0, nx)


def call_kick(dev, dtype, r, dt, gx, gy, u, v, E):
    real = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    fn = getattr(dev._L, "armon_hip_body_force" + ("_f32" if np.dtype(dtype) == np.float32 else ""))
    ptr = lambda a: None if a is None else C.c_void_p(a.ptr)
    return fn(dev.ctx, r, real(dt), real(gx), real(gy), ptr(u), ptr(v), ptr(E))


@functools.lru_cache(maxsize=None)
def planted_state(nx, ny, g, dtype):
    """A random state over the whole ghosted block with -0.0 planted in u, v and E: in real cells and in ghost cells."""
    f = rand_state(nx, ny, g, "perfect_gas", dtype, 1000 * nx + ny + g)
    T = np.dtype(dtype).type
    row = nx + 2 * g
    for k in ("u", "v", "E"):
        a = f[k]
        a[0] = a[row * g + g] = a[row * (g + ny - 1) + g + nx - 1] = a[row * g + g - 1] = a[-1] = T(-0.)
        a.setflags(write=False)
    return f


@pytest.mark.parametrize("g", [2, 5])
@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: f"{w[0]}x{w[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_kick_is_the_restatement_bit_for_bit(dev, dtype, window, g):
    nx, ny = window
    T = np.dtype(dtype).type
    f = planted_state(nx, ny, g, dtype)
    r = real_range(nx, ny, g)
    dt = float(T(0.0123))
    d = {k: dev.empty(f[k].size, dtype) for k in ("u", "v", "E")}
    try:
        for gx, gy in ((G_VALUE, 0.), (0., G_VALUE), (G_VALUE, -G_VALUE), (0., 0.), (-0., 0.)):
            for k in d:
                d[k].copy_from_host(f[k])
            assert call_kick(dev, dtype, r, dt, gx, gy, d["u"], d["v"], d["E"]) == 0, dev._L.armon_hip_last_error()
            dev.wait()
            got = {k: d[k].to_host() for k in d}
            want = {k: f[k].copy() for k in d}
            BF.kick_real(want, nx, ny, g, dt, gx, gy)
            for k in d:
                assert same_bits(got[k], want[k]), (k, gx, gy, int((bits(got[k]) != bits(want[k])).sum()))
            # what must keep its bits, against the ORIGINAL: every ghost cell, and every cell of a zero component's plane
            sy, sx = ny + 2 * g, nx + 2 * g
            ghost = np.ones((sy, sx), dtype=bool)
            ghost[g:g + ny, g:g + nx] = False
            for k, moved in (("u", gx != 0), ("v", gy != 0), ("E", gx != 0 or gy != 0)):
                keep = ghost.ravel() if moved else np.ones(sy * sx, dtype=bool)
                assert np.array_equal(bits(got[k])[keep], bits(f[k])[keep]), (k, gx, gy)
                assert np.signbit(got[k][0]) and np.signbit(got[k][-1]) and got[k][0] == 0        # the planted -0.0 of a ghost
                if moved:
                    real = ~ghost.ravel()
                    assert (bits(got[k])[real] != bits(f[k])[real]).mean() > 0.9, (k, gx, gy)    # and it did move the rest
        # a plane that is not touched may be NULL
        d["v"].copy_from_host(f["v"])
        d["E"].copy_from_host(f["E"])
        assert call_kick(dev, dtype, r, dt, 0., G_VALUE, None, d["v"], d["E"]) == 0
        assert call_kick(dev, dtype, r, dt, 0., 0., None, None, None) == 0
        dev.wait()
    finally:
        for a in d.values():
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_kick_refuses_before_any_launch(dev, dtype):
    nx, ny, g = 5, 3, 2
    f = planted_state(nx, ny, g, dtype)
    r = real_range(nx, ny, g)
    d = {k: dev.from_host(f[k]) for k in ("u", "v", "E")}
    err = lambda: dev._L.armon_hip_last_error().decode()
    try:
        for bad in (float("nan"), float("inf"), -float("inf")):
            for pos, name in enumerate(("dt", "gx", "gy")):
                args = [0.01, 1., 1.]
                args[pos] = bad
                assert call_kick(dev, dtype, r, *args, d["u"], d["v"], d["E"]) != 0
                assert name in err().split(), err()
        for (gx, gy), missing in (((1., 0.), "u"), ((0., 1.), "v"), ((1., 1.), "u"), ((1., 1.), "v"), ((1., 0.), "E"), ((0., 1.), "E")):
            arrays = {k: (None if k == missing else d[k]) for k in d}
            assert call_kick(dev, dtype, r, 0.01, gx, gy, arrays["u"], arrays["v"], arrays["E"]) != 0
            assert missing in err().split(), err()
        from armon_amd._lib import Range
        assert call_kick(dev, dtype, Range(0, -1, 3, 0, 5), 0.01, 1., 1., d["u"], d["v"], d["E"]) != 0 and "range" in err()
        dev.wait()
        for k in d:
            assert same_bits(d[k].to_host(), f[k]), k                      # nothing was written
    finally:
        for a in d.values():
            a.free()


# ---- forced runs -----------------------------------------------------------------------------------------------------------------
def problem(boundaries, **kw):
    from armon_amd import Disc, HalfPlane, Problem, State
    return Problem("forced", State(1., p=1.), [(HalfPlane((1, 2), 1.2), State(0.6, u=0.1, p=0.8)),
                                                (Disc((0.45, 0.55), r=0.22), State(2., u=0.3, v=-0.2, p=2.5))],
                   boundaries=boundaries, samples=2, cfl=0.4, maxtime=1., **kw)


def host_state(grid, names=STATE):
    host = grid.device_to_host(names)
    return {k: host[k].copy() for k in names}


def real(grid, a):
    return grid.real_view(a).copy()


def run_cycles(params, n, grid=None, after_cycle=None):
    """``n`` cycles of the single block driven as ``time_loop`` drives them → (grid, the initial ghosted state, the step of
    every cycle). ``after_cycle(grid, dt)`` runs between a cycle and the clock's advance."""
    from armon_amd.solver import BlockGrid, cycle_ends, init_test, solver_cycle
    if grid is None:
        grid = BlockGrid(params)
        init_test(params, grid)
    else:
        init_test(params, grid, tune=False)
    gdt = grid.global_dt
    gdt.reset()
    grid.dt_inflight.clear()
    first = host_state(grid)
    dts = []
    while gdt.cycle < n:
        assert not solver_cycle(params, grid, last_cycle=cycle_ends(params, gdt) or gdt.cycle == n - 1)
        dts.append(gdt.current_dt)
        if after_cycle is not None:
            after_cycle(grid, gdt.current_dt)
        gdt.next_cycle()
    params.wait()
    return grid, first, dts


def cpu_run(params, first, dts, dtype=None, force=None, cell=None):
    """The CPU run: the oracle's sweeps in ``split_axes`` order alternated with the restated kick, from the ghosted state
    ``first`` with the steps ``dts`` → the flat ghosted arrays. ``dtype``: the precision to run in (default: the run's)."""
    from armon_amd.blocking import first_side, last_side
    from armon_amd.solver import split_axes
    dtype = np.dtype(dtype or params.data_type)
    T = dtype.type
    nx, ny = params.N
    g = params.nghost
    gx, gy = params.gravity if force is None else force
    f = {k: first[k].astype(dtype) for k in STATE}
    for cycle, dt in enumerate(dts):
        for axis, factor in split_axes(params.axis_splitting, cycle):
            ax = int(axis) - 1
            pick = (lambda uv: uv) if ax == 0 else (lambda uv: (uv[1], uv[0]))      # (along the axis, across it)
            dx = float(params.cell_size(ax)) if cell is None else cell[ax]
            res = reference_sweep(f, nx, ny, g, ax, params.riemann_scheme, params.riemann_limiter, params.projection_scheme,
                                  params.test.eos, float(T(dt) * T(factor)), dx, 1, 1, pick(params.test.boundary_condition(first_side(axis))),
                                  pick(params.test.boundary_condition(last_side(axis))), dtype)
            f = {k: getattr(res, k) for k in STATE}
        BF.kick_real(f, nx, ny, g, T(dt), gx, gy)
    return f


PATHS = {"fused": dict(), "pair": dict(placement_min_bytes=0, placement_tries=1), "staged": dict(use_fused_sweep=False)}


def forced_params(path, boundaries, dtype="float64", exact=True, **kw):
    kw.setdefault("gravity", FORCE)
    kw.setdefault("N", N)
    return A().ArmonParameters(test=problem(boundaries), data_type=dtype, silent=5, exact_arithmetic=exact, **PATHS[path], **kw)


# ---- 2. a whole forced run against the CPU -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cst_dt", [True, False], ids=["cst_dt", "cfl"])
@pytest.mark.parametrize("boundaries", ["Dirichlet", "FreeFlow"])
@pytest.mark.parametrize("dtype,path", [(d, p) for d in DTYPES for p in PATHS if (d, p) != ("float32", "pair")])   # (the pair cycle is fp64)
def test_an_exact_forced_run_is_the_cpus(dtype, path, boundaries, cst_dt):
    from armon_amd.solver import pair_cycle, pair_usable
    step = dict(cst_dt=True, Dt=2e-3) if cst_dt else dict()
    params = forced_params(path, boundaries, dtype, **step)
    assert (path == "pair") == bool(params.use_fused_sweep and pair_usable(params))
    grid, first, dts = run_cycles(params, 5)
    assert (path == "pair") == bool(params.use_fused_sweep and pair_cycle(params, grid))
    assert len(dts) == 5 and all(np.isfinite(dt) and dt > 0 for dt in dts) and (not cst_dt or set(dts) == {params.T(2e-3)})
    want = cpu_run(params, first, dts)
    got = host_state(grid)
    for k in STATE:
        assert same_bits(real(grid, got[k]), real(grid, want[k])), (k, float(np.abs(real(grid, got[k]) - real(grid, want[k])).max()))
    # and the force did something: the same run without it ends elsewhere
    free = cpu_run(params, first, dts, force=(0., 0.))
    assert not same_bits(real(grid, free["v"]), real(grid, want["v"]))


@pytest.mark.parametrize("boundaries", ["Dirichlet", "FreeFlow"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_tuned_forced_run_stays_within_the_rounding_of_the_run(dtype, boundaries):
    """The default tuned arithmetic against the exact run, with the yardstick of tests/test_gpu_sweep_random_state.py
    (test_tuned_forms_agree_and_stay_within_the_rounding_of_the_operation) taken for the operation that is run here — 5 forced
    cycles, 10 sweeps and 5 kicks — instead of one sweep: per field kappa = max|cpu32 - cpu64| / (eps32 max|cpu64|), both CPU
    runs (oracle sweeps + restated kick) on the fp32 rounding of this very initial state with the same steps and cell sizes —
    how many roundings of the field maximum the whole run costs when every operation is rounded once; nothing the kernels
    compute enters. The tuned run in precision P may deviate from the fp64 CPU run on its own input (which the exact GPU run
    equals bit for bit in fp64: the test above) by at most 4 kappa eps_P max|field|, that file's bound. Prints what it
    measures (pytest -s)."""
    params = forced_params("fused", boundaries, dtype, exact=False, cst_dt=True, Dt=float(np.float32(2e-3)))
    grid, first, dts = run_cycles(params, 5)
    got = host_state(grid)
    ref64 = cpu_run(params, first, dts, dtype="float64")
    first32 = {k: first[k].astype(np.float32) for k in STATE}
    cell = [float(np.float32(params.cell_size(0))), float(np.float32(params.cell_size(1)))]
    o64, o32 = (cpu_run(params, first32, dts, dtype=t, cell=cell, force=tuple(float(np.float32(v)) for v in params.gravity))
                for t in ("float64", "float32"))
    eps32, eps = float(np.finfo(np.float32).eps), float(np.finfo(np.dtype(dtype)).eps)
    for k in STATE:
        a64 = real(grid, o64[k])
        kappa = float(np.abs(real(grid, o32[k]).astype(np.float64) - a64).max() / (eps32 * np.abs(a64).max()))
        assert kappa > 0.5, (k, kappa)                         # a yardstick, not an accident of one cell
        want = real(grid, ref64[k])
        dev_ = float(np.abs(real(grid, got[k]).astype(np.float64) - want).max() / (eps * np.abs(want).max()))
        print(f"\ntuned forced run {dtype} {boundaries} {k}: {dev_:.2f} eps of the field maximum, kappa {kappa:.2f} (bound {4 * kappa:.2f})")
        assert dev_ <= 4 * kappa, (k, dev_, kappa)


# ---- 3. composition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "pair"])
def test_forced_cycles_are_unforced_cycles_with_the_kick_between_them(path):
    from armon_amd.solver import pair_cycle
    n = 6
    params = forced_params(path, "Dirichlet", cst_dt=True, Dt=2e-3)
    grid, first, dts = run_cycles(params, n)
    assert (path == "pair") == bool(pair_cycle(params, grid))
    forced = host_state(grid)
    nx, ny = params.N

    def host_kick(grid, dt):
        host = host_state(grid, ("u", "v", "E"))
        BF.kick_real(host, nx, ny, params.nghost, dt, *params.gravity)
        grid.host_to_device(host)

    params.forced = False                                       # the same grid, the same parameters, no kick on the device
    try:
        grid, again, dts2 = run_cycles(params, n, grid=grid, after_cycle=host_kick)
    finally:
        params.forced = True
    assert dts2 == dts and all(same_bits(again[k], first[k]) for k in STATE)
    composed = host_state(grid)
    for k in STATE:
        assert same_bits(real(grid, composed[k]), real(grid, forced[k])), k
    assert not same_bits(real(grid, first["v"]), real(grid, forced["v"]))


# ---- 4. decomposition -----------------------------------------------------------------------------------------------------------
def run_block(**kw):
    kw.setdefault("silent", 5)
    stats = A().armon(A().ArmonParameters(return_data=True, **kw))
    host = stats.data.device_to_host(STATE)
    return stats, {k: stats.data.real_view(host[k]).copy() for k in STATE}


@functools.lru_cache(maxsize=None)
def block_12_cycles(exact):
    stats, f = run_block(test=problem("Dirichlet"), N=N, maxcycle=12, gravity=FORCE, exact_arithmetic=exact)
    return stats, f, stats.data.state_digest()


@pytest.mark.parametrize("exact", [False, True], ids=["tuned", "exact"])
@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "in-order"])
@pytest.mark.parametrize("native", [False, True], ids=["host-driven", "native_cycle"])
@pytest.mark.parametrize("P", [(1, 1), (2, 1), (2, 2)], ids=str)
def test_forced_tiles_are_the_single_block(P, native, overlap, exact):
    from armon_amd.multi_tile import TileGroup
    stats, want, digest = block_12_cycles(exact)
    assert stats.cycles == 12
    group = TileGroup(P, test=problem("Dirichlet"), N=N, maxcycle=12, gravity=FORCE, exact_arithmetic=exact, silent=5,
                      native_cycle=native, overlap_halo=overlap)
    try:
        got_stats = group.run()
        assert (got_stats.cycles, got_stats.final_time, got_stats.last_dt) == (stats.cycles, stats.final_time, stats.last_dt)
        got = group.gather(STATE)
        for k in STATE:
            assert same_bits(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))
        assert group.state_digest() == digest
    finally:
        group.close()


def test_staged_forced_tiles_are_the_single_block():
    from armon_amd.multi_tile import TileGroup
    kw = dict(test=problem("FreeFlow"), N=N, maxcycle=6, gravity=FORCE, use_fused_sweep=False, silent=5)
    stats, want = run_block(**kw)
    group = TileGroup((2, 2), **kw)
    try:
        group.run()
        got = group.gather(STATE)
        for k in STATE:
            assert same_bits(got[k], want[k]), k
    finally:
        group.close()


# ---- 5. restart -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fused", "staged"])
def test_a_forced_run_restarts_bit_for_bit(tmp_path, path):
    from armon_amd import SolverException, checkpoint
    kw = dict(test=problem("Dirichlet"), N=N, gravity=FORCE, **PATHS[path])
    whole, f_whole = run_block(maxcycle=12, **kw)
    run_block(maxcycle=12, checkpoint_step=5, output_dir=str(tmp_path), **kw)
    path5 = tmp_path / "checkpoint_000005.ckpt"
    header = checkpoint.read_header(str(path5))
    assert header["gravity"] == [float(v).hex() for v in FORCE] and header["cycle"] == 5
    again, f_again = run_block(maxcycle=12, restart_from=str(path5), **kw)
    assert again.data.state_digest() == whole.data.state_digest() and again.cycles == whole.cycles == 12
    for k in STATE:
        assert same_bits(f_again[k], f_whole[k]), k
    # another force, and a file without the key while a force is set (or the other way round), are refused
    for other in ((0.7, 1.3), (0., 0.)):
        with pytest.raises(SolverException) as e:
            run_block(maxcycle=12, restart_from=str(path5), **{**kw, "gravity": other})
        assert e.value.category == "config" and "gravity" in str(e.value)
    run_block(maxcycle=5, checkpoint_at_end=True, checkpoint_file="free", output_dir=str(tmp_path), **{**kw, "gravity": (0., 0.)})
    assert "gravity" not in checkpoint.read_header(str(tmp_path / "free_000005.ckpt"))
    with pytest.raises(SolverException) as e:
        run_block(maxcycle=12, restart_from=str(tmp_path / "free_000005.ckpt"), **kw)
    assert e.value.category == "config" and "gravity" in str(e.value)
    # ... and so is a comparison of states under different forces
    with pytest.raises(SolverException) as e:
        whole.data.compare_state(str(tmp_path / "free_000005.ckpt"))
    assert e.value.category == "config" and "gravity" in str(e.value)
    assert whole.data.compare_state(str(tmp_path / "checkpoint_000010.ckpt")) is not None


# ---- 6. off is off ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("test", ["Sod_circ", "problem"])
def test_a_zero_force_is_no_force(tmp_path, test):
    case = problem("Dirichlet") if test == "problem" else test
    kw = dict(test=case, N=N, maxcycle=8, checkpoint_at_end=True)
    plain, f_plain = run_block(output_dir=str(tmp_path / "plain"), **kw)
    zero, f_zero = run_block(output_dir=str(tmp_path / "zero"), gravity=(0., -0.), **kw)
    assert zero.data.state_digest() == plain.data.state_digest()
    a = open(tmp_path / "plain" / "checkpoint_000008.ckpt", "rb").read()
    b = open(tmp_path / "zero" / "checkpoint_000008.ckpt", "rb").read()
    assert a == b and b"gravity" not in a[:4112]


# ---- 7. the graph fallback ------------------------------------------------------------------------------------------------------
def test_graph_cycles_with_a_force_give_the_host_driven_bits():
    from armon_amd.solver import graph_cycles_usable
    kw = dict(test=problem("Dirichlet"), N=N, maxcycle=12, gravity=FORCE)
    plain, f_plain = run_block(**kw)
    graph, f_graph = run_block(graph_cycles=True, **kw)
    assert not graph_cycles_usable(graph.data.params) and not hasattr(graph.data, "graph_report")
    free = A().ArmonParameters(test=problem("Dirichlet"), N=N, maxcycle=12, graph_cycles=True, silent=5)
    assert free.device is not None and graph_cycles_usable(free)                # the force is what switches it off
    assert (graph.cycles, graph.final_time, graph.last_dt) == (plain.cycles, plain.final_time, plain.last_dt)
    assert graph.data.state_digest() == plain.data.state_digest()
    for k in STATE:
        assert same_bits(f_graph[k], f_plain[k]), k


# ---- 8. - 10. the hydrostatic column --------------------------------------------------------------------------------------------
def column_params(ny, **kw):
    """gamma = 7/5, rho = 1, p(y) = 2.5 - y at the cell centres of [0, 4 dy] x [0, 1], walls on all sides, gravity (0, -1)."""
    from armon_amd import Problem
    dy = 1. / ny
    y = (np.arange(ny) + 0.5) * dy
    p = np.repeat((2.5 - y)[:, None], 4, axis=1)
    one, zero = np.ones((ny, 4)), np.zeros((ny, 4))
    column = Problem.from_arrays(one, zero, zero, p=p, name="column", gamma=7 / 5, boundaries="Dirichlet", domain_size=(4 * dy, 1.),
                                 gravity=(0., -1.), maxtime=0.5)
    return A().ArmonParameters(test=column, N=(4, ny), cst_dt=True, Dt=0.3 * dy / 1.9, silent=5, return_data=True, **kw)


@functools.lru_cache(maxsize=None)
def column_run(ny):
    stats = A().armon(column_params(ny))
    host = stats.data.device_to_host(STATE)
    return stats, {k: stats.data.real_view(host[k]).copy() for k in STATE}


def test_a_hydrostatic_column_stays_nearly_at_rest():
    """Physics, independent of the kick's restatement. No tolerances: u stays exactly zero, and the residual velocity — first
    order, from the mirror wall, which is not well balanced — shrinks with the cell size and stays far below the free fall
    |g| t = 0.5. The CPU restatement (oracle sweeps + numpy kick, fp64) gives max|v| = 0.0163, 0.0077, 0.0039 for ny = 16, 32,
    64. Prints what it measures (pytest -s)."""
    vmax = {}
    for ny in (32, 64):
        stats, f = column_run(ny)
        assert abs(stats.final_time - 0.5) < stats.last_dt and stats.cycles > ny
        assert not f["u"].any(), ny                              # exactly zero (of either sign)
        assert np.isfinite(f["v"]).all() and (f["rho"] > 0).all()
        vmax[ny] = float(np.abs(f["v"]).max())
        print(f"\nhydrostatic column ny = {ny}: max|v| = {vmax[ny]:.6g} after {stats.cycles} cycles, t = {stats.final_time:.6g}")
    assert vmax[64] < vmax[32] < 0.5, vmax


def test_check_result_does_not_hold_a_forced_run_to_conservation():
    # (the kick does work on a gas in motion: its total energy changes, and check_result must not call that a failure)
    stats = A().armon(A().ArmonParameters(test=problem("Dirichlet"), N=N, maxcycle=12, gravity=FORCE, check_result=True, silent=5))
    assert stats.cycles == 12
    stats = A().armon(A().ArmonParameters(test="Sod_circ", N=N, maxcycle=8, gravity=FORCE, check_result=True, silent=5))
    assert stats.cycles == 8
    A().armon(A().ArmonParameters(test=problem("Dirichlet"), N=N, maxcycle=12, check_result=True, silent=5))     # and holds the others


def test_the_closed_column_keeps_its_mass(tmp_path):
    """The history's exact mass sum between cycle 0 and the end: the walls are closed and the kick moves no mass. atol = 1e-12,
    the tolerance of the reference's conservation test."""
    stats = A().armon(column_params(32, history_step=20, output_dir=str(tmp_path)))
    mass = np.asarray(stats.history.mass, dtype=np.float64)
    assert len(mass) >= 3 and stats.history.cycle[0] == 0 and stats.history.cycle[-1] == stats.cycles
    assert abs(mass[0] - 4. / 32) <= 1e-12                       # rho = 1 on [0, 4 dy] x [0, 1]
    assert abs(mass[-1] - mass[0]) <= 1e-12, (mass[0], mass[-1])
    energy = np.asarray(stats.history.energy, dtype=np.float64)
    assert np.isfinite(energy).all()
