"""Passive scalars on the GPU: armon_hip_sweep_scalars against the restatement built from the oracle's
stage calls (tests/scalars_restated.py), whole runs, initial planes and output, and the refusals of the C ABI.

One sweep: every output plane starts as the harness' marker (a NaN with a payload, compared as integers), so what the sweep
writes — the real cells of phi_out — and what it must leave alone — ghosts, phi_in, the eight state arrays of the descriptor,
p, c and the dt scalar — is checked cell by cell. Shapes: X (250, 9), (123, 5): more than one 120-cell strip and 4-row
workgroup, a partial last one, an odd pitch; Y (530, 37), (70, 101): more than one 256-lane group and 32-row run, partial
ones; and the smallest block the state sweep accepts (LAG x LAG cells, tests/test_gpu_random_shapes.py). The mirror factors
of the harness have a transverse factor of -1 on the high side: the planes are mirrored with +1 all the same.
Tuned arithmetic prints what it measures (pytest -s)."""
import os
import random

import numpy as np
import pytest

from scalars_harness import WALLS, Planes, assert_untouched, case_numbers, descriptor, kappa_of_plane, lag_of, launch, rand_planes
from scalars_restated import restated_sweep, run_cycles
from sweep_harness import F_HIGH, F_LOW, MARKER, bits, block_cache
from sweep_reference import STATE, rand_state, real_mask

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("ARMON_RANDOM_SEED", "20261020"))
X_SHAPES = [(250, 9), (123, 5), None]          # None: the smallest block of the configuration
Y_SHAPES = [(530, 37), (70, 101), None]
SCHEMES = [("GAD", "minmod"), ("GAD", "superbee"), ("GAD", "no_limiter"), ("Godunov", "minmod")]
PROJECTIONS = ["euler", "euler_2nd"]
EOSES = ["perfect_gas", "bizarrium"]
BCS = [(1, 1), (1, 0), (0, 1), (0, 0)]
GHOSTS = (4, 5)
NSS = (1, 4)
DTYPES = ("float64", "float32")


def A():
    import armon_amd
    return armon_amd


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


# ---- one sweep through the C ABI -----------------------------------------------------------------------------------------

def draw_cases(seed):
    rng = random.Random(seed)
    decks = {}

    def deal(name, values):
        if not decks.get(name):
            decks[name] = list(values)
            rng.shuffle(decks[name])
        return decks[name].pop()

    cases = []
    for rounds in range(2):
        for dtype in DTYPES:
            for axis in (0, 1):
                for sh in range(3):
                    scheme, limiter = deal(dtype + "scheme", SCHEMES)
                    projection = deal(dtype + "proj", PROJECTIONS)
                    g = deal(dtype + "g", GHOSTS)
                    shape = (X_SHAPES, Y_SHAPES)[axis][sh]
                    if shape is None:
                        shape = (lag_of(scheme, projection),) * 2
                    cases.append(dict(dtype=dtype, axis=axis, nx=shape[0], ny=shape[1], g=g, scheme=scheme, limiter=limiter,
                                      projection=projection, eos=deal(dtype + "eos", EOSES), bc=deal(dtype + "bc", BCS),
                                      ns=deal(dtype + "ns", NSS), seed=rng.randint(0, 10 ** 6)))
    for dtype in DTYPES:                                   # what the issue asks of the draw
        mine = [c for c in cases if c["dtype"] == dtype]
        assert {(c["scheme"], c["limiter"]) for c in mine} == set(SCHEMES)
        for key, values in (("projection", PROJECTIONS), ("eos", EOSES), ("bc", BCS), ("g", GHOSTS), ("ns", NSS), ("axis", (0, 1))):
            assert {c[key] for c in mine} == set(values), (dtype, key)
    return cases


def case_id(c):
    return (f"{c['dtype']}-{'XY'[c['axis']]}-{c['nx']}x{c['ny']}-g{c['g']}-{c['scheme']}-{c['limiter']}-{c['projection']}-{c['eos']}-"
            f"bc{c['bc'][0]}{c['bc'][1]}-ns{c['ns']}")


@pytest.mark.parametrize("case", draw_cases(SEED), ids=case_id)
def test_exact_scalar_sweep_is_the_restatement(blocks, case):
    c = case
    nx, ny, g, axis, ns = c["nx"], c["ny"], c["g"], c["axis"], c["ns"]
    blk = blocks(nx, ny, g, c["dtype"])
    opts = (axis, c["scheme"], c["limiter"], c["projection"], c["eos"])
    f = rand_state(nx, ny, g, c["eos"], c["dtype"], c["seed"])
    planes = rand_planes(nx, ny, g, ns, c["dtype"], c["seed"] + 1)
    dt, dx = case_numbers(nx, ny, axis, c["eos"], c["dtype"])
    want, _ = restated_sweep(f, planes, nx, ny, g, *opts, dt, dx, c["bc"][0], c["bc"][1], F_LOW, F_HIGH, c["dtype"])
    inside = real_mask(nx, ny, g, axis)
    mark = MARKER[blk.dtype.name]
    P = Planes(blk, ns)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload(planes)
        d = descriptor(blk, *opts, True, dt, bc=c["bc"])
        launch(blk, d, P.inp, P.out)
        got_in, got = P.fetch()
        for k in range(ns):
            assert np.isfinite(want[k][inside]).all()
            assert np.array_equal(bits(got_in[k]), bits(planes[k])), f"phi_in[{k}] was modified"
            stray = np.flatnonzero((bits(got[k]) != mark) & ~inside)
            assert stray.size == 0, f"phi_out[{k}]: {stray.size} cells written outside the real cells, first at {stray[0]}"
            bad = np.flatnonzero((bits(got[k]) != bits(want[k])) & inside)
            assert bad.size == 0, (f"phi_out[{k}]: {bad.size} cells differ from the restatement, first at flat index {bad[0]} "
                                   f"(pitch {nx + 2 * g}): {got[k][bad[0]]!r} != {want[k][bad[0]]!r}")
        assert_untouched(blk, f, "exact scalar sweep")
        if ns > 1:                                         # plane k of the ns = 4 launch is the ns = 1 launch on it
            for k in range(ns):
                P.out[0].copy_from_host(blk.marker)
                launch(blk, d, [P.inp[k]], [P.out[0]])
                blk.dev.wait()
                assert np.array_equal(bits(P.out[0].to_host()), bits(got[k])), f"plane {k}: ns = 1 and ns = {ns} differ"
    finally:
        P.free()


# ---- tuned arithmetic ----------------------------------------------------------------------------------------------------

TUNED_CASES = [(dtype, axis, shape, scheme, limiter, projection, eos, g)
               for dtype in DTYPES for axis, shape, scheme, limiter, projection, eos, g in [
                   (0, (250, 9), "GAD", "minmod", "euler_2nd", "perfect_gas", 4), (0, (123, 5), "Godunov", "minmod", "euler", "bizarrium", 5),
                   (1, (530, 37), "GAD", "minmod", "euler_2nd", "perfect_gas", 4), (1, (70, 101), "GAD", "superbee", "euler", "bizarrium", 5),
                   (0, (123, 5), "GAD", "no_limiter", "euler_2nd", "bizarrium", 4), (1, (70, 101), "Godunov", "minmod", "euler_2nd", "perfect_gas", 4)]]


@pytest.mark.parametrize("dtype,axis,shape,scheme,limiter,projection,eos,g", TUNED_CASES,
                         ids=lambda v: v if isinstance(v, str) else ("x".join(map(str, v)) if isinstance(v, tuple) else str(v)))
def test_tuned_scalar_sweep(blocks, dtype, axis, shape, scheme, limiter, projection, eos, g):
    """A plane that holds the state's transverse velocity comes out as the transverse velocity armon_hip_sweep writes, bit
    for bit — under mirrors whose transverse factor is +1, the one a plane is mirrored with (every boundary type of the
    solver); random planes stay within 4 kappa eps of the field maximum from the fp64 restatement."""
    walls = dict(f_low=(-1., 1.), f_high=(1., 1.))
    nx, ny = shape
    seed = 4242 + nx
    blk = blocks(nx, ny, g, dtype)
    opts = (axis, scheme, limiter, projection, eos)
    f = rand_state(nx, ny, g, eos, dtype, seed)
    planes = rand_planes(nx, ny, g, 2, dtype, seed + 1)
    dt, dx = case_numbers(nx, ny, axis, eos, dtype)
    t_name = "v" if axis == 0 else "u"
    inside = real_mask(nx, ny, g, axis)
    P = Planes(blk, 3)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload([f[t_name]] + planes)
        d = descriptor(blk, *opts, False, dt, **walls)
        launch(blk, d, P.inp, P.out)
        _, got = P.fetch()
        assert_untouched(blk, f, "tuned scalar sweep")
        blk.sweep(*opts, False, dt, **walls)               # the state sweep of the same descriptor
        state = blk.fetch()
        assert np.array_equal(bits(got[0])[inside], bits(state[t_name])[inside]), "the plane of ut is not the sweep's ut"
        mark = MARKER[blk.dtype.name]
        for k in range(3):
            assert ((bits(got[k]) == mark) == ~inside).all(), f"phi_out[{k}]: not exactly the real cells were written"
        # random planes against the fp64 restatement of the input the kernel got
        kappa = kappa_of_plane(nx, ny, g, *opts, seed)
        f64 = {k: a.astype(np.float64) for k, a in f.items()}
        ref, _ = restated_sweep(f64, [p.astype(np.float64) for p in planes], nx, ny, g, *opts, dt, dx, 1, 1, walls["f_low"], walls["f_high"], "float64")
        eps = float(np.finfo(blk.dtype).eps)
        for k in range(2):
            want = ref[k][inside]
            r = float(np.abs(got[k + 1][inside].astype(np.float64) - want).max() / (eps * np.abs(want).max()))
            print(f"\n{dtype} {'XY'[axis]} {nx}x{ny} {scheme} {projection} {eos}: plane {k} {r:.2f} eps of the field maximum "
                  f"(kappa {kappa[k]:.2f}: {r / kappa[k]:.2f} of it, bound 4 kappa)")
            assert r <= 4 * kappa[k], (k, r, kappa[k])
    finally:
        P.free()


TUNED_CONFIGS = [("GAD", "minmod", "euler_2nd", "perfect_gas"), ("Godunov", "minmod", "euler", "bizarrium")]
# X: odd pitch (the clamped scalar-access path, a partial last strip and row group); the 16-B path with more than one strip; the
# smallest block of the configuration (None: LAG x LAG). Y: partial lane group, more than one run.
TUNED_PLANE_SHAPES = [(0, (123, 5), 5), (0, (250, 9), 4), (0, None, 4), (1, (70, 101), 5)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme,limiter,projection,eos", TUNED_CONFIGS, ids=lambda v: v)
@pytest.mark.parametrize("axis,shape,g", TUNED_PLANE_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tuned_planes_do_not_depend_on_their_company(blocks, axis, shape, g, scheme, limiter, projection, eos, dtype):
    """Tuned arithmetic: plane k of an ns = 4 launch is, bit for bit, the ns = 1 launch on that plane; and in the same ns = 4
    launch the plane that holds the state's transverse velocity is the transverse velocity armon_hip_sweep writes (mirrors
    whose transverse factor is +1, as in test_tuned_scalar_sweep)."""
    nx, ny = shape if shape is not None else (lag_of(scheme, projection),) * 2
    seed = 777 + nx
    blk = blocks(nx, ny, g, dtype)
    opts = (axis, scheme, limiter, projection, eos)
    f = rand_state(nx, ny, g, eos, dtype, seed)
    t_name = "v" if axis == 0 else "u"
    planes = [f[t_name]] + rand_planes(nx, ny, g, 3, dtype, seed + 1)
    dt, _ = case_numbers(nx, ny, axis, eos, dtype)
    inside = real_mask(nx, ny, g, axis)
    mark = MARKER[blk.dtype.name]
    P = Planes(blk, 4)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload(planes)
        d = descriptor(blk, *opts, False, dt, **WALLS)
        launch(blk, d, P.inp, P.out)
        _, got = P.fetch()
        assert_untouched(blk, f, "tuned scalar sweep")
        for k in range(4):
            assert ((bits(got[k]) == mark) == ~inside).all(), f"phi_out[{k}]: not exactly the real cells were written"
        for k in range(4):
            P.out[0].copy_from_host(blk.marker)
            launch(blk, d, [P.inp[k]], [P.out[0]])
            blk.dev.wait()
            assert np.array_equal(bits(P.out[0].to_host()), bits(got[k])), f"plane {k}: ns = 1 and ns = 4 differ"
        blk.sweep(*opts, False, dt, **WALLS)               # the state sweep of the same descriptor
        state = blk.fetch()
        assert np.array_equal(bits(got[0])[inside], bits(state[t_name])[inside]), "the plane of ut is not the sweep's ut"
    finally:
        P.free()


# ---- runs ------------------------------------------------------------------------------------------------------------------

RUN_SHAPES = [(96, 8), (8, 96), (40, 24)]


def smooth_state(N, dtype, seed=1):
    """A smooth, non-uniform state of the unit square whose velocities take both signs → (ny, nx) arrays rho, u, v, E."""
    nx, ny = N
    y, x = np.meshgrid((np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    rng = np.random.default_rng(seed)
    rho = 1. + 0.3 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0.02 * rng.uniform(-1, 1, x.shape)
    u = 0.3 * np.cos(2 * np.pi * (x + y)) + 0.02 * rng.uniform(-1, 1, x.shape)
    v = 0.25 * np.sin(2 * np.pi * (x - 2 * y)) + 0.02 * rng.uniform(-1, 1, x.shape)
    p = 1. + 0.2 * np.cos(2 * np.pi * x)
    E = p / (0.4 * rho) + 0.5 * (u * u + v * v)
    return {k: a.astype(dtype).astype(np.float64) for k, a in dict(rho=rho, u=u, v=v, E=E).items()}


def problem_of(s, scalars=None, boundaries="Dirichlet", **kw):
    return A().Problem.from_arrays(s["rho"], s["u"], s["v"], E=s["E"], boundaries=boundaries, scalars=scalars, maxtime=1e9, **kw)


def run(**kw):
    kw.setdefault("silent", 5)
    stats = A().armon(A().ArmonParameters(return_data=True, **kw))
    host = stats.data.device_to_host(STATE)
    out = {k: stats.data.real_view(host[k]).copy() for k in STATE}
    for name in stats.scalars:
        out["s:" + name] = stats.data.scalar(name)
    return stats, out


def same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("periodic", [False, True], ids=["walls", "periodic"])
@pytest.mark.parametrize("N,splitting", [((96, 8), "X_only"), ((8, 96), "Y_only"), ((40, 24), "X_only"), ((40, 24), "Y_only")])
def test_a_plane_that_starts_as_the_transverse_velocity_stays_it(N, splitting, periodic, exact, dtype):
    s = smooth_state(N, dtype)
    t_name = "v" if splitting == "X_only" else "u"
    sides = ("Dirichlet",) * 4
    if periodic:
        sides = ("Periodic", "Periodic", "Dirichlet", "Dirichlet") if splitting == "X_only" else ("Dirichlet", "Dirichlet", "Periodic", "Periodic")
    stats, out = run(test=problem_of(s, {"phi": s[t_name]}, boundaries=sides), N=N, data_type=dtype, axis_splitting=splitting,
                     exact_arithmetic=exact, maxcycle=12, cfl=0.4)
    assert stats.cycles == 12 and stats.scalars == ("phi",)
    assert not same_bits(out[t_name], s[t_name].astype(dtype))          # it moved
    assert same_bits(out["s:phi"], out[t_name])


def test_gravity_does_not_kick_a_plane():
    N = (40, 24)
    s = smooth_state(N, "float64")
    stats, out = run(test=problem_of(s, {"phi": s["v"]}), N=N, axis_splitting="X_only", maxcycle=10, cfl=0.4, gravity=(0.7, 0.))
    _, free = run(test=problem_of(s), N=N, axis_splitting="X_only", maxcycle=10, cfl=0.4)
    assert not same_bits(out["u"], free["u"])                          # the force acted
    assert same_bits(out["s:phi"], out["v"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,splitting,periodic", [((40, 24), "Sequential", (False, False)), ((96, 8), "Strang", (False, False)),
                                                  ((8, 96), "Strang", (False, True)), ((40, 24), "Sequential", (True, False))])
def test_exact_runs_are_the_restatements_cycles(N, splitting, periodic, dtype):
    from armon_amd.blocking import Axis
    from armon_amd.solver import split_axes
    nx, ny = N
    g, cycles, Dt = 4, 10, 1e-3
    s = smooth_state(N, dtype)
    rng = np.random.default_rng(9)
    phis = {"a": rng.uniform(0., 1., (ny, nx)).astype(dtype).astype(np.float64), "b": s["rho"] - 1.}
    sides = tuple("Periodic" if periodic[k // 2] else "Dirichlet" for k in range(4))
    stats, out = run(test=problem_of(s, phis, boundaries=sides), N=N, data_type=dtype, axis_splitting=splitting, exact_arithmetic=True,
                     maxcycle=cycles, cst_dt=True, Dt=Dt, nghost=g)
    assert stats.cycles == cycles

    def ghosted(a):
        full = np.zeros((ny + 2 * g, nx + 2 * g), dtype=dtype)
        full[g:g + ny, g:g + nx] = a
        return full.ravel()
    T = np.dtype(dtype).type
    order = lambda cycle: tuple((0 if axis == Axis.X else 1, f) for axis, f in split_axes(splitting, cycle))
    wall = ((-1., 1.), (-1., 1.))
    want, state = run_cycles({k: ghosted(s[k]) for k in STATE}, [ghosted(phis["a"]), ghosted(phis["b"])], nx, ny, g, order, cycles, Dt,
                             (float(T(1.) / T(nx)), float(T(1.) / T(ny))), "GAD", "minmod", "euler_2nd", "perfect_gas", dtype,
                             {0: wall, 1: wall}, periodic=periodic)
    real = lambda a: a.reshape(ny + 2 * g, -1)[g:g + ny, g:g + nx]
    for k in STATE:
        assert same_bits(out[k], real(state[k])), k
    for name, w in zip("ab", want):
        assert same_bits(out["s:" + name], real(w)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_scalars_do_not_change_the_state_and_take_the_single_sweeps(dtype):
    N = (40, 24)
    s = smooth_state(N, dtype)
    kw = dict(N=N, data_type=dtype, maxcycle=15, cfl=0.4, placement_min_bytes=0, placement_tries=1)
    plain, want = run(test=problem_of(s), **kw)
    dyed, got = run(test=problem_of(s, {"dye": s["rho"]}), **kw)
    assert (plain.cycles, plain.final_time, plain.last_dt) == (dyed.cycles, dyed.final_time, dyed.last_dt)
    for k in STATE:
        assert same_bits(got[k], want[k]), k
    assert dyed.data.pair_cycles == 0
    if dtype == "float64":
        assert plain.data.pair_cycles > 0                               # (what the run without scalars takes at this setting)
    graph, again = run(test=problem_of(s, {"dye": s["rho"]}), graph_cycles=True, **kw)
    assert (graph.cycles, graph.final_time) == (dyed.cycles, dyed.final_time)
    for k in list(STATE) + ["s:dye"]:
        assert same_bits(again[k], got[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("N,splitting,periodic", [((40, 24), "Sequential", (False, False)), ((96, 8), "Strang", (True, False)),
                                                  ((8, 96), "Sequential", (False, True))])
def test_a_uniform_plane_and_the_content_of_a_plane(N, splitting, periodic, exact, dtype):
    """A uniform 0.7 deviates by at most 4 eps x 0.7 per sweep executed (the oracle measured 1.43 eps for one sweep); the
    content of a random positive plane, summed on the host in fp64, drifts by at most 4 eps per sweep executed, relatively."""
    nx, ny = N
    cycles = 12
    s = smooth_state(N, dtype)
    rng = np.random.default_rng(21)
    phi0 = rng.uniform(0.5, 1.5, (ny, nx)).astype(dtype).astype(np.float64)
    sides = tuple("Periodic" if periodic[k // 2] else "Dirichlet" for k in range(4))
    stats, out = run(test=problem_of(s, [A().Scalar("flat", 0.7), A().Scalar("dye", array=phi0)], boundaries=sides), N=N,
                     data_type=dtype, axis_splitting=splitting, exact_arithmetic=exact, maxcycle=cycles, cfl=0.4)
    sweeps = cycles * (3 if splitting == "Strang" else 2)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    T = np.dtype(dtype).type
    dev = float(np.abs(out["s:flat"].astype(np.float64) - float(T(0.7))).max() / (eps * 0.7))
    before = float((s["rho"] * phi0).sum())
    after = float((out["rho"].astype(np.float64) * out["s:dye"].astype(np.float64)).sum())
    drift = abs(after - before) / (eps * before)
    print(f"\n{dtype} {N} {splitting} periodic {periodic} {'exact' if exact else 'tuned'}: uniform plane {dev:.2f} eps, content drift "
          f"{drift:.2f} eps after {sweeps} sweeps (bounds {4 * sweeps})")
    assert dev <= 4 * sweeps
    assert drift <= 4 * sweeps


@pytest.mark.parametrize("compress", [False, True], ids=["dense", "packed"])
def test_checkpoint_and_restart_carry_the_planes(tmp_path, compress):
    from armon_amd import checkpoint
    N = (40, 24)
    s = smooth_state(N, "float64")
    prob = lambda: problem_of(s, {"dye": s["rho"], "ink": s["v"]})
    kw = dict(N=N, cfl=0.4, axis_splitting="Strang")
    whole, want = run(test=prob(), maxcycle=12, **kw)
    _, _half = run(test=prob(), maxcycle=6, checkpoint_at_end=True, checkpoint_compress=compress, output_dir=str(tmp_path),
                   checkpoint_file="ck", **kw)
    path = os.path.join(str(tmp_path), "ck_000006.ckpt")
    header = checkpoint.read_header(path)
    assert header["planes"] == ["rho", "u", "v", "E", "s:dye", "s:ink"] and header["scalars"] == ["dye", "ink"]
    assert set(header["digests"]) == set(header["planes"])
    resumed, got = run(test=prob(), maxcycle=12, restart_from=path, **kw)
    assert (resumed.cycles, resumed.final_time, resumed.last_dt) == (whole.cycles, whole.final_time, whole.last_dt)
    for k in want:
        assert same_bits(got[k], want[k]), k
    diff = resumed.data.compare_state(path, rtol=0.)
    assert set(diff.vars) >= {"s:dye", "s:ink"} and diff.different      # six cycles later: every plane is compared, and moved
    with pytest.raises(A()._lib.SolverException, match="scalars"):
        run(test=problem_of(s, {"dye": s["rho"]}), maxcycle=12, restart_from=path, **kw)


# ---- initial planes and output -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("samples", [1, 4])
def test_a_region_built_plane_is_the_density_of_its_twin_problem(samples, dtype):
    from armon_amd import Box, Disc, Ellipse, HalfPlane, Problem, Scalar, State
    from armon_amd.solver import BlockGrid, init_test
    shapes = [(Disc((0.4, 0.55), 0.23), 2.5), (HalfPlane((1, 2), 0.9), 0.125), (Box(x=(0.6, 0.93), y=(0.1, 0.47)), 7.),
              (Ellipse((0.3, 0.3), (0.25, 0.1)), 1e-3)]
    N, g = (45, 37), 5

    def planes(test, names, **kw):
        params = A().ArmonParameters(test=test, N=N, nghost=g, data_type=dtype, silent=5, **kw)
        grid = BlockGrid(params)
        init_test(params, grid)
        return grid, {k: grid.data[k].to_host() for k in names}
    twin = Problem("twin", State(0.75, p=1.), [(sh, State(v, p=1.)) for sh, v in shapes], samples=samples)
    _, want = planes(twin, ["rho"])
    host = Problem("host", State(1., p=1.), [(Disc((0.5, 0.5), 0.2), State(2., p=2.))], samples=samples,
                   scalars=[Scalar("dye", 0.75, shapes)])
    grid, got = planes(host, ["s:dye", "s:neg"], scalars=[Scalar("neg", -0.75, [(sh, -v) for sh, v in shapes])])
    assert np.array_equal(bits(got["s:dye"]), bits(want["rho"]))       # ghosts included: global positions only
    inner = grid.real_view(got["s:neg"])
    assert np.isfinite(inner).all() and (inner < 0).all()              # values of either sign
    if samples == 1:
        assert np.array_equal(got["s:neg"], -want["rho"])
    given = [0.75] + [v for _, v in shapes]
    assert (~np.isin(grid.real_view(want["rho"]), np.array(given, dtype=dtype))).any() == (samples > 1)      # cut cells take a mean
    # derive: the plane in the slot of rho
    twin_grid, _ = planes(twin, ["rho"])
    a, b = grid.derive(["scalar:dye"], factor=2), twin_grid.derive(["rho"], factor=2)
    assert same_bits(a["scalar:dye"], b["rho"]) and a["scalar:dye"].shape == (19, 23)
    both = grid.derive(["scalar:neg", "rho", "scalar:dye"], factor=2, reduce={"scalar:neg": "min"})
    assert same_bits(both["scalar:dye"], b["rho"]) and same_bits(both["rho"], grid.derive(["rho"], factor=2)["rho"])
    assert same_bits(both["scalar:neg"], grid.derive(["scalar:neg"], factor=2, reduce="min")["scalar:neg"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_array_plane_is_the_array_rounded(dtype):
    from armon_amd.solver import BlockGrid, init_test
    N = (45, 37)
    rng = np.random.default_rng(2)
    a = rng.normal(size=(N[1], N[0]))
    params = A().ArmonParameters(test="Sod", N=N, data_type=dtype, silent=5, scalars={"dye": a, "two": 2 * a})
    grid = BlockGrid(params)
    init_test(params, grid)
    assert same_bits(grid.scalar("dye"), a.astype(dtype)) and same_bits(grid.scalar("two"), (2 * a).astype(dtype))
    with pytest.raises(A()._lib.SolverException, match="no scalar"):
        grid.scalar("ink")


# ---- refusals at the C ABI -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_c_abi_refuses_before_any_launch(blocks, dtype):
    nx, ny, g = 70, 33, 4
    blk = blocks(nx, ny, g, dtype)
    opts = (0, "GAD", "minmod", "euler_2nd", "perfect_gas")
    f = rand_state(nx, ny, g, "perfect_gas", dtype, 3)
    planes = rand_planes(nx, ny, g, 4, dtype, 4)
    dt, _ = case_numbers(nx, ny, 0, "perfect_gas", dtype)
    P = Planes(blk, 4)
    spare = blk.dev.empty(blk.n, blk.dtype)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload(planes)
        fresh = lambda **kw: descriptor(blk, *opts, kw.pop("exact", True), dt, **kw)

        def refused(match, d=None, inp=None, out=None, ns=None):
            inp, out = (P.inp if inp is None else inp), (P.out if out is None else out)
            msg = launch(blk, fresh() if d is None else d, inp, out, ns=ns, expect=1)
            assert match in msg, (match, msg)

        refused("ns = 0", ns=0)
        refused("ns = 5", inp=P.inp + [spare], out=P.out + [spare], ns=5)
        refused("phi_in[2] is NULL", inp=P.inp[:2] + [None] + P.inp[3:])
        refused("phi_out[1] is NULL", out=P.out[:1] + [None] + P.out[2:])
        refused("phi_out[3] aliases phi_in[0]", out=P.out[:3] + [P.inp[0]])
        refused("phi_out[0] aliases phi_out[2]", out=P.out[:2] + [P.out[0]] + P.out[3:])
        refused("phi_out[0] aliases a state array", out=[blk.grid.data["rho"]] + P.out[1:])
        refused("phi_out[1] aliases a state array", out=P.out[:1] + [blk.grid.alt["E"]] + P.out[2:])
        d = fresh()
        d.dt_state = spare.ptr
        refused("dt_state", d)
        d = fresh()
        d.out_lo, d.out_hi = 4, nx
        refused("out_lo / out_hi", d)
        d = fresh()
        d.out_lo, d.out_hi = 0, nx                          # the whole block, spelled out: accepted
        launch(blk, d, P.inp, P.out)
        P.upload(planes)
        d = fresh()
        d.x_kernel = 3
        refused("x_kernel", d)
        d = fresh()
        d.u_factor_low = 0.5
        refused("mirror factors", d)
        d = fresh()
        d.nghost = 3
        refused("nghost", d)
        for field, value, match in (("axis", 2, "axis"), ("scheme", 7, "scheme"), ("projection", 9, "projection"), ("eos", 5, "EOS"),
                                    ("limiter", 8, "limiter"), ("nx", 0, "empty block"), ("rho_in", None, "NULL state array")):
            d = fresh()
            setattr(d, field, value)
            refused(match, d)
        _, outs = P.fetch()
        mark = MARKER[blk.dtype.name]
        for k, a in enumerate(outs):
            assert (bits(a) == mark).all(), f"phi_out[{k}] was written by a refused call"
        assert_untouched(blk, f, "refused calls")
    finally:
        blk.dev.wait()
        spare.free()
        P.free()
