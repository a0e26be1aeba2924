"""Bound-preserving transport of the passive scalars on the GPU: armon_hip_sweep_scalars_bounded against its
restatement (tests/bounded_restated.py), whole runs with ``scalar_transport="bounded"``, checkpoints, and the refusals of the
new entry points. The single launches go through the harness of the scalar sweep (tests/scalars_harness.py) with the bounded
entry point in the place of ``armon_hip_sweep_scalars``; their inputs are those tests/test_bounded_host.py holds the margin of
the clamp on. Tuned arithmetic prints what it measures (pytest -s)."""
import functools
import os

import numpy as np
import pytest

import scalars_harness
from bounded_restated import BCS, CONFIGS, SHAPES, bounded_sweep, launch_inputs, run_cycles
from bounded_planes import assert_in_local_range
from scalars_harness import WALLS, Planes, assert_untouched, descriptor, exact_launch_is_the_restatement, rand_planes
from scalars_harness import bounded_launch as launch
from sweep_harness import F_HIGH, F_LOW, MARKER, bits, block_cache
from sweep_reference import STATE, rand_state, real_mask

pytestmark = pytest.mark.gpu

DTYPES = ("float64", "float32")


def A():
    import armon_amd
    return armon_amd


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


ids = lambda v: v if isinstance(v, str) else ("-".join(map(str, v)) if isinstance(v, tuple) else str(v))


# ---- one sweep through the C ABI -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bc", BCS, ids=lambda v: f"bc{v[0]}{v[1]}")
@pytest.mark.parametrize("config", CONFIGS, ids=ids)
@pytest.mark.parametrize("axis,shape,g", SHAPES, ids=ids)
def test_exact_bounded_sweep_is_the_restatement(blocks, axis, shape, g, config, bc, dtype):
    """Bit for bit on the real cells, nothing else written, inputs and state untouched; ns = 4, and every plane of it alone."""
    nx, ny, f, planes, dt, dx = launch_inputs(axis, shape, g, config, dtype)
    want, _, _ = bounded_sweep(f, planes, nx, ny, g, axis, *config, dt, dx, bc[0], bc[1], F_LOW, F_HIGH, dtype)
    blk = blocks(nx, ny, g, dtype)
    got = exact_launch_is_the_restatement(blk, f, planes, want, axis, *config, dt, bc=bc, launch=launch)
    inside = real_mask(nx, ny, g, axis)
    for p, o in zip(planes, got):                          # (the planes hold values in [-1, 2]: the bound is their own range)
        assert o[inside].min() >= p.min() and o[inside].max() <= p.max()


@functools.lru_cache(maxsize=None)
def bounded_kappa(axis, shape, g, config):
    """scalars_harness.plane_kappa with the bounded restatement: per plane max|restated32 − restated64| / (eps32 max|restated64|)
    over the real cells, both on the same fp32 numbers under walls. Returns (kappas, nothing else)."""
    nx, ny, f32, planes32, dt, dx = launch_inputs(axis, shape, g, config, "float32", ns=2)
    opts = (nx, ny, g, axis, *config, dt, dx, 1, 1, WALLS["f_low"], WALLS["f_high"])
    o32, _, _ = bounded_sweep(f32, planes32, *opts, "float32")
    o64, _, _ = bounded_sweep({k: a.astype(np.float64) for k, a in f32.items()}, [p.astype(np.float64) for p in planes32], *opts, "float64")
    inside = real_mask(nx, ny, g, axis)
    eps32 = float(np.finfo(np.float32).eps)
    kappa = tuple(float(np.abs(a32[inside].astype(np.float64) - a64[inside]).max() / (eps32 * np.abs(a64[inside]).max()))
                  for a32, a64 in zip(o32, o64))
    assert all(k > 0.5 for k in kappa), kappa              # a yardstick, not an accident of one cell
    return kappa


# (not the smallest block: its 16 cells give no yardstick — kappa 0.37 on the restatement alone, an accident of single cells)
TUNED = [(0, (250, 9), 4, CONFIGS[0]), (0, (123, 5), 5, CONFIGS[1]), (0, (123, 5), 5, CONFIGS[0]), (1, (530, 37), 4, CONFIGS[0]),
         (1, (70, 101), 5, CONFIGS[1]), (1, (70, 101), 5, CONFIGS[0])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis,shape,g,config", TUNED, ids=ids)
def test_tuned_bounded_sweep(blocks, axis, shape, g, config, dtype):
    """Within 4 kappa eps of the field maximum from the fp64 restatement of the input the kernel got; exactly the real cells are
    written; plane k of the ns = 4 launch is the ns = 1 launch, bit for bit; no value leaves its plane's range, nor the range
    of the mirrored input at its own cell and the two beside it."""
    nx, ny, f, planes, dt, dx = launch_inputs(axis, shape, g, config, dtype)
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    mark = MARKER[blk.dtype.name]
    P = Planes(blk, 4)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload(planes)
        d = descriptor(blk, axis, *config, False, dt, **WALLS)
        launch(blk, d, P.inp, P.out)
        got_in, got = P.fetch()
        assert_untouched(blk, f, "tuned bounded sweep")
        for k in range(4):
            assert np.array_equal(bits(got_in[k]), bits(planes[k])), f"phi_in[{k}] was modified"
            assert ((bits(got[k]) == mark) == ~inside).all(), f"phi_out[{k}]: not exactly the real cells were written"
            assert got[k][inside].min() >= planes[k].min() and got[k][inside].max() <= planes[k].max()
            assert_in_local_range(got[k], planes[k], inside, nx, ny, g, axis, what=f"plane {k}: ")     # cell by cell: i - 1, i, i + 1
        for k in range(4):
            P.out[0].copy_from_host(blk.marker)
            launch(blk, d, [P.inp[k]], [P.out[0]])
            blk.dev.wait()
            assert np.array_equal(bits(P.out[0].to_host()), bits(got[k])), f"plane {k}: ns = 1 and ns = 4 differ"
        kappa = bounded_kappa(axis, shape, g, config)
        f64 = {k: a.astype(np.float64) for k, a in f.items()}
        ref, _, _ = bounded_sweep(f64, [p.astype(np.float64) for p in planes[:2]], nx, ny, g, axis, *config, dt, dx, 1, 1,
                                  WALLS["f_low"], WALLS["f_high"], "float64")
        eps = float(np.finfo(blk.dtype).eps)
        for k in range(2):
            want = ref[k][inside]
            r = float(np.abs(got[k][inside].astype(np.float64) - want).max() / (eps * np.abs(want).max()))
            print(f"\n{dtype} {'XY'[axis]} {nx}x{ny} {config[0]} {config[2]} {config[3]}: plane {k} {r:.2f} eps of the field maximum "
                  f"(kappa {kappa[k]:.2f}: {r / kappa[k]:.2f} of it, bound 4 kappa)")
            assert r <= 4 * kappa[k], (k, r, kappa[k])
    finally:
        P.free()


# ---- runs ------------------------------------------------------------------------------------------------------------------

N, CYCLES, DT, GHOSTS = (48, 40), 10, 1e-3, 4


def smooth_state(dtype, seed=1):
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


def unit_plane(dtype, seed=5):
    """Random values in [0, 1], about a third of the cells on either end of the range."""
    nx, ny = N
    return np.clip(np.random.default_rng(seed).uniform(-1., 2., (ny, nx)), 0., 1.).astype(dtype).astype(np.float64)


def problem_of(s, scalars, periodic_x=False, **kw):
    sides = ("Periodic", "Periodic", "Dirichlet", "Dirichlet") if periodic_x else ("Dirichlet",) * 4
    return A().Problem.from_arrays(s["rho"], s["u"], s["v"], E=s["E"], boundaries=sides, scalars=scalars, maxtime=1e9, **kw)


def run(**kw):
    kw.setdefault("silent", 5)
    stats = A().armon(A().ArmonParameters(return_data=True, N=N, nghost=GHOSTS, **kw))
    host = stats.data.device_to_host(STATE)
    out = {k: stats.data.real_view(host[k]).copy() for k in STATE}
    for name in stats.scalars:
        out["s:" + name] = stats.data.scalar(name)
    return stats, out


def same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("periodic_x", [False, True], ids=["walls", "periodic-x"])
def test_a_bounded_run_keeps_the_range_and_the_state(periodic_x, exact, dtype):
    """Ten cycles at a constant step, no gravity. After every cycle the random plane lies within [min φ₀, max φ₀] = [0, 1] exactly
    and the uniform plane is what it was, bit for bit; the same run under "remap" leaves the range; the state is the state of
    the "remap" run, bit for bit; in exact arithmetic the run is the restatement's."""
    from armon_amd.blocking import Axis
    from armon_amd.solver import split_axes
    nx, ny = N
    s = smooth_state(dtype)
    phi0 = unit_plane(dtype)
    assert phi0.min() == 0. and phi0.max() == 1.
    T = np.dtype(dtype).type
    kw = dict(data_type=dtype, exact_arithmetic=exact, cst_dt=True, Dt=DT)
    scalars = lambda: [A().Scalar("dye", array=phi0), A().Scalar("flat", 0.7)]
    lowest, highest = np.inf, -np.inf
    for cycles in range(1, CYCLES + 1):
        stats, out = run(test=problem_of(s, scalars(), periodic_x), scalar_transport="bounded", maxcycle=cycles, **kw)
        assert stats.cycles == cycles and stats.scalar_transport == "bounded" and stats.scalars == ("dye", "flat")
        assert out["s:dye"].min() >= 0. and out["s:dye"].max() <= 1., (cycles, out["s:dye"].min(), out["s:dye"].max())
        assert same_bits(out["s:flat"], np.full((ny, nx), T(0.7))), cycles
        old_stats, old = run(test=problem_of(s, scalars(), periodic_x), maxcycle=cycles, **kw)
        assert old_stats.scalar_transport == "remap"
        lowest, highest = min(lowest, old["s:dye"].min()), max(highest, old["s:dye"].max())
        for k in STATE:                                    # the rule touches the planes only
            assert same_bits(out[k], old[k]), (cycles, k)
    assert not same_bits(out["s:dye"], phi0.astype(dtype)) and not same_bits(out["s:dye"], old["s:dye"])
    print(f"\n{dtype} {'exact' if exact else 'tuned'} periodic-x {periodic_x}: remap reaches [{lowest:.6f}, {highest:.6f}], bounded "
          f"ends in [{out['s:dye'].min():.6f}, {out['s:dye'].max():.6f}]")
    assert lowest < 0. or highest > 1.
    if exact:
        g = GHOSTS

        def ghosted(a):
            full = np.zeros((ny + 2 * g, nx + 2 * g), dtype=dtype)
            full[g:g + ny, g:g + nx] = a
            return full.ravel()
        order = lambda cycle: tuple((0 if axis == Axis.X else 1, f) for axis, f in split_axes("Sequential", cycle))
        wall = ((-1., 1.), (-1., 1.))
        want, state, _ = run_cycles({k: ghosted(s[k]) for k in STATE}, [ghosted(phi0), np.full((nx + 2 * g) * (ny + 2 * g), T(0.7))], nx, ny, g,
                                    order, CYCLES, DT, (float(T(1.) / T(nx)), float(T(1.) / T(ny))), "GAD", "minmod", "euler_2nd",
                                    "perfect_gas", dtype, {0: wall, 1: wall}, periodic=(periodic_x, False))
        real = lambda a: a.reshape(ny + 2 * g, -1)[g:g + ny, g:g + nx]
        for k in STATE:
            assert same_bits(out[k], real(state[k])), k
        assert same_bits(out["s:dye"], real(want[0])) and same_bits(out["s:flat"], real(want[1]))


@pytest.mark.parametrize("compress", [False, True], ids=["dense", "packed"])
def test_checkpoint_and_restart_of_a_bounded_run(tmp_path, compress):
    from armon_amd import checkpoint
    s = smooth_state("float64")
    prob = lambda **kw: problem_of(s, {"dye": unit_plane("float64"), "ink": s["v"]}, **kw)
    kw = dict(cfl=0.4, axis_splitting="Strang")
    whole, want = run(test=prob(scalar_transport="bounded"), maxcycle=12, **kw)
    run(test=prob(), scalar_transport="bounded", maxcycle=6, checkpoint_at_end=True, checkpoint_compress=compress, output_dir=str(tmp_path),
        checkpoint_file="ck", **kw)
    path = os.path.join(str(tmp_path), "ck_000006.ckpt")
    header = checkpoint.read_header(path)
    assert header["scalar_transport"] == "bounded" and header["scalars"] == ["dye", "ink"]
    resumed, got = run(test=prob(), scalar_transport="bounded", maxcycle=12, restart_from=path, **kw)
    assert (resumed.cycles, resumed.final_time, resumed.last_dt) == (whole.cycles, whole.final_time, whole.last_dt)
    assert resumed.scalar_transport == "bounded"
    for k in want:
        assert same_bits(got[k], want[k]), k
    assert got["s:dye"].min() >= 0. and got["s:dye"].max() <= 1.
    with pytest.raises(A()._lib.SolverException, match="scalar_transport = 'bounded', this run has scalar_transport = 'remap'"):
        run(test=prob(), maxcycle=12, restart_from=path, **kw)
    plain, _ = run(test=prob(), maxcycle=6, **kw)
    with pytest.raises(A()._lib.SolverException, match="scalar_transport"):
        plain.data.compare_state(path, rtol=0.)


# ---- refusals at the C ABI -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_the_bounded_entry_points_refuse_before_any_launch(blocks, dtype):
    """What tests/test_gpu_scalars.py::test_the_c_abi_refuses_before_any_launch lists, of the new entry points."""
    nx, ny, g = 70, 33, 4
    blk = blocks(nx, ny, g, dtype)
    opts = (0, "GAD", "minmod", "euler_2nd", "perfect_gas")
    f = rand_state(nx, ny, g, "perfect_gas", dtype, 3)
    planes = rand_planes(nx, ny, g, 4, dtype, 4)
    dt, _ = scalars_harness.case_numbers(nx, ny, 0, "perfect_gas", dtype)
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
