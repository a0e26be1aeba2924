"""Periodic sides on the GPU (csrc/periodic.hip): the kernel against a numpy restatement of its rule, and
whole runs of a lone periodic block against the CPU oracle's periodic runs, against periodic tile groups, under translation,
on a smooth wave, and through everything around the solver. "Equals" always means bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
DTYPES = ("float64", "float32")
PERIODIC = [(True, True), (True, False), (False, True)]


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


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------
def restated(a, axis, pitch, g, layers, nx, ny):
    """The rule of include/armon_hip.h on the flat vector ``a`` (a copy is returned) and the mask of the cells it writes."""
    rows = ny + 2 * g
    out = a[:rows * pitch].reshape(rows, pitch).copy()
    src = out.copy()
    mask = np.zeros((rows, pitch), dtype=bool)
    n = nx if axis == 0 else ny
    for l in range(layers):
        if axis == 0:
            out[g:g + ny, g - 1 - l] = src[g:g + ny, g + n - 1 - l]
            out[g:g + ny, g + n + l] = src[g:g + ny, g + l]
            mask[g:g + ny, g - 1 - l] = mask[g:g + ny, g + n + l] = True
        else:
            out[g - 1 - l, g:g + nx] = src[g + n - 1 - l, g:g + nx]
            out[g + n + l, g:g + nx] = src[g + l, g:g + nx]
            mask[g - 1 - l, g:g + nx] = mask[g + n + l, g:g + nx] = True
    return out.ravel(), mask.ravel()


def marked(size, dtype, seed):
    """``size`` distinct bit patterns (NaNs, subnormals and signed zeros among them): a moved value is told from any other."""
    u = np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32
    mult = 0x9E3779B97F4A7C15 if u is np.uint64 else 0x9E3779B1
    with np.errstate(over="ignore"):
        a = (np.arange(1, size + 1, dtype=u) + u(seed)) * u(mult)
    return a.view(dtype)


def call_wrap(dev, dtype, axis, pitch, g, layers, nx, ny, ptrs, nvars=None, ctx="dev"):
    fn = getattr(dev._L, "armon_hip_periodic_ghosts" + ("_f32" if np.dtype(dtype) == np.float32 else ""))
    vars_ = None if ptrs is None else (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    return fn(dev.ctx if ctx == "dev" else ctx, axis, pitch, g, layers, nx, ny, len(ptrs) if nvars is None else nvars, vars_)


# (nx, ny, nghost, extra pitch, nvars, element offset of the vectors): odd and even pitches, a pitch padded to a whole 128-B line
# (64 x 24 with nghost 4: 72 -> 80 fp64 / 96 fp32 is covered by +8 / +24), a vector one element off a 16-B boundary
SHAPES = [(37, 5, 4, 0, 4, 0), (37, 5, 5, 0, 1, 0), (5, 37, 4, 0, 7, 0), (5, 37, 5, 3, 8, 0), (64, 24, 4, 0, 4, 0),
          (64, 24, 4, 8, 4, 0), (64, 24, 4, 24, 8, 0), (64, 24, 5, 0, 7, 1), (64, 24, 4, 0, 4, 1), (130, 3, 4, 1, 1, 0),
          (4, 4, 4, 0, 4, 0), (5, 5, 5, 0, 8, 0), (2, 9, 4, 0, 1, 0), (9, 2, 5, 6, 4, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "{}x{}-g{}-pad{}-v{}-off{}".format(*s))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_the_wrap_is_the_rule_and_touches_nothing_else(dev, axis, dtype, shape):
    nx, ny, g, pad, nvars, off = shape
    pitch = nx + 2 * g + pad
    size = pitch * (ny + 2 * g)
    item = np.dtype(dtype).itemsize
    host = [marked(size + off, dtype, 7919 * k) for k in range(nvars)]
    d = [dev.empty(size + off, dtype) for _ in range(nvars)]
    n = nx if axis == 0 else ny
    try:
        for layers in sorted({1, 2, g}):
            if layers > n:
                continue
            for a, h in zip(d, host):
                a.copy_from_host(h)
            assert call_wrap(dev, dtype, axis, pitch, g, layers, nx, ny, [a.ptr + off * item for a in d]) == 0, \
                dev._L.armon_hip_last_error()
            dev.wait()
            for k, (a, h) in enumerate(zip(d, host)):
                got = a.to_host()
                want, mask = restated(h[off:], axis, pitch, g, layers, nx, ny)
                assert mask.sum() == 2 * layers * (ny if axis == 0 else nx)
                assert np.array_equal(bits(got[:off]), bits(h[:off])), (k, layers)
                assert np.array_equal(bits(got[off:])[~mask], bits(h[off:])[~mask]), (k, layers, "a cell outside the ghosts moved")
                assert np.array_equal(bits(got[off:]), bits(want)), (k, layers)
                assert (bits(got[off:])[mask] != bits(h[off:])[mask]).all(), (k, layers)      # every ghost was written
    finally:
        for a in d:
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_a_block_of_more_rows_than_a_grid_extent_is_one_launch(dev, axis, dtype):
    nx, ny, g, nvars = 4, 70001, 4, 2
    pitch = nx + 2 * g
    size = pitch * (ny + 2 * g)
    host = [marked(size, dtype, 104729 * k) for k in range(nvars)]
    d = [dev.from_host(h) for h in host]
    try:
        assert call_wrap(dev, dtype, axis, pitch, g, g, nx, ny, [a.ptr for a in d]) == 0, dev._L.armon_hip_last_error()
        dev.wait()
        for a, h in zip(d, host):
            want, _ = restated(h, axis, pitch, g, g, nx, ny)
            assert np.array_equal(bits(a.to_host()), bits(want))
    finally:
        for a in d:
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", [0, 1], ids=["x", "y"])
def test_a_block_of_more_spans_than_the_grid_holds_waves_is_one_launch(dev, axis, dtype):
    """The wide twin: along y, 2 variables x 8 rows x 2344 spans of a wave (1172 in fp32) are at least twice as many wave items as a grid
    capped at 8 workgroups of 4 waves per CU holds waves, on any device of up to 293 CUs: every wave of k_periodic_y goes round
    its grid-stride loop a second time (on 256 CUs: 8192 waves, 37504 and 18752 items); along x, the two lines are 300007 cells apart."""
    nx, ny, g, nvars = 300007, 5, 4, 2
    pitch = nx + 2 * g
    size = pitch * (ny + 2 * g)
    host = [marked(size, dtype, 130003 * k) for k in range(nvars)]
    d = [dev.from_host(h) for h in host]
    try:
        assert call_wrap(dev, dtype, axis, pitch, g, g, nx, ny, [a.ptr for a in d]) == 0, dev._L.armon_hip_last_error()
        dev.wait()
        for a, h in zip(d, host):
            want, mask = restated(h, axis, pitch, g, g, nx, ny)
            got = a.to_host()
            assert np.array_equal(bits(got), bits(want))
            assert (bits(got)[mask] != bits(h)[mask]).all()                                  # every ghost was written
    finally:
        for a in d:
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wrap_refuses_before_any_launch(dev, dtype):
    nx, ny, g = 6, 3, 4
    pitch = nx + 2 * g
    host = marked(pitch * (ny + 2 * g), dtype, 1)
    a = dev.from_host(host)
    err = lambda: dev._L.armon_hip_last_error().decode()
    p = [a.ptr]
    try:
        for what, kw in (("ctx", dict(ctx=None)), ("axis", dict(axis=2)), ("axis", dict(axis=-1)), ("nvars", dict(ptrs=[], nvars=0)),
                         ("nvars", dict(ptrs=p * 9)), ("vars", dict(ptrs=None, nvars=1)), ("vars[1]", dict(ptrs=[a.ptr, None])),
                         ("layers", dict(layers=0)), ("layers", dict(layers=g + 1)), ("layers", dict(axis=1, layers=4)),
                         ("row_length", dict(pitch=pitch - 1)), ("nx", dict(nx=0)), ("ny", dict(ny=0))):
            args = dict(axis=0, pitch=pitch, g=g, layers=g, nx=nx, ny=ny, ptrs=p)
            args.update(kw)
            assert call_wrap(dev, dtype, **args) != 0, what
            assert what in err(), (what, err())
        # n < layers on the other axis is no obstacle, and n == layers is allowed
        assert call_wrap(dev, dtype, 0, pitch, g, g, nx, ny, p) == 0
        assert call_wrap(dev, dtype, 1, pitch, g, 3, nx, ny, p) == 0
        dev.wait()
        want, _ = restated(restated(host, 0, pitch, g, g, nx, ny)[0], 1, pitch, g, 3, nx, ny)
        assert np.array_equal(bits(a.to_host()), bits(want))                  # and the refused calls wrote nothing
    finally:
        a.free()


# ---- whole runs ---------------------------------------------------------------------------------------------------------------
def run_block(**kw):
    kw.setdefault("silent", 5)
    stats = A().armon(A().ArmonParameters(return_data=True, **kw))
    host = stats.data.device_to_host(STATE)
    return stats, {k: stats.data.real_view(host[k]).copy() for k in STATE}


def run_group(P, names=STATE, **kw):
    from armon_amd.multi_tile import TileGroup
    kw.setdefault("silent", 5)
    group = TileGroup(P, **kw)
    try:
        stats = group.run()
        return stats, group.gather(names), group.state_digest()
    finally:
        group.close()


# ---- 2. a lone block against the oracle ----------------------------------------------------------------------------------------
GODUNOV = dict(scheme="Godunov", projection="euler")
ORACLE_RUNS = [
    ("Sod_circ", (41, 27), (True, True), dict(maxcycle=30)),
    ("Sod_circ", (41, 27), (True, False), dict(maxcycle=20, axis_splitting="Strang", nghost=5)),
    ("Sod_circ", (41, 27), (False, True), dict(maxcycle=20, axis_splitting="SequentialSym")),
    ("Sod_circ", (41, 27), (True, True), dict(maxcycle=12, axis_splitting="X_only", **GODUNOV)),
    ("Sod_circ", (41, 27), (True, True), dict(maxcycle=12, axis_splitting="Y_only", nghost=5)),
    ("Sedov", (41, 27), (True, True), dict(maxcycle=20, axis_splitting="Strang")),
    ("Sedov", (41, 27), (True, False), dict(maxcycle=12, **GODUNOV)),
    ("Sedov", (41, 27), (False, True), dict(maxcycle=12, nghost=5)),
    ("Bizarrium", (41, 27), (True, True), dict(maxcycle=20, axis_splitting="SequentialSym", nghost=5)),
    ("Bizarrium", (41, 27), (True, False), dict(maxcycle=12)),
    ("Bizarrium", (41, 27), (False, True), dict(maxcycle=12, axis_splitting="Strang", **GODUNOV)),
    ("Sod_circ", (64, 24), (True, True), dict(maxcycle=20, data_type="float32")),
    ("Sedov", (64, 24), (False, True), dict(maxcycle=12, data_type="float32", axis_splitting="Strang")),
    ("Bizarrium", (64, 24), (True, False), dict(maxcycle=12, data_type="float32", nghost=5)),
]


def run_id(r):
    test, N, per, o = r
    return f"{test}-{N[0]}x{N[1]}-per{int(per[0])}{int(per[1])}-" + "-".join(f"{v}" for k, v in sorted(o.items()))


@pytest.mark.parametrize("run", ORACLE_RUNS, ids=run_id)
def test_a_lone_periodic_block_is_the_oracles(oracle, run):
    test, N, periodic, opts = run
    dtype = np.dtype(opts.get("data_type", "float64"))
    g = opts.get("nghost", 4)
    opts = dict(opts, maxtime=1e3)                      # the cycle count ends every run, not the case's own final time
    orun, f = oracle.solve(test=test, N=N, periodic=periodic, **{**opts, "data_type": dtype.type})
    ref = {k: oracle.real_view(f[k], N[0], N[1], g) for k in STATE}
    assert orun.cycles == opts["maxcycle"] and all(np.isfinite(ref[k]).all() for k in STATE)
    for path, kw in (("fused exact", dict(exact_arithmetic=True)), ("staged", dict(use_fused_sweep=False))):
        stats, got = run_block(test=test, N=N, periodic=periodic, **opts, **kw)
        assert (stats.cycles, stats.last_dt, stats.final_time) == (orun.cycles, orun.last_dt, orun.final_time), path
        for k in STATE:
            assert same_bits(got[k], ref[k]), (path, k, float(np.abs(got[k] - ref[k]).max()))
    # the tuned arithmetic: the project's bar (tests/test_gpu_random_shapes.py)
    stats, got = run_block(test=test, N=N, periodic=periodic, **opts)
    f64 = dtype.itemsize == 8
    assert stats.cycles == orun.cycles
    assert abs(stats.last_dt - orun.last_dt) <= (1e-12 if f64 else 1e-4) * orun.last_dt
    for k in STATE:
        scale = max(float(np.abs(ref[k]).max()), 1e-300)
        assert np.abs(got[k] - ref[k]).max() <= (1e-11 if f64 else 2e-4) * scale, (k, float(np.abs(got[k] - ref[k]).max() / scale))


def test_the_walls_of_the_same_case_give_other_bits(oracle):
    """The periodic runs above are not the wall runs in disguise."""
    _, wall = run_block(test="Sod_circ", N=(41, 27), maxcycle=30, exact_arithmetic=True)
    _, wrapped = run_block(test="Sod_circ", N=(41, 27), maxcycle=30, exact_arithmetic=True, periodic=(True, True))
    assert not same_bits(wall["rho"], wrapped["rho"])


# ---- 3. a lone block equals the periodic tile group ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lone_sedov(exact):
    stats, f = run_block(test="Sedov", N=(48, 36), maxcycle=14, periodic=(True, True), exact_arithmetic=exact)
    return stats, f, stats.data.state_digest()


@pytest.mark.parametrize("exact", [False, True], ids=["tuned", "exact"])
@pytest.mark.parametrize("native", [False, True], ids=["host-driven", "native_cycle"])
@pytest.mark.parametrize("P", [(1, 1), (2, 2), (3, 1)], ids=str)
def test_a_lone_periodic_block_is_the_periodic_group(P, native, exact):
    stats, want, digest = lone_sedov(exact)
    assert stats.cycles == 14
    got_stats, got, got_digest = run_group(P, test="Sedov", N=(48, 36), maxcycle=14, periodic=(True, True), exact_arithmetic=exact,
                                           native_cycle=native)
    assert (got_stats.cycles, got_stats.final_time, got_stats.last_dt) == (stats.cycles, stats.final_time, stats.last_dt)
    for k in STATE:
        assert same_bits(got[k], want[k]), (k, float(np.abs(got[k] - want[k]).max()))
    assert got_digest == digest


# ---- 4. translation invariance --------------------------------------------------------------------------------------------------
NS = (24, 20)
SHIFT = (7, 5)


def smooth_state():
    """A smooth, doubly periodic state on the unit square (every field a few harmonics of the cell centres)."""
    nx, ny = NS
    x = ((np.arange(nx) + 0.5) / nx)[None, :]
    y = ((np.arange(ny) + 0.5) / ny)[:, None]
    s, c = lambda t: np.sin(2 * np.pi * t), lambda t: np.cos(2 * np.pi * t)
    rho = 1. + 0.3 * s(x) * c(y) + 0.1 * c(2 * x + y)
    u = 0.4 * c(x) + 0.2 * s(y - x)
    v = -0.3 * s(x + 2 * y) + 0.1 * c(y)
    p = 1. + 0.2 * c(x - y) + 0.1 * s(2 * x)
    return rho, u, v, p


def rolled(a):
    return np.roll(a, (SHIFT[1], SHIFT[0]), axis=(0, 1))


def smooth_problem(shift, boundaries="Periodic"):
    from armon_amd import Problem
    rho, u, v, p = (rolled(a) if shift else a for a in smooth_state())
    return Problem.from_arrays(rho, u, v, p=p, name="smooth", gamma=7 / 5, boundaries=boundaries, cfl=0.4, maxtime=10.)


TRANSLATION = [(s, c) for s in ("Sequential", "Strang", "SequentialSym") for c in (False, True)]


def oracle_from(oracle, problem, splitting, cst_dt, cycles=20):
    """The oracle's run from the bound problem's arrays (gamma = 7/5: the perfect gas of every built-in case; Sod_circ names
    the EOS only, both axes are periodic)."""
    nx, ny = NS
    bound = A().ArmonParameters(test=problem, N=NS).test
    f = oracle.alloc_fields(nx, ny, 4)
    _, f = oracle.solve(test="Sod_circ", N=NS, maxcycle=0, fields=f)          # x, y, mask
    for k in STATE:
        oracle.real_view(f[k], nx, ny, 4)[...] = bound.arrays[k]
    step = dict(cst_dt=True, Dt=2e-3) if cst_dt else dict(cfl=0.4)
    run, f = oracle.solve(test="Sod_circ", N=NS, maxcycle=cycles, maxtime=10., fields=f, skip_init=True, periodic=(True, True),
                          axis_splitting=splitting, **step)
    return run, {k: oracle.real_view(f[k], nx, ny, 4).copy() for k in STATE}


@pytest.mark.parametrize("splitting,cst_dt", TRANSLATION, ids=lambda v: v if isinstance(v, str) else ("cst_dt" if v else "cfl"))
def test_a_translated_state_gives_the_translated_run(oracle, splitting, cst_dt):
    step = dict(cst_dt=True, Dt=2e-3) if cst_dt else dict()
    kw = dict(N=NS, maxcycle=20, axis_splitting=splitting, **step)
    orun, oref = oracle_from(oracle, smooth_problem(False), splitting, cst_dt)
    orun_s, oref_s = oracle_from(oracle, smooth_problem(True), splitting, cst_dt)
    assert (orun.cycles, orun.last_dt, orun.final_time) == (orun_s.cycles, orun_s.last_dt, orun_s.final_time) and orun.cycles == 20
    assert all(same_bits(rolled(oref[k]), oref_s[k]) for k in STATE)          # the oracle is translation invariant
    for path, o in (("fused exact", dict(exact_arithmetic=True)), ("staged", dict(use_fused_sweep=False))):
        base, f = run_block(test=smooth_problem(False), **kw, **o)
        moved, f_s = run_block(test=smooth_problem(True), **kw, **o)
        assert (base.cycles, base.last_dt, base.final_time) == (moved.cycles, moved.last_dt, moved.final_time) == \
               (orun.cycles, orun.last_dt, orun.final_time), path
        for k in STATE:
            assert same_bits(rolled(f[k]), f_s[k]), (path, k)
            assert same_bits(f[k], oref[k]), (path, k)
    # tuned arithmetic: the oracle tolerance is asserted; whether the bits are equal as well is printed (pytest -s)
    base, f = run_block(test=smooth_problem(False), **kw)
    moved, f_s = run_block(test=smooth_problem(True), **kw)
    assert base.cycles == moved.cycles == orun.cycles
    assert abs(base.last_dt - orun.last_dt) <= 1e-12 * orun.last_dt and abs(moved.last_dt - orun.last_dt) <= 1e-12 * orun.last_dt
    equal = all(same_bits(rolled(f[k]), f_s[k]) for k in STATE) and base.last_dt == moved.last_dt
    print(f"\ntuned translation {splitting} {'cst_dt' if cst_dt else 'cfl'}: bits equal under the roll: {equal}")
    for k in STATE:
        scale = float(np.abs(oref[k]).max())
        assert np.abs(f[k] - oref[k]).max() <= 1e-11 * scale and np.abs(f_s[k] - oref_s[k]).max() <= 1e-11 * scale, k


# ---- 5. the pair path -----------------------------------------------------------------------------------------------------------
def test_an_x_periodic_block_keeps_the_pair_and_a_y_periodic_one_does_not():
    """A stream along x with a dense disc on the left edge: the sides are felt from the first cycle on (a wall stops the
    stream, a periodic side lets it through), so the wall run below really is another run."""
    from armon_amd import Disc, Problem, State
    from armon_amd.solver import pair_cycle
    stream = Problem("stream", State(1., u=1., v=0.2, p=1.), [(Disc((0.1, 0.5), r=0.2), State(2., u=1., v=0.2, p=1.))], cfl=0.4)
    kw = dict(test=stream, N=(512, 384), maxcycle=6)
    pair = dict(placement_min_bytes=1 << 20, placement_tries=1)
    single, f_single = run_block(periodic=(True, False), **kw)
    paired, f_pair = run_block(periodic=(True, False), **kw, **pair)
    assert single.data.pair_cycles == 0 and not pair_cycle(single.data.params, single.data)
    assert paired.data.pair_cycles == 6 and pair_cycle(paired.data.params, paired.data)
    assert (single.cycles, single.last_dt, single.final_time) == (paired.cycles, paired.last_dt, paired.final_time)
    for k in STATE:
        assert same_bits(f_pair[k], f_single[k]), k
    _, f_wall = run_block(**kw, **pair)
    assert not same_bits(f_wall["rho"], f_pair["rho"])
    for per in ((False, True), (True, True)):
        y, f_y = run_block(periodic=per, **kw, **pair)
        assert y.data.pair_cycles == 0 and y.data.pair_cells is None and not pair_cycle(y.data.params, y.data), per
        _, f_plain = run_block(periodic=per, **kw)
        assert all(same_bits(f_y[k], f_plain[k]) for k in STATE), per


# ---- 6. the density wave --------------------------------------------------------------------------------------------------------
def wave_problem(n, along):
    from armon_amd import Problem
    N = (n, 8) if along == "x" else (8, n)
    t = (np.arange(n) + 0.5) / n
    line = 1. + 0.2 * np.sin(2 * np.pi * t)
    rho = np.repeat(line[None, :], 8, axis=0) if along == "x" else np.repeat(line[:, None], 8, axis=1)
    one, zero = np.ones_like(rho), np.zeros_like(rho)
    u, v = (one, zero) if along == "x" else (zero, one)
    return N, Problem.from_arrays(rho, u, v, p=one, name="wave", gamma=7 / 5, boundaries="Periodic", cfl=0.5, maxtime=1.)


def wave_error(f, n, along, t_final):
    rho = f["rho"] if along == "x" else f["rho"].T
    assert all(same_bits(rho[0], rho[j]) for j in range(8))                   # rows identical
    t = (np.arange(n) + 0.5) / n
    return float(np.abs(rho[0] - (1. + 0.2 * np.sin(2 * np.pi * (t - t_final)))).mean())


@functools.lru_cache(maxsize=None)
def oracle_wave(n, along):
    from oracle import oracle as O
    N, problem = wave_problem(n, along)
    bound = A().ArmonParameters(test=problem, N=N).test
    f = O.alloc_fields(N[0], N[1], 4)
    _, f = O.solve(test="Sod_circ", N=N, maxcycle=0, fields=f)
    for k in STATE:
        O.real_view(f[k], N[0], N[1], 4)[...] = bound.arrays[k]
    run, f = O.solve(test="Sod_circ", N=N, cfl=0.5, maxtime=1., fields=f, skip_init=True, periodic=(True, True))
    return run, {k: O.real_view(f[k], N[0], N[1], 4).copy() for k in STATE}


@pytest.mark.parametrize("along", ["x", "y"])
def test_an_advected_density_wave_converges(oracle, along):
    """rho = 1 + 0.2 sin 2 pi x, u = 1, p = 1, doubly periodic, t = 1: one period. The CPU oracle gives mean|rho - rho0(x - t)|
    = 3.156e-3 at N = 64 and 8.995e-4 at 128 (297 and 595 cycles). The exact flavour gives the oracle's bits, so its errors;
    the tuned flavour's are printed (pytest -s)."""
    errors = {}
    for n in (64, 128):
        N, problem = wave_problem(n, along)
        orun, oref = oracle_wave(n, along)
        stats, f = run_block(test=problem, N=N, exact_arithmetic=True)
        assert (stats.cycles, stats.last_dt, stats.final_time) == (orun.cycles, orun.last_dt, orun.final_time)
        assert all(same_bits(f[k], oref[k]) for k in STATE)
        errors[n] = wave_error(f, n, along, stats.final_time)
        assert errors[n] == wave_error(oref, n, along, orun.final_time)
        across = f["u"] if along == "x" else f["v"]
        assert np.abs(across - 1.).max() < 3e-15
        tuned, g = run_block(test=problem, N=N)
        print(f"\ndensity wave along {along}, N = {n}: exact {errors[n]:.4e} ({stats.cycles} cycles), tuned "
              f"{wave_error(g, n, along, tuned.final_time):.4e} ({tuned.cycles} cycles)")
    assert errors[128] <= errors[64] / 3, errors
    assert abs(errors[64] - 3.156e-3) < 1e-6 and abs(errors[128] - 8.995e-4) < 1e-7, errors


# ---- 7. conservation ------------------------------------------------------------------------------------------------------------
def test_a_periodic_box_keeps_mass_and_momentum_and_a_wall_does_not(tmp_path):
    kw = dict(N=NS, maxcycle=20, history_step=1, exact_arithmetic=True)
    drift = {}
    for name in ("Periodic", "Dirichlet"):
        stats, _ = run_block(test=smooth_problem(False, boundaries=name), output_dir=str(tmp_path / name), **kw)
        h = stats.history
        assert h.cycle[0] == 0 and h.cycle[-1] == stats.cycles == 20
        mass, mx, my = (np.asarray(getattr(h, c), dtype=np.float64) for c in ("mass", "momentum_x", "momentum_y"))
        scale = float(np.abs(mass[0]))                                        # |momentum| <= max|u| mass < mass
        drift[name] = (abs(mass[-1] - mass[0]) / scale, max(abs(mx[-1] - mx[0]), abs(my[-1] - my[0])) / scale)
        print(f"\n{name}: relative drift of mass {drift[name][0]:.3e}, of momentum (by the mass) {drift[name][1]:.3e}")
    assert drift["Periodic"][0] <= 1e-12 and drift["Periodic"][1] <= 1e-12, drift
    assert drift["Dirichlet"][0] <= 1e-12 and drift["Dirichlet"][1] > 1e-6, drift     # the test can see a wall


# ---- 8. around the solver -------------------------------------------------------------------------------------------------------
def wrapped_difference(a, axis, h, T):
    """Central differences with wrap-around, in the data type: (a[i+1] - a[i-1]) / (2 h)."""
    return (np.roll(a, -1, axis=axis) - np.roll(a, 1, axis=axis)) / (T(2) * T(h))


def test_derived_fields_take_central_differences_across_a_periodic_edge():
    from armon_amd.multi_tile import TileGroup
    names = ["vorticity", "grad_rho", "divergence"]
    kw = dict(test="Sod_circ", N=(48, 36), maxcycle=10, periodic=(True, True), exact_arithmetic=True)
    stats, f = run_block(**kw)
    lone = stats.data.derive(names)
    group = TileGroup((2, 2), silent=5, **kw)
    try:
        group.run()
        tiles = group.derive(names)
    finally:
        group.close()
    T = np.float64
    dx, dy = stats.data.params.cell_size(0), stats.data.params.cell_size(1)
    gx, gy = wrapped_difference(f["rho"], 1, dx, T), wrapped_difference(f["rho"], 0, dy, T)
    want = {"vorticity": wrapped_difference(f["v"], 1, dx, T) - wrapped_difference(f["u"], 0, dy, T),
            "divergence": wrapped_difference(f["u"], 1, dx, T) + wrapped_difference(f["v"], 0, dy, T),
            "grad_rho": np.sqrt(gx * gx + gy * gy)}
    for q in names:
        assert same_bits(np.asarray(lone[q]), np.asarray(tiles[q])), q
        assert same_bits(np.asarray(lone[q]), want[q]), (q, float(np.abs(lone[q] - want[q]).max()))
    # with one periodic axis the other keeps its one-sided edges: the interior columns agree with the wrapped restatement
    stats, f = run_block(**{**kw, "periodic": (True, False)})
    half = stats.data.derive(["divergence"])["divergence"]
    full = wrapped_difference(f["u"], 1, dx, T) + wrapped_difference(f["v"], 0, dy, T)
    assert same_bits(np.asarray(half)[1:-1], full[1:-1]) and not same_bits(np.asarray(half)[0], full[0])


def test_a_lone_blocks_checkpoint_restarts_in_a_group_and_back(tmp_path):
    from armon_amd import SolverException
    kw = dict(test="Sedov", N=(48, 36), periodic=(True, False), maxcycle=16)
    whole, f_whole = run_block(**kw)
    run_block(checkpoint_step=10, output_dir=str(tmp_path), **kw)
    path = str(tmp_path / "checkpoint_000010.ckpt")
    stats, got, digest = run_group((2, 1), restart_from=path, **kw)
    assert digest == whole.data.state_digest() and stats.cycles == whole.cycles == 16
    assert all(same_bits(got[k], f_whole[k]) for k in STATE)
    # the reverse: the group's file into the lone block
    run_group((2, 1), checkpoint_step=10, checkpoint_file="group", output_dir=str(tmp_path), **kw)
    again, f_again = run_block(restart_from=str(tmp_path / "group_000010.ckpt"), **kw)
    assert again.data.state_digest() == whole.data.state_digest() and all(same_bits(f_again[k], f_whole[k]) for k in STATE)
    assert open(path, "rb").read() == open(tmp_path / "group_000010.ckpt", "rb").read()
    # other boundaries: refused, for a restart and for a comparison
    for other in ((False, False), (True, True)):
        with pytest.raises(SolverException) as e:
            run_block(restart_from=path, **{**kw, "periodic": other})
        assert e.value.category == "config" and "periodic" in str(e.value)
    walls, _ = run_block(**{**kw, "periodic": (False, False)})
    with pytest.raises(SolverException) as e:
        walls.data.compare_state(path)
    assert e.value.category == "config" and "periodic" in str(e.value)
    assert whole.data.compare_state(path) is not None


def test_gravity_in_a_periodic_channel_equals_its_group():
    from armon_amd import Disc, Problem, State
    channel = Problem("channel", State(1., p=1.), [(Disc((0.3, 0.6), r=0.2), State(2., u=0.3, p=1.5))],
                      boundaries=("Periodic", "Periodic", "Dirichlet", "Dirichlet"), gravity=(0., -0.1), cfl=0.4, maxtime=1.)
    kw = dict(test=channel, N=(48, 36), maxcycle=12)
    for o in (dict(), dict(exact_arithmetic=True)):
        stats, want = run_block(**kw, **o)
        assert stats.data.params.periodic == (True, False) and stats.data.params.forced
        got_stats, got, digest = run_group((2, 1), **kw, **o)
        assert (got_stats.cycles, got_stats.final_time, got_stats.last_dt) == (stats.cycles, stats.final_time, stats.last_dt)
        assert all(same_bits(got[k], want[k]) for k in STATE) and digest == stats.data.state_digest()


def test_the_in_situ_passes_run_on_a_periodic_block(tmp_path):
    kw = dict(test="Sod_circ", N=(48, 36), periodic=(True, True), maxcycle=8, output_dir=str(tmp_path))
    stats, f = run_block(profile_at_end=True, profile_kind="x", history_step=4, image_at_end=True, image_quantity=["vorticity"],
                         checkpoint_at_end=True, checkpoint_compress=True, check_result=True, **kw)
    grid = stats.data
    assert len(stats.profiles) == 1 and len(stats.images) == 1 and os.path.exists(stats.images[0])
    coarse = grid.coarsen(4)
    assert coarse["rho"].shape == (9, 12) and np.isfinite(coarse["rho"]).all()
    packed = str(tmp_path / "checkpoint_000008.ckpt")
    assert not grid.compare_state(packed).different                          # the packed file holds this very state
    again, f_again = run_block(restart_from=packed, **{**kw, "maxcycle": 12})
    whole, f_whole = run_block(**{**kw, "maxcycle": 12})
    assert all(same_bits(f_again[k], f_whole[k]) for k in STATE)


def test_graph_cycles_fall_back_to_the_host_driven_loop():
    kw = dict(test="Sod_circ", N=(48, 36), periodic=(True, True), maxcycle=12)
    plain, f = run_block(**kw)
    graph, g = run_block(graph_cycles=True, **kw)
    assert not hasattr(graph.data, "graph_report")
    assert (graph.cycles, graph.final_time, graph.last_dt) == (plain.cycles, plain.final_time, plain.last_dt)
    assert all(same_bits(f[k], g[k]) for k in STATE)
