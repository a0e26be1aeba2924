"""Body forces without a GPU: the ``gravity`` option of ``Problem`` and ``ArmonParameters`` — validation,
rounding, what it switches off — the problem digest and the checkpoint header with and without a force, and the restated
kick (tests/body_force_restated.py) against exact rational arithmetic."""
import hashlib
import json
import math
from fractions import Fraction

import numpy as np
import pytest

import armon_amd
from armon_amd import ArmonParameters, HalfPlane, Problem, SolverException, State
from armon_amd import analytic, checkpoint

import body_force_restated as BF


def layers(**kw):
    return Problem("layers", State(1., p=1.), [(HalfPlane((0, 1), 0.5), State(2., p=1.))], **kw)


def config_error(fn):
    with pytest.raises(SolverException) as e:
        fn()
    assert e.value.category == "config", e.value
    return str(e.value)


# ---- the option ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [None, 1., (1.,), (1., 2., 3.), "ab", ("1", 0.), (True, 0.), (0., None), (math.nan, 0.),
                                 (0., math.inf), (-math.inf, 0.), [(0., 1.), 0.]], ids=repr)
def test_gravity_takes_two_finite_numbers(bad):
    assert "gravity" in config_error(lambda: layers(gravity=bad))
    if bad is not None:                                         # (None = "not given" for the option of ArmonParameters)
        assert "gravity" in config_error(lambda: ArmonParameters(test="Sod", N=(8, 8), gravity=bad))
        assert "gravity" in config_error(lambda: ArmonParameters(test=layers(), N=(8, 8), gravity=bad))


def test_a_value_that_overflows_the_data_type_is_refused():
    ArmonParameters(test="Sod", N=(8, 8), gravity=(0., 1e300))
    assert "float32" in config_error(lambda: ArmonParameters(test="Sod", N=(8, 8), gravity=(0., 1e300), data_type=np.float32))
    assert "float32" in config_error(lambda: ArmonParameters(test=layers(gravity=(-1e300, 0.)), N=(8, 8), data_type=np.float32))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_values_are_rounded_to_the_data_type_when_bound(dtype):
    g = (0.1, -1. / 3.)
    want = tuple(float(dtype(v)) for v in g)
    for params in (ArmonParameters(test=layers(gravity=g), N=(8, 8), data_type=dtype),
                   ArmonParameters(test=layers(), N=(8, 8), data_type=dtype, gravity=g),
                   ArmonParameters(test="Sod", N=(8, 8), data_type=dtype, gravity=g)):
        assert params.test.gravity == want and params.gravity == want and params.forced
        assert all(isinstance(v, float) for v in params.test.gravity)
    assert (want != g) == (dtype is np.float32)
    # a value below the data type's range is no force at all; a negative zero is a zero
    tiny = ArmonParameters(test=layers(gravity=(1e-60, -0.)), N=(8, 8), data_type=np.float32)
    assert tiny.test.gravity == (0., 0.) and not tiny.forced and math.copysign(1., tiny.test.gravity[1]) == 1.


def test_the_option_overrides_the_problem_and_defaults_to_it():
    P = layers(gravity=(0., -1.))
    assert P.gravity == (0., -1.) and layers().gravity == (0., 0.)
    assert ArmonParameters(test=P, N=(8, 8)).test.gravity == (0., -1.)
    assert ArmonParameters(test=P, N=(8, 8), gravity=(2., 0.)).test.gravity == (2., 0.)
    off = ArmonParameters(test=P, N=(8, 8), gravity=(0., 0.))
    assert off.test.gravity == (0., 0.) and not off.forced and off.test.conservative
    plain = ArmonParameters(test="Sod", N=(8, 8))
    assert plain.test.gravity == (0., 0.) and not plain.forced


def test_a_forced_run_is_not_held_to_conservation():
    assert ArmonParameters(test=layers(), N=(8, 8)).test.conservative
    assert ArmonParameters(test="Sod", N=(8, 8)).test.conservative
    for g in ((0., -1.), (1e-3, 0.), (2., 3.)):
        assert not ArmonParameters(test=layers(gravity=g), N=(8, 8)).test.conservative
        assert not ArmonParameters(test=layers(), N=(8, 8), gravity=g).test.conservative
        assert not ArmonParameters(test="Sod", N=(8, 8), gravity=g).test.conservative
    # a problem that gave conservation up on its own does not get it back
    assert not ArmonParameters(test=layers(conservative=False), N=(8, 8), gravity=(0., 0.)).test.conservative


def test_no_closed_form_under_a_force():
    sod = Problem.like("Sod")
    free = ArmonParameters(test=sod, N=(16, 16))
    assert analytic.has_closed_form(free.test) and analytic.reference_for(free, 0.05) is not None
    for params in (ArmonParameters(test=sod, N=(16, 16), gravity=(0., -1.)), ArmonParameters(test="Sod", N=(16, 16), gravity=(0.5, 0.)),
                   ArmonParameters(test="Sedov", N=(16, 16), gravity=(0., 1e-3))):
        assert not analytic.has_closed_form(params.test)
        with pytest.raises(SolverException) as e:
            analytic.reference_for(params, 0.05)
        assert e.value.category == "analytic" and "no closed-form" in str(e.value)
    assert "closed form" in config_error(lambda: ArmonParameters(test="Sod", N=(16, 16), gravity=(0., -1.), error_norms_at_end=True))


def test_bizarrium_may_be_forced():
    """No path reads a stored p after the cycle (DESIGN.md §4.12 says what was checked), so the combination is allowed."""
    params = ArmonParameters(test="Bizarrium", N=(16, 16), gravity=(0., -9.81))
    assert params.test.eos == "bizarrium" and params.forced
    P = Problem("b", State(1e4, E=1e6), eos="bizarrium", gravity=(1., 1.))
    assert ArmonParameters(test=P, N=(8, 8)).test.gravity == (1., 1.)


def test_graph_cycles_fall_back_under_a_force():
    from armon_amd.solver import graph_cycles_usable
    on = dict(test="Sod", N=(16, 16), silent=5, graph_cycles=True)
    assert not graph_cycles_usable(ArmonParameters(gravity=(0., -1.), **on))
    # (without a force the answer needs a device: `owns_ctx`; the GPU tests cover it)


# ---- digest and header -------------------------------------------------------------------------------------------------------
PARENT_KEYS = ("arrays", "background", "boundaries", "eos", "gamma", "regions", "samples")       # what the digest held before


def parent_digest(test):
    """sha256 of the canonical JSON of the description as it was before the option existed: exactly those seven keys."""
    d = {k: test.description[k] for k in PARENT_KEYS}
    return hashlib.sha256(json.dumps(d, sort_keys=True).encode("utf-8")).hexdigest()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_without_a_force_digest_and_header_are_the_parents(dtype):
    kw = dict(N=(16, 12), data_type=dtype)
    rho = np.ones((12, 16))
    problems = {"regions": lambda **g: layers(**g), "preset": lambda **g: Problem.like("Sedov"),
                "arrays": lambda **g: Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, **g)}
    for name, make in problems.items():
        plain = ArmonParameters(test=make(), **kw)
        zero = ArmonParameters(test=make(gravity=(0., 0.)), gravity=(0., -0.), **kw)
        assert sorted(plain.test.description) == sorted(PARENT_KEYS), name
        assert plain.test.digest == zero.test.digest == parent_digest(plain.test), name
        h_plain, h_zero = checkpoint.bit_options(plain), checkpoint.bit_options(zero)
        assert "gravity" not in h_plain and h_plain == h_zero, name
        assert sorted(h_plain) == sorted(checkpoint.BIT_FIELDS + checkpoint.PROBLEM_FIELDS), name
        assert json.dumps(h_plain, sort_keys=True) == json.dumps(h_zero, sort_keys=True)
    for case in ("Sod", "Bizarrium"):
        h = checkpoint.bit_options(ArmonParameters(test=case, **kw))
        assert h == checkpoint.bit_options(ArmonParameters(test=case, gravity=(0., 0.), **kw))
        assert sorted(h) == sorted(checkpoint.BIT_FIELDS)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_with_a_force_digest_and_header_differ_and_carry_what_the_device_receives(dtype):
    kw = dict(N=(16, 12), data_type=dtype)
    g = (0.1, -1. / 3.)
    plain = ArmonParameters(test=layers(), **kw)
    forced = ArmonParameters(test=layers(gravity=g), **kw)
    assert forced.test.digest != plain.test.digest != ""
    assert forced.test.digest == ArmonParameters(test=layers(), gravity=g, **kw).test.digest
    assert forced.test.digest != ArmonParameters(test=layers(gravity=(g[1], g[0])), **kw).test.digest
    assert forced.test.description["gravity"] == [float(dtype(v)).hex() for v in g]
    assert parent_digest(forced.test) == plain.test.digest           # nothing else moved
    h = checkpoint.bit_options(forced)
    assert h["gravity"] == [float(dtype(v)).hex() for v in g]
    rest = {k: v for k, v in h.items() if k not in ("gravity", "problem_digest")}
    assert rest == {k: v for k, v in checkpoint.bit_options(plain).items() if k != "problem_digest"}
    built_in = checkpoint.bit_options(ArmonParameters(test="Sod", gravity=(0., -1.), **kw))
    assert built_in["gravity"] == [float(0.).hex(), float(-1.).hex()] and built_in["test"] == "Sod"


def header_of(params):
    h = dict(checkpoint.bit_options(params))
    h.update(cycle=3, time=float(0.01).hex())
    return h


def test_check_compatible_refuses_another_force():
    kw = dict(N=(16, 12), maxcycle=10)
    for make in (lambda **o: ArmonParameters(test="Sod", **kw, **o), lambda **o: ArmonParameters(test=layers(), **kw, **o)):
        plain, down, up = make(), make(gravity=(0., -1.)), make(gravity=(0., 1.))
        for params in (plain, down, up):
            checkpoint.check_compatible(params, header_of(params), "f.ckpt")
        checkpoint.check_compatible(plain, header_of(make(gravity=(0., 0.))), "f.ckpt")      # a missing key is (0, 0)
        for run, file in ((down, plain), (plain, down), (up, down), (down, make(gravity=(-1., 0.)))):
            msg = config_error(lambda: checkpoint.check_compatible(run, header_of(file), "f.ckpt"))
            assert "gravity" in msg, msg


def test_a_damaged_gravity_key_is_an_io_error():
    params = ArmonParameters(test="Sod", N=(8, 8), gravity=(0., -1.))
    good = dict(checkpoint.bit_options(params), planes=["rho"], digests={"rho": "0"}, cycle=0, time="0x0p+0", current_dt="0x0p+0",
                next_cycle_dt="0x0p+0", pending_dt=None)
    checkpoint._check_header(good, "f.ckpt")
    for bad in ([1., 2.], ["0x1p+0"], "0x1p+0", ["0x1p+0", "zz"], None):
        with pytest.raises(SolverException) as e:
            checkpoint._check_header(dict(good, gravity=bad), "f.ckpt")
        assert e.value.category == "io" and "gravity" in str(e.value)


# ---- the library's host side ----------------------------------------------------------------------------------------------------
def test_the_cycles_kick_arithmetic_under_sanitizers(tmp_path):
    """csrc/cycle_kick.hpp — which cells a tile of armon_hip_mgpu_cycle kicks and with which step — is plain C++: run on the
    CPU as a program of its own under ASan / UBSan, like the tile pool (tests/test_tile_pool.py)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cycle_kick_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", os.path.join(root, "tests", "native", "cycle_kick_test.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and "cycle_kick OK" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]


def test_the_groups_force_is_refused_without_a_group():
    import ctypes as C
    L = armon_amd.lib()
    assert L.armon_hip_mgpu_set_body_force(None, C.c_double(0.), C.c_double(-1.)) != 0
    assert b"NULL" in L.armon_hip_last_error()


# ---- the restated kick -------------------------------------------------------------------------------------------------------
def exact_internal(u, v, E):
    return [Fraction(float(e)) - (Fraction(float(a)) ** 2 + Fraction(float(b)) ** 2) / 2 for a, b, e in zip(u, v, E)]


@pytest.mark.parametrize("force", [(3., 0.), (0., -9.81), (2.5, -7.)], ids=str)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_kick_leaves_the_internal_energy_alone_to_rounding(dtype, force):
    """e = E - (u² + v²) / 2 before and after the restated kick, both evaluated in exact rational arithmetic on the stored values.

    The bound. Write r = eps / 2 for the unit roundoff, a = dt gx in exact arithmetic and a~ = fl(a) = a (1 + e1). The kick
    stores hx = fl((dt / 2) gx) = a~ / 2 (the halving is exact) and u' = fl(u + a~) = u* (1 + e2) with u* = u + a~. For u* the
    kinetic energy changes by (u*² - u²) / 2 = a~ (u + a~ / 2) = a~ (u + hx) EXACTLY: that is why the formula has no
    cancellation. What the kick adds instead is fl(dt fl(fl(gx fl(u + hx)) + the same in y)), which differs from
    Wx + Wy, Wx = a~ (u + hx), by five roundings: a for a~ (e1, on Wx), the sum u + hx and the product by gx (on Wx), the sum
    of the two components and the product by dt (on Wx + Wy) — and likewise in y: at most 5 r (|Wx| + |Wy|) to first order.
    Storing u' instead of u* moves its kinetic energy by u*² e2: at most r u'² (and r v'²), and the final sum E + dE is
    rounded once: r |E'|. Together |e' - e| <= r (|E'| + u'² + v'² + 5 (|Wx| + |Wy|)), to which 1 % is added for the terms of
    second order. With these states the bound is at most 1.7 ulp of E (asserted below: under 4)."""
    T = np.dtype(dtype).type
    rng = np.random.default_rng(7)
    n = 400
    u, v = rng.uniform(-1, 1, n).astype(T), rng.uniform(-1, 1, n).astype(T)
    E = rng.uniform(2., 4., n).astype(T)
    u[:3], v[:3] = T(0), T(-0.)
    dt = T(0.0123)
    gx, gy = T(force[0]), T(force[1])
    u1, v1, E1 = BF.kick(u, v, E, dt, gx, gy)
    assert (u1 is u) == (gx == 0) and (v1 is v) == (gy == 0)          # the plane of a zero component is the same object
    r = Fraction(float(np.finfo(T).eps)) / 2
    before, after = exact_internal(u, v, E), exact_internal(u1, v1, E1)
    worst = 0.
    for k in range(n):
        a, b = Fraction(float(dt * gx)), Fraction(float(dt * gy))
        Wx, Wy = a * (Fraction(float(u[k])) + a / 2), b * (Fraction(float(v[k])) + b / 2)
        bound = r * (abs(Fraction(float(E1[k]))) + Fraction(float(u1[k])) ** 2 + Fraction(float(v1[k])) ** 2 + 5 * (abs(Wx) + abs(Wy)))
        bound *= Fraction(101, 100)
        assert abs(after[k] - before[k]) <= bound, (k, float(after[k] - before[k]), float(bound))
        worst = max(worst, float(bound / (r * 2 * abs(Fraction(float(E[k]))))))
    assert worst < 4.                                                    # "a few ulp of E": the bound itself is that small
    # and the velocities are what they should be
    assert np.array_equal(u1, u + dt * gx) and np.array_equal(v1, v + dt * gy)


def test_a_zero_force_returns_the_arrays_themselves():
    u, v, E = (np.full(4, x) for x in (-0., 1., 2.))
    assert all(a is b for a, b in zip(BF.kick(u, v, E, 0.1, 0., -0.), (u, v, E)))
    f = {k: np.arange(36.) for k in ("u", "v", "E")}
    BF.kick_real(f, 2, 2, 2, 0.5, 0., 2.)
    assert np.array_equal(f["u"], np.arange(36.))
    changed = np.flatnonzero(f["v"] != np.arange(36.))
    assert list(changed) == [14, 15, 20, 21] and np.array_equal(f["v"][changed], np.arange(36.)[changed] + 1.)
