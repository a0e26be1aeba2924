"""In-situ profiles, the host side (no GPU): the ABI, the argument checks, the fixed-point rule against exact rationals, the merge,
the file round trip and the run options."""
import ctypes as C
import math
import os
import random
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import armon_amd
from armon_amd import io as aio
from armon_amd import profile as prof
from armon_amd._lib import SIGNATURES, ProfileBin, ProfileSpec, SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import SolverStats, graph_cycles_usable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("profile_reset", "profile", "profile_f32", "profile_bounds", "profile_bounds_f32")


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "armon_hip.h")).read()
    L = armon_amd.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"ARMON_API int armon_hip_%s\(" % name, header), name
        assert "armon_hip_" + name in SIGNATURES
        assert getattr(L, "armon_hip_" + name).argtypes == SIGNATURES["armon_hip_" + name][1]
    assert "ARMON_PROFILE_X = 0, ARMON_PROFILE_Y = 1, ARMON_PROFILE_R = 2" in header
    assert "2^31" in header                                      # the limit on the cells of one bin is stated
    assert C.sizeof(ProfileBin) == 192 and C.sizeof(ProfileSpec) == 96
    assert ProfileSpec.scale_exp.offset == 72 and ProfileBin.rho_min.offset == 136


def good_spec(**kw):
    s = ProfileSpec()
    s.kind, s.eos, s.nbins, s.width = 2, 0, 10, 1
    s.cx, s.cy, s.dx, s.dy, s.inv_dr, s.gamma = 4.0, 4.0, 0.125, 0.125, 8.0, 1.4
    for k, v in kw.items():
        if k == "scale_exp":
            s.scale_exp[:] = v
        else:
            setattr(s, k, v)
    return s


def test_a_null_context_and_every_bad_argument_are_refused():
    L = armon_amd.lib()
    fake_ctx = C.create_string_buffer(4096)          # never dereferenced: every check below comes before the first use of the context
    ctx = C.cast(fake_ctx, C.c_void_p)
    data = C.cast(C.create_string_buffer(64), C.c_void_p)
    geometry = dict(row_length=16, nghost=4, nx=8, ny=8, col0=0, row0=0, wnx=8, wny=8, gcol=0, grow=0)

    def call(fn, ctx=ctx, spec=None, out=data, rho=data, **kw):
        g = {**geometry, **kw}
        spec = good_spec() if spec is None else spec
        return fn(ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], rho, data, data, data, g["col0"], g["row0"], g["wnx"], g["wny"],
                  g["gcol"], g["grow"], C.byref(spec) if spec is not False else None, out)

    inf, nan = math.inf, math.nan
    for name in ("profile", "profile_f32", "profile_bounds", "profile_bounds_f32"):
        fn = getattr(L, "armon_hip_" + name)
        assert call(fn, ctx=None) == 1, name
        assert b"ctx" in L.armon_hip_last_error()
        # the window rules of state_pack
        for bad in (dict(nx=0), dict(ny=0), dict(nghost=-1), dict(row_length=15), dict(col0=-1), dict(row0=-1), dict(wnx=0), dict(wny=0),
                    dict(col0=1), dict(row0=1), dict(wnx=9), dict(wny=9), dict(nx=1 << 31, row_length=(1 << 31) + 8),
                    dict(gcol=-1), dict(grow=-1)):
            assert call(fn, **bad) == 1, (name, bad)
        assert call(fn, rho=None) == 1 and call(fn, out=None) == 1 and call(fn, spec=False) == 1
        # the spec
        for bad in (dict(nbins=0), dict(nbins=-3), dict(width=0), dict(kind=3), dict(kind=-1), dict(eos=2), dict(eos=-2),
                    dict(dx=0.0), dict(dx=-1.0), dict(dx=inf), dict(dx=nan), dict(dy=0.0), dict(dy=inf), dict(dy=nan),
                    dict(inv_dr=0.0), dict(inv_dr=-2.0), dict(inv_dr=inf), dict(inv_dr=nan), dict(cx=nan), dict(cy=inf),
                    dict(scale_exp=[0, 0, 5000, 0, 0])):
            assert call(fn, spec=good_spec(**bad)) == 1, (name, bad)
    assert L.armon_hip_profile_reset(None, 4, data) == 1
    assert L.armon_hip_profile_reset(ctx, 0, data) == 1 and L.armon_hip_profile_reset(ctx, 4, None) == 1


def exact(t, s):
    """round-half-even(t / 2^s) by exact rationals (Python rounds a Fraction half to even)."""
    return round(Fraction(t) / Fraction(2) ** s)


def test_quantise_against_exact_rationals():
    rng = random.Random(20261018)
    draws = []
    for _ in range(3000):
        e, s = rng.randint(-1074, 200), rng.randint(-1100, 150)
        t = math.ldexp(rng.uniform(-1, 1), e)
        draws.append((t, s))
        draws.append((t, math.frexp(t)[1] - rng.randint(0, 100)))        # the quantum within reach of the value
    for t, s in draws:
        Q = exact(t, s)
        assert prof.quantise(t, s) == (Q if abs(Q) < 1 << 95 else None), (t.hex(), s)
    # ties go to even, on both sides of zero
    for k, want in ((0.5, 0), (1.5, 2), (2.5, 2), (3.5, 4), (-0.5, 0), (-1.5, -2), (-2.5, -2), (6.5, 6), (7.5, 8)):
        for s in (-30, 0, 17):
            assert prof.quantise(math.ldexp(k, s), s) == want
    assert prof.quantise(math.ldexp(1 + 2 ** -52, 52), 53) == 1 and prof.quantise(math.ldexp(1.0, 52), 53) == 0      # just above a tie; the tie
    # subnormals, exactly representable at the finest quantum
    assert prof.quantise(5e-324, -1074) == 1 and prof.quantise(-5e-324, -1074) == -1 and prof.quantise(5e-324, -1073) == 0
    assert prof.quantise(3 * 5e-324, -1073) == 2 and prof.quantise(2.5e-310, -1074) == exact(2.5e-310, -1074)
    # far below the quantum
    assert prof.quantise(1e-300, 0) == 0 and prof.quantise(-1e-300, -900) == 0 and prof.quantise(0.0, 5) == 0 and prof.quantise(-0.0, 5) == 0
    # the 2^95 edge: the last value below it is good, the edge itself and a value that rounds up to it are bad
    below = math.ldexp(1 - 2 ** -53, 95)
    assert prof.quantise(below, 0) == (1 << 95) - (1 << 42) and prof.quantise(-below, 0) == -((1 << 95) - (1 << 42))
    assert prof.quantise(math.ldexp(1.0, 95), 0) is None and prof.quantise(-math.ldexp(1.0, 95), 0) is None
    assert prof.quantise(1.0, -95) is None and prof.quantise(1.0, -94) == 1 << 94 and prof.quantise(1e300, -4096) is None
    for t in (math.inf, -math.inf, math.nan):
        assert prof.quantise(t, 0) is None
    # the default scale keeps the largest term below 2^94
    for t in (1.0, 0.999, 1e11, 3e-7, 5e-324):
        s = prof.default_scale([int(np.array([abs(t)]).view(np.uint64)[0])] * 5)[0]
        assert 1 << 93 <= abs(prof.quantise(t, s)) < 1 << 94 or t == 5e-324
    assert prof.default_scale([0] * 5) == (-94,) * 5


def test_quantise_limbs_is_the_scalar_rule():
    """The one vectorised quantiser (the oracle of the profile, analytic and history records) against ``quantise`` and ``limbs``,
    over magnitudes and scales on both sides of the quantum, shifts up to the 2^95 edge included."""
    rng, nrng = random.Random(20261018), np.random.default_rng(5)
    values = [math.ldexp(rng.uniform(-1, 1), rng.randint(-120, 40)) for _ in range(4000)]
    values += (nrng.standard_normal(600) * 10.0 ** nrng.integers(-30, 30, 600)).tolist()
    values += [0.0, -0.0, math.inf, -math.inf, math.nan, 5e-324, -5e-324, 0.5, 1.5, 2.5, -2.5, math.ldexp(1.0, 33), 1e308, 2.0 ** 40,
               -2.0 ** 41 + 1]
    t = np.array(values)
    for s in (-1070, -130, -94, -80, -62, -60, -40, -20, -3, 0, 1, 5, 7, 900):
        l0, l1, l2, ok = prof.quantise_limbs(t, s)
        for i, x in enumerate(values):
            Q = prof.quantise(x, s)
            assert bool(ok[i]) == (Q is not None), (x, s)
            if Q is not None:
                got = (int(l0[i]), int(l1[i]), int(l2[i]))
                assert got == prof.limbs(abs(Q)) and prof.from_limbs(got) == abs(Q), (x, s)
                assert prof.from_limbs(prof.limbs(Q)) == Q and all(abs(l) < 1 << 32 for l in prof.limbs(Q))


def test_limbs_round_trip():
    rng = random.Random(7)
    for Q in [0, 1, -1, (1 << 32) - 1, 1 << 32, -(1 << 32), (1 << 64) - 1, 1 << 64, (1 << 95) - 1, -((1 << 95) - 1)] + \
            [rng.randint(-(1 << 95) + 1, (1 << 95) - 1) for _ in range(500)]:
        l = prof.limbs(Q)
        assert prof.from_limbs(l) == Q and all(abs(v) < 1 << 32 for v in l) and all(v * Q >= 0 for v in l)
    # the limbs of a sum are not the sum of the limbs: why the record keeps the per-cell limbs apart
    assert tuple(a + b for a, b in zip(prof.limbs(1 << 32), prof.limbs(-1))) == (-1, 1, 0) != prof.limbs((1 << 32) - 1)


def test_order_keys():
    values = [-math.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, math.inf]
    keys = [prof.order_key(v) for v in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)              # -0.0 orders below +0.0
    for v in values:
        assert np.array([prof.from_key(prof.order_key(v))]).tobytes() == np.array([v]).tobytes()


def drawn_profile(rng, spec, scale):
    raw = prof.neutral(spec[2])
    for b in range(spec[2]):
        if rng.random() < 0.2:
            continue
        raw[b, :17] = [rng.getrandbits(64) for _ in range(17)]
        raw[b, 17:21] = [rng.getrandbits(64) for _ in range(4)]
    return prof.Profile(raw, spec, scale)


def test_merge_is_associative_and_commutative_and_refuses_mismatches():
    rng = random.Random(3)
    spec = (2, 0, 9, 1, 4.0, 4.0, 0.125, 0.125, 8.0, 1.4)
    scale = (-90, -91, -92, -93, -94)
    a, b, c = (drawn_profile(rng, spec, scale) for _ in range(3))
    assert a.merge(b) == b.merge(a)
    assert a.merge(b).merge(c) == a.merge(b.merge(c)) == c.merge(a).merge(b)
    zero = prof.Profile(prof.neutral(9), spec, scale)
    assert a.merge(zero) == a and zero.merge(zero) == zero
    for other in (prof.Profile(prof.neutral(9), (0,) + spec[1:], scale), prof.Profile(prof.neutral(9), spec[:1] + (-1,) + spec[2:], scale),
                  prof.Profile(prof.neutral(8), spec[:2] + (8,) + spec[3:], scale), prof.Profile(prof.neutral(9), spec[:8] + (4.0,) + spec[9:], scale),
                  prof.Profile(prof.neutral(9), spec, (-90, -91, -92, -93, -95))):
        with pytest.raises(SolverException) as e:
            a.merge(other)
        assert e.value.category == "config"


def test_the_reference_record_decodes_to_the_means():
    """A hand-made 2 x 3 state, kind x: exact sums, means rounded once, extrema, an empty bin, a bad cell."""
    rho = np.array([[1.0, 2.0, 0.1], [3.0, 2.0, math.nan]])
    u = np.array([[0.5, -1.0, 0.3], [0.25, 1.0, 0.0]])
    v = np.zeros((2, 3))
    E = np.array([[2.0, 2.0, 0.7], [2.0, 4.0, 1.0]])
    p = np.array([[1.0, -0.0, 0.2], [3.0, 0.0, 1.0]])
    scale = (-60,) * 5
    raw = prof.reference_record("x", 4, scale, rho, u, v, E, p)
    P = prof.Profile(raw, (0, 0, 4, 1, 0.0, 0.0, 0.5, 0.5, 1.0, 1.4), scale, origin=(10.0, 0.0))
    assert P.n.tolist() == [2, 2, 1, 0] and P.n_bad.tolist() == [0, 0, 1, 0]
    assert P.sums[0][:2] == [4 << 60, 4 << 60] and P.sums[1][:2] == [(5 << 60) // 4, 0] and P.sums[0][2] == prof.quantise(0.1, -60)
    assert P.rho.tolist()[:2] == [2.0, 2.0] and P.un.tolist()[0] == 1.25 / 4 and P.E.tolist()[1] == 3.0 and P.p.tolist()[0] == 2.0
    assert P.rho[2] == float(Fraction(prof.quantise(0.1, -60), 1 << 60)) and math.isnan(P.rho[3]) and math.isnan(P.un[3])
    assert math.isnan(P.un[1]) is False and P.un[1] == 0.0
    assert P.rho_min.tolist()[:3] == [1.0, 2.0, 0.1] and P.rho_max.tolist()[:3] == [3.0, 2.0, 0.1] and math.isnan(P.rho_min[3])
    assert np.array([P.p_min[1]]).tobytes() == np.array([-0.0]).tobytes() and np.array([P.p_max[1]]).tobytes() == np.array([0.0]).tobytes()
    assert P.coord.tolist() == [10.25, 10.75, 11.25, 11.75]
    assert "2 cells" not in P.report() and "5 cells, 1 bad" in P.report()
    # without p the fifth sum and its extrema stay neutral
    raw = prof.reference_record("y", 2, scale, rho, u, v, E, None)
    assert not raw[:, 14:17].any() and (raw[:, 19] == prof.MASK).all() and not raw[:, 20].any() and raw[:, 0].tolist() == [3, 2]


def same_table(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() or np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def test_the_file_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    rho, E = rng.uniform(0.1, 2, (6, 5)), rng.uniform(1, 3, (6, 5))
    u, v, p = rng.normal(0, 1, (6, 5)), rng.normal(0, 1e-200, (6, 5)), rng.uniform(0, 1e11, (6, 5))
    scale = (-90, -90, -290, -90, -50)
    geometry = dict(cx=2.3, cy=3.1, dx=0.2, dy=0.25, inv_dr=1 / 0.3)
    for kind, spec in (("r", (2, 0, 7, 1, 2.3, 3.1, 0.2, 0.25, 1 / 0.3, 1.4)), ("x", (0, 0, 4, 2, 0.0, 0.0, 0.2, 0.25, 1.0, 1.4))):
        raw = prof.reference_record(kind, spec[2], scale, rho, u, v, E, p, **(geometry if kind == "r" else dict(width=2)))
        P = prof.Profile(raw, spec, scale, origin=(-1.0, 0.5), cycle=12, time=0.1234567890123)
        path = str(tmp_path / f"p_{kind}.txt")
        aio.write_profile_file(path, P, 17)
        same_table(aio.read_profile_file(path), P.table())
        assert len(open(path).read().splitlines()) == 2 + spec[2]
    assert math.isnan(P.table()["rho"][3]) and P.table()["n"][3] == 0      # (x, width 2, 5 columns: the fourth bin is empty)


def test_option_defaults_and_configuration_errors():
    p = ArmonParameters(test="Sod", N=(8, 8))
    assert (p.profile_step, p.profile_kind, p.profile_bins, p.profile_width, p.profile_centre, p.profile_dr, p.profile_file,
            p.profile_at_end, p.state_profile) == (0, "x", None, 1, None, None, "profile", False, False)
    assert p.use_fused_sweep and not p.state_compare and p.checkpoint_step == 0
    p = ArmonParameters(test="Sedov", N=(8, 8), profile_step=3, profile_kind="r", profile_dr=0.1, profile_centre=(0.1, 0.2), profile_bins=5,
                        output_dir="out", profile_file="ring")
    assert p.state_profile and p.use_fused_sweep and prof.profile_path(p, 12) == "out/ring_000012.txt"
    for bad in (dict(profile_step=-1), dict(profile_step=1.5), dict(profile_step=True), dict(profile_step="2"), dict(profile_kind="z"),
                dict(profile_kind="R"), dict(profile_width=0), dict(profile_width=-2), dict(profile_width=1.5), dict(profile_dr=0.0),
                dict(profile_dr=-0.1), dict(profile_dr=float("nan")), dict(profile_dr=float("inf")), dict(profile_bins=0),
                dict(profile_file=""), dict(profile_file="a/b"), dict(profile_centre=(0.0,)), dict(profile_centre=(0.0, float("nan")))):
        with pytest.raises(SolverException) as e:
            ArmonParameters(test="Sod", N=(8, 8), **bad)
        assert e.value.category == "config", bad


def test_the_options_are_refused_for_ranks(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    ArmonParameters(test="Sod", N=(8, 8), use_MPI=True)
    for opts in (dict(profile_step=2), dict(profile_at_end=True)):
        with pytest.raises(SolverException) as e:
            ArmonParameters(test="Sod", N=(8, 8), use_MPI=True, **opts)
        assert e.value.category == "config" and "use_MPI" in e.value.msg


def test_graph_replay_steps_aside_and_stats_default():
    def usable(**kw):
        p = ArmonParameters(test="Sod", N=(8, 8), graph_cycles=True, silent=5, **kw)
        p._device = types.SimpleNamespace(owns_ctx=True)
        return graph_cycles_usable(p)
    assert usable() is True
    assert usable(profile_step=2) is False and usable(profile_at_end=True) is False
    assert usable(profile_kind="r", profile_dr=0.5) is True              # the other options alone ask for nothing
    assert SolverStats(0.0, 0.0, 0, 0.0, 0, 0.0).profiles == []


def test_the_default_binning():
    p = ArmonParameters(test="Sedov", N=(10, 6))                         # the domain [-1, 1]^2
    dx, dy = float(p.cell_size(0)), float(p.cell_size(1))
    assert prof.make_spec(p, "x", width=4)[:4] == (0, 0, 3, 4) and prof.make_spec(p, "y", with_p=False)[:4] == (1, -1, 6, 1)
    s = prof.make_spec(p, "r")
    assert (s[4], s[5]) == (5.0, 3.0) and s[8] == 1.0 / min(dx, dy)
    far = math.hypot(5 * dx, 3 * dy)
    assert s[2] == math.floor(far / min(dx, dy)) + 1                      # reaches the farthest corner
    s = prof.make_spec(p, "r", centre=(p.origin[0] + 0.33, p.origin[1] + 0.1), dr=0.05, bins=7)
    assert s[2] == 7 and s[8] == 1 / 0.05
    assert s[4] == ((p.origin[0] + 0.33) - p.origin[0]) / dx and s[5] == ((p.origin[1] + 0.1) - p.origin[1]) / dy
    assert prof.make_spec(ArmonParameters(test="Bizarrium", N=(8, 8)), "x")[1] == 1
    for bad in (dict(kind="q"), dict(kind="x", width=0), dict(kind="r", dr=0.0), dict(kind="x", bins=0)):
        with pytest.raises(SolverException):
            prof.make_spec(p, **bad)
