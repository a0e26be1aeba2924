"""Run history, the host side (no GPU): the ABI, the rule in Python on hand-made states, the merge, the default scale, the file
and its restart handling, and the run options."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import armon_amd
from armon_amd import history as H
from armon_amd import io as aio
from armon_amd import profile as prof
from armon_amd._lib import SIGNATURES, HistoryRecord, HistorySpec, SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import SolverStats, graph_cycles_usable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("history_create", "history_destroy", "history_set_gauges", "history_sample", "history_sample_f32", "history_read")


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "armon_hip.h")).read()
    L = armon_amd.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"ARMON_API int armon_hip_%s\(" % name, header), name
        assert "armon_hip_" + name in SIGNATURES
        assert getattr(L, "armon_hip_" + name).argtypes == SIGNATURES["armon_hip_" + name][1]
    assert C.sizeof(HistoryRecord) == 320 == 8 * H.WORDS
    assert HistoryRecord.sum.offset == 8 * H.W_SUM and HistoryRecord.ext.offset == 8 * H.W_EXT and HistoryRecord.reserved.offset == 288
    assert C.sizeof(HistorySpec) == 48 and HistorySpec.scale_exp.offset == 24
    assert "#define ARMON_HISTORY_MAX_GAUGES 64" in header and H.MAX_GAUGES == 64


def perfect_gas(rho, u, v, E, gamma=1.4):
    """p, c of the perfect gas in the arrays' own type, operation for operation as the EOS kernel."""
    T = rho.dtype.type
    with np.errstate(all="ignore"):
        e = E - T(0.5) * (u * u + v * v)
        p = (T(gamma) - T(1.)) * rho * e
        return p, np.sqrt(T(gamma) * p / rho)


def hand_state(ny=4, nx=6, dtype=np.float64):
    rho = np.full((ny, nx), 1.0, dtype=dtype)
    u = np.zeros((ny, nx), dtype=dtype)
    v = np.zeros((ny, nx), dtype=dtype)
    E = np.full((ny, nx), 2.5, dtype=dtype)
    return rho, u, v, E


def record_of(rho, u, v, E, scale=(-60,) * 6, **kw):
    p, c = perfect_gas(rho, u, v, E)
    return H.reference_record(rho, u, v, E, p, c, scale_exp=scale, **kw)


def test_a_nan_cell_counts_in_n_bad_only():
    rho, u, v, E = hand_state()
    clean = record_of(rho, u, v, E)
    rho[2, 3] = math.nan
    rec = record_of(rho, u, v, E)
    assert int(rec[H.W_N]) == 23 and int(rec[H.W_BAD]) == 1 and int(clean[H.W_N]) == 24 and int(clean[H.W_BAD]) == 0
    rho[2, 3] = 1.0
    skip = H.merge_raw(record_of(rho[:2], u[:2], v[:2], E[:2], global_nx=6),
                       H.merge_raw(record_of(rho[2:3, :3], u[2:3, :3], v[2:3, :3], E[2:3, :3], origin=(0, 2), global_nx=6),
                                   H.merge_raw(record_of(rho[2:3, 4:], u[2:3, 4:], v[2:3, 4:], E[2:3, 4:], origin=(4, 2), global_nx=6),
                                               record_of(rho[3:], u[3:], v[3:], E[3:], origin=(0, 3), global_nx=6))))
    got = rec.copy()
    got[H.W_BAD] = 0
    assert np.array_equal(got, skip)                                    # the record of the 23 other cells, word for word
    for bad in (("u", math.inf), ("E", -math.inf), ("v", math.nan)):
        f = dict(zip(("rho", "u", "v", "E"), hand_state()))
        f[bad[0]][1, 1] = bad[1]
        r = record_of(f["rho"], f["u"], f["v"], f["E"])
        assert (int(r[H.W_N]), int(r[H.W_BAD])) == (23, 1), bad
    # |Q| >= 2^95: rho = 2 at a quantum of 2^-94
    r = record_of(*hand_state(), scale=(-94,) + (-60,) * 5)
    assert int(r[H.W_N]) == 24
    rho, u, v, E = hand_state()
    rho[0, 0] = 2.0
    r = record_of(rho, u, v, E, scale=(-94,) + (-60,) * 5)
    assert (int(r[H.W_N]), int(r[H.W_BAD])) == (23, 1)


def test_two_equal_maxima_resolve_to_the_lower_index_and_minus_zero_orders_below_plus_zero():
    rho, u, v, E = hand_state()
    rho[3, 1] = rho[1, 4] = 3.0                 # g = 19 and g = 10
    rho[2, 2] = rho[0, 5] = 0.25                # g = 14 and g = 5
    R = H.HistoryRecord(record_of(rho, u, v, E), (-60,) * 6, 1.0, 6)
    assert R.rho_max == 3.0 and R.at["rho_max"] == (4, 1) and R.rho_min == 0.25 and R.at["rho_min"] == (5, 0)
    # whichever half comes first
    a = record_of(rho[:2], u[:2], v[:2], E[:2], global_nx=6)
    b = record_of(rho[2:], u[2:], v[2:], E[2:], origin=(0, 2), global_nx=6)
    assert np.array_equal(H.merge_raw(a, b), R.raw) and np.array_equal(H.merge_raw(b, a), R.raw)
    # a fluid at rest: q2 == +0.0 everywhere, the first cell holds the maximum; Mach 0
    assert R.speed_max == 0.0 and R.at["speed_max"] == (0, 0) and R.mach_max == 0.0
    assert prof.order_key(-0.0) < prof.order_key(0.0)
    # E = +0.0 in one cell and -0.0 in another (rho = 1, u = v = 0): e = E, and -0.0 is the minimum although it comes later
    rho, u, v, E = hand_state()
    E[:] = 1.0
    E[1, 1], E[2, 2] = 0.0, -0.0
    p, c = perfect_gas(rho, u, v, E)
    c[1, 1] = c[2, 2] = 1.0                     # (the sound speed of a cold cell is 0 / NaN-free here: keep both cells good)
    R = H.HistoryRecord(H.reference_record(rho, u, v, E, p, c, scale_exp=(-60,) * 6), (-60,) * 6, 1.0, 6)
    assert R.n == 24 and R.at["e_min"] == (2, 2) and math.copysign(1.0, R.e_min) == -1.0 and R.e_min == 0.0


def test_internal_energy_is_the_exact_difference_of_two_integer_sums():
    rng = np.random.default_rng(11)
    shape = (9, 14)
    rho, u, v, E = rng.uniform(0.1, 2, shape), rng.standard_normal(shape), rng.standard_normal(shape), rng.uniform(20, 24, shape)
    scale = (-70, -68, -68, -66, -66, -69)
    raw = record_of(rho, u, v, E, scale=scale)
    R = H.HistoryRecord(raw, scale, 0.125, 14)
    assert R.n == rho.size
    # the sums are the exact sums of the rounded addends
    t, _ = H.cell_terms(rho, u, v, E, *perfect_gas(rho, u, v, E))
    for k in range(6):
        assert R.sums[k] == sum(prof.quantise(x, scale[k]) for x in t[k].ravel().tolist()), k
    from fractions import Fraction
    assert R.internal == float(Fraction(R.sums[3] - R.sums[4]) * Fraction(2) ** -66 * Fraction(0.125))
    assert R.energy == float(Fraction(R.sums[3]) * Fraction(2) ** -66 * Fraction(0.125))
    assert R.kinetic >= 0 and abs(R.internal - (R.energy - R.kinetic)) <= 2 ** -52 * R.energy
    assert math.isnan(H.HistoryRecord(raw, (-70, -68, -68, -66, -65, -69), 0.125, 14).internal)     # two quanta: no exact difference
    assert R.speed_max == math.sqrt((u * u + v * v).max()) and R.at["speed_max"] == tuple(int(i) for i in np.unravel_index(np.argmax(u * u + v * v), shape))[::-1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_any_split_by_rows_or_by_columns_merges_to_the_whole(dtype):
    rng = np.random.default_rng(3)
    shape = (11, 17)
    rho, u, v, E = (rng.uniform(0.1, 2, shape).astype(dtype), rng.standard_normal(shape).astype(dtype), rng.standard_normal(shape).astype(dtype),
                    rng.uniform(20, 24, shape).astype(dtype))
    u[4, 4] = math.nan
    scale = H.default_scale(record_of(rho, u, v, E))
    whole = record_of(rho, u, v, E, scale=scale, origin=(3, 2), global_nx=40)
    assert int(whole[H.W_N]) == rho.size - 1 and not whole[36:].any()
    for cut in (1, 5, 10):
        a = record_of(rho[:cut], u[:cut], v[:cut], E[:cut], scale=scale, origin=(3, 2), global_nx=40)
        b = record_of(rho[cut:], u[cut:], v[cut:], E[cut:], scale=scale, origin=(3, 2 + cut), global_nx=40)
        assert np.array_equal(H.merge_raw(a, b), whole) and np.array_equal(H.merge_raw(b, a), whole), ("rows", cut)
    for cut in (1, 8, 16):
        a = record_of(rho[:, :cut], u[:, :cut], v[:, :cut], E[:, :cut], scale=scale, origin=(3, 2), global_nx=40)
        b = record_of(rho[:, cut:], u[:, cut:], v[:, cut:], E[:, cut:], scale=scale, origin=(3 + cut, 2), global_nx=40)
        assert np.array_equal(H.merge_raw(a, b), whole) and np.array_equal(H.merge_raw(b, a), whole), ("columns", cut)
    assert np.array_equal(H.merge_raw(H.neutral(), whole), whole)


def initial_state(oracle, test, N=(100, 100), g=4):
    """rho, u, v, E of the test case's initial state and the EOS's p, c of it, from the CPU oracle (real cells, fp64)."""
    nx, ny = N
    _run, f = oracle.solve(test=test, N=N, maxcycle=0, nghost=g)
    args = [oracle.ptr(f[k]) for k in (("rho", "u", "v", "E") if test == "Bizarrium" else ("rho", "E", "u", "v")) + ("p", "c", "g")]
    r = oracle.domain_range(nx, ny, g)
    if test == "Bizarrium":
        oracle.lib().armon_oracle_bizarrium_EOS(r, *args)
    else:
        oracle.lib().armon_oracle_perfect_gas_EOS(r, 7 / 5, *args)
    return [oracle.real_view(f[k], nx, ny, g).copy() for k in ("rho", "u", "v", "E", "p", "c")]


@pytest.mark.parametrize("test", ["Sod", "Sedov", "Bizarrium"])
def test_the_default_scale_leaves_no_bad_cell_and_sixteen_bits_of_headroom(oracle, test):
    rho, u, v, E, p, c = initial_state(oracle, test)
    first = H.reference_record(rho, u, v, E, p, c, scale_exp=H.FIRST_SCALE)         # any scale that refuses no cell: the extrema do not depend on it
    scale = H.default_scale(first)
    assert scale[3] == scale[4] and scale[1] == scale[2]
    again = H.reference_record(rho, u, v, E, p, c, scale_exp=(-20,) * 6)
    assert np.array_equal(first[H.W_EXT:], again[H.W_EXT:]) and H.default_scale(again) == scale
    rec = H.reference_record(rho, u, v, E, p, c, scale_exp=scale)
    assert int(rec[H.W_BAD]) == 0 and int(rec[H.W_N]) == rho.size
    # rho and p may grow 2^16-fold, and not 2^18-fold: 2^(e - 1) <= B < 2^e puts the largest |Q| in [2^77, 2^78) at the start
    big = H.reference_record(rho * 2.0 ** 16, u, v, E, p * 2.0 ** 16, c, scale_exp=(scale[0],) + (0,) * 4 + (scale[5],))
    assert int(big[H.W_BAD]) == 0
    for grown in ((rho * 2.0 ** 18, p), (rho, p * 2.0 ** 18)):
        big = H.reference_record(grown[0], u, v, E, grown[1], c, scale_exp=(scale[0],) + (0,) * 4 + (scale[5],))
        assert int(big[H.W_BAD]) > 0
    # the quantum stays far below the last bit of the largest term
    assert scale[0] <= math.frexp(float(rho.max()))[1] - 53 - 20
    # a velocity field that turns ALL of the largest cell's energy into motion still fits the momentum and kinetic scales
    fast = np.sqrt(2 * np.abs(E - 0.5 * (u * u + v * v)).max())
    moving = H.reference_record(rho, np.full_like(u, fast), v, E, p, c, scale_exp=scale)
    assert int(moving[H.W_BAD]) == 0


def small_history(gauges=((0.25, 0.5), (1.0, 1.0)), rows=5, seed=2):
    rng = np.random.default_rng(seed)
    scale = (-70, -68, -68, -66, -66, -69)
    h = H.History(scale, 1.0 / 64, 8, gauges, [(2, 4), (7, 7)][:len(gauges)])
    time = 0.0
    for i in range(rows):
        shape = (8, 8)
        rho, u, v, E = rng.uniform(0.1, 2, shape), rng.standard_normal(shape), rng.standard_normal(shape), rng.uniform(20, 24, shape)
        dt = 0.0 if i == 0 else float(rng.uniform(1e-3, 2e-3))
        time += dt
        h.append(3 * i, time, dt, record_of(rho, u, v, E, scale=scale), rng.standard_normal((len(gauges), 5)))
    return h


def same_table(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype == np.float64 and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
        else:
            assert a[k] == b[k], k


def test_the_file_round_trip_is_exact(tmp_path):
    h = small_history()
    path = str(tmp_path / "history.txt")
    aio.write_history_file(path, h, (8, 8))
    same_table(aio.read_history_file(path), h.table())
    text = open(path).read().splitlines()
    head = [line for line in text if line.startswith("#")]
    assert head[0] == "# history version=1" and "# scale_exp=-70,-68,-68,-66,-66,-69" in head and any(line.startswith("# ds=") for line in head)
    assert sum(line.startswith("# gauge") for line in head) == 2 and head[-1].startswith("# columns=cycle,time,dt,n,n_bad,mass,momentum_x")
    rows = [line for line in text if not line.startswith("#")]
    assert len(rows) == 5 and all(len(r.split()) == len(H.COLUMNS) + 10 for r in rows)
    assert all(re.fullmatch(r"[ +-]?\d\.\d{17}e[+-]\d+", v) for v in rows[1].split())          # %#24.17e
    # written in two batches: the same bytes
    two = str(tmp_path / "two.txt")
    first = H.History(*h._meta())
    first.append(h.cycle[:2], h.time[:2], h.dt[:2], h.raw[:2], h.gauge_values[:2])
    aio.write_history_file(two, first, (8, 8))
    aio.append_history_rows(two, h, 2)
    assert open(two).read() == open(path).read()
    # the columns are the decoded records
    t = h.table()
    assert t["mass"][3] == h.records[3].mass == h.mass[3] and t["g1_E"][2] == h.gauge_values[2, 1, 3] == h.gauges_of(1)["E"][2]
    assert t["rho_max_gx"][1] == h.records[1].at["rho_max"][0] and list(t["cycle"]) == [0, 3, 6, 9, 12]
    # equality is on the words; concat joins what append would have built
    rest = H.History(*h._meta())
    rest.append(h.cycle[2:], h.time[2:], h.dt[2:], h.raw[2:], h.gauge_values[2:])
    assert first.concat(rest) == h and first != h and rest.concat(first) != h
    other = small_history(seed=3)
    assert other != h and np.array_equal(h.raw, small_history().raw)
    with pytest.raises(SolverException):
        h.concat(small_history(gauges=()))


def test_a_restart_keeps_the_rows_up_to_its_cycle_and_refuses_another_header(tmp_path):
    h = small_history()
    path = str(tmp_path / "history.txt")
    aio.write_history_file(path, h, (8, 8))
    head = aio.read_history_header(path)
    aio.check_history_header(path, head, h, (8, 8))                     # its own header: accepted
    aio.truncate_history_file(path, 6)
    t = aio.read_history_file(path)
    assert list(t["cycle"]) == [0, 3, 6] and t["mass"][2] == h.mass[2]
    aio.append_history_rows(path, h, 3)                                 # the restarted run appends what follows
    whole = str(tmp_path / "whole.txt")
    aio.write_history_file(whole, h, (8, 8))
    assert open(path).read() == open(whole).read()
    aio.truncate_history_file(path, 7)                                  # a cycle between two rows
    assert list(aio.read_history_file(path)["cycle"]) == [0, 3, 6]
    # every field of the header is compared, and named
    meta = h._meta()
    for field, other, grid in (("scale_exp", H.History((-70, -68, -68, -66, -66, -68), *meta[1:]), (8, 8)),
                               ("ds", H.History(meta[0], 1.0 / 32, *meta[2:]), (8, 8)),
                               ("N", h, (8, 16)),
                               ("gauge1", H.History(*meta[:3], ((0.25, 0.5), (0.75, 1.0)), meta[4]), (8, 8)),
                               ("gauge1", H.History(*meta[:3], meta[3][:1], meta[4][:1]), (8, 8)),
                               ("gauge0", H.History(*meta[:3], meta[3], ((3, 4), (7, 7))), (8, 8))):
        with pytest.raises(SolverException) as e:
            aio.check_history_header(path, head, other, grid)
        assert e.value.category == "config" and f": {field} is " in e.value.msg, (field, e.value.msg)
    junk = str(tmp_path / "junk.txt")
    open(junk, "w").write("# profile kind=x\n1 2 3\n")
    with pytest.raises(SolverException) as e:
        aio.read_history_header(junk)
    assert e.value.category == "config" and "version" in e.value.msg


def test_every_option_is_refused_as_the_docstring_says():
    base = dict(test="Sod", N=(8, 8))
    p = ArmonParameters(**base)
    assert (p.history_step, p.history_file, p.history_gauges, p.history_capacity, p.history_scale_exp) == (0, "history", (), 256, None)
    p = ArmonParameters(history_step=3, history_file="h", history_gauges=[(0.1, 0.2), (1, 1)], history_capacity=8,
                        history_scale_exp=[-70, -68, -68, -66, -66, -69], **base)
    assert (p.history_step, p.history_file, p.history_gauges, p.history_capacity, p.history_scale_exp) == \
        (3, "h", ((0.1, 0.2), (1.0, 1.0)), 8, (-70, -68, -68, -66, -66, -69))
    for bad in (dict(history_step=-1), dict(history_step=1.5), dict(history_step=True), dict(history_step="2"), dict(history_file=""),
                dict(history_file="a/b"), dict(history_capacity=0), dict(history_capacity=65537), dict(history_capacity=2.0),
                dict(history_capacity=True), dict(history_gauges=[(0.5,)]), dict(history_gauges=[(0.5, math.nan)]), dict(history_gauges=3),
                dict(history_gauges=[(1.5, 0.5)]), dict(history_gauges=[(0.5, -0.01)]), dict(history_gauges=[(0.5, 0.5)] * 65),
                dict(history_scale_exp=(0,) * 5), dict(history_scale_exp=(0,) * 5 + (5000,)), dict(history_scale_exp="abc"),
                dict(history_step=2, use_MPI=True, P=(1, 1))):
        with pytest.raises(SolverException) as e:
            ArmonParameters(**base, **bad)
        assert e.value.category == "config", bad
    assert len(ArmonParameters(history_gauges=[(0.5, 0.5)] * 64, **base).history_gauges) == 64
    # the cell of a point: the domain is closed, a point on a cell edge belongs to the cell above it
    p = ArmonParameters(test="Sedov", N=(8, 4))
    assert H.gauge_cells(p, [(-1.0, -1.0), (1.0, 1.0), (0.0, 0.0), (-0.75, 0.49)]) == [(0, 0), (7, 3), (4, 2), (1, 2)]


def test_graph_cycles_are_not_used_with_a_history():
    import types

    def usable(**kw):
        p = ArmonParameters(test="Sod", N=(8, 8), graph_cycles=True, silent=5, **kw)
        p._device = types.SimpleNamespace(owns_ctx=True)
        return graph_cycles_usable(p)
    assert usable() is True and usable(history_step=1) is False and usable(history_gauges=[(0.5, 0.5)]) is True
    assert SolverStats(0.0, 0.0, 0, 0.0, 0, 0.0).history is None
