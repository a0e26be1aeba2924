"""Mixing measures, the host side (no GPU): the ABI, the argument checks, the restated rules on hand-made fields, the whole-record
measures against exact rationals, the merge, the histogram's edges, the file round trips and the run options."""
import ctypes as C
import math
import os
import re
import types
from fractions import Fraction

import numpy as np
import pytest

import armon_amd
from armon_amd import io as aio
from armon_amd import mixing as mix
from armon_amd import profile as prof
from armon_amd._lib import SIGNATURES, MixingBin, MixingSpec, PdfSpec, SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import SolverStats, graph_cycles_usable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mixing_reset", "mixing", "mixing_f32", "mixing_bounds", "mixing_bounds_f32", "scalar_pdf_reset", "scalar_pdf",
                "scalar_pdf_f32")
SCALE = (-60,) * 5


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "armon_hip.h")).read()
    L = armon_amd.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"ARMON_API int armon_hip_%s\(" % name, header), name
        assert "armon_hip_" + name in SIGNATURES
        assert getattr(L, "armon_hip_" + name).argtypes == SIGNATURES["armon_hip_" + name][1]
    assert "WORD FOR WORD" in header[header.index("mixing measures"):]
    assert "t0 = rho, t1 = phi, t2 = phi * phi, t3 = rho * phi, t4 = t3 * phi" in header
    assert "fb = floor((phi - lo) * inv_w)" in header and "#define ARMON_PDF_MAX_BINS 1024" in header
    assert C.sizeof(MixingBin) == 160 and C.sizeof(MixingSpec) == 104 and C.sizeof(PdfSpec) == 24
    assert MixingBin.phi_min.offset == 136 and MixingSpec.scale_exp.offset == 24 and PdfSpec.nbins.offset == 16
    assert mix.WORDS * 8 == C.sizeof(MixingBin) and mix.MAX_SCALARS == 4
    for name in ("MixingProfile", "ScalarPDF", "mixing_state", "pdf_state"):
        assert getattr(armon_amd, name) is getattr(mix, name)


def mixing_spec(**kw):
    s = MixingSpec()
    s.axis, s.nbins, s.width = 1, 8, 1
    for k, v in kw.items():
        if k == "scale_exp":
            s.scale_exp[v[0]][v[1]] = v[2]
        else:
            setattr(s, k, v)
    return s


def pdf_spec(**kw):
    s = PdfSpec()
    s.lo, s.inv_w, s.nbins, s.rho_scale_exp = 0.0, 64.0, 64, -60
    for k, v in kw.items():
        setattr(s, k, v)
    return s


WINDOW_REFUSALS = (dict(nx=0), dict(ny=0), dict(nghost=-1), dict(row_length=15), dict(col0=-1), dict(row0=-1), dict(wnx=0), dict(wny=0),
                   dict(col0=1), dict(row0=1), dict(wnx=9), dict(wny=9), dict(nx=1 << 31, row_length=(1 << 31) + 8))


def test_a_null_context_and_every_bad_argument_are_refused():
    L = armon_amd.lib()
    fake_ctx = C.create_string_buffer(4096)          # never dereferenced: every check below comes before the first use of the context
    ctx = C.cast(fake_ctx, C.c_void_p)
    data = C.cast(C.create_string_buffer(64), C.c_void_p)
    geometry = dict(row_length=16, nghost=4, nx=8, ny=8, col0=0, row0=0, wnx=8, wny=8, gcol=0, grow=0)
    planes = (C.c_void_p * 4)(data, data, data, data)

    def call(fn, ctx=ctx, spec=None, out=data, rho=data, ns=2, phi=planes, **kw):
        g = {**geometry, **kw}
        spec = mixing_spec() if spec is None else spec
        return fn(ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], rho, ns, phi, g["col0"], g["row0"], g["wnx"], g["wny"],
                  g["gcol"], g["grow"], C.byref(spec) if spec is not False else None, out)

    for name in ("mixing", "mixing_f32", "mixing_bounds", "mixing_bounds_f32"):
        fn = getattr(L, "armon_hip_" + name)
        assert call(fn, ctx=None) == 1, name
        assert b"ctx" in L.armon_hip_last_error()
        for bad in WINDOW_REFUSALS + (dict(gcol=-1), dict(grow=-1)):
            assert call(fn, **bad) == 1, (name, bad)
        assert call(fn, rho=None) == 1 and call(fn, out=None) == 1 and call(fn, spec=False) == 1 and call(fn, phi=None) == 1
        for ns in (0, -1, 5):
            assert call(fn, ns=ns) == 1, (name, ns)
        assert call(fn, ns=3, phi=(C.c_void_p * 4)(data, data, None, data)) == 1 and b"phi[2]" in L.armon_hip_last_error()
        for bad in (dict(nbins=0), dict(nbins=-3), dict(width=0), dict(axis=2), dict(axis=-1), dict(scale_exp=(1, 3, 5000)),
                    dict(scale_exp=(0, 0, -4097))):
            assert call(fn, spec=mixing_spec(**bad)) == 1, (name, bad)
    assert L.armon_hip_mixing_reset(None, 1, 4, data) == 1
    for ns, nbins, out in ((0, 4, data), (5, 4, data), (1, 0, data), (1, 4, None)):
        assert L.armon_hip_mixing_reset(ctx, ns, nbins, out) == 1

    def pdf(fn, ctx=ctx, spec=None, out=data, rho=data, phi=data, **kw):
        g = {**geometry, **kw}
        spec = pdf_spec() if spec is None else spec
        return fn(ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], rho, phi, g["col0"], g["row0"], g["wnx"], g["wny"],
                  C.byref(spec) if spec is not False else None, out)

    inf, nan = math.inf, math.nan
    for name in ("scalar_pdf", "scalar_pdf_f32"):
        fn = getattr(L, "armon_hip_" + name)
        assert pdf(fn, ctx=None) == 1, name
        for bad in WINDOW_REFUSALS:
            assert pdf(fn, **bad) == 1, (name, bad)
        assert pdf(fn, rho=None) == 1 and pdf(fn, phi=None) == 1 and pdf(fn, out=None) == 1 and pdf(fn, spec=False) == 1
        for bad in (dict(nbins=0), dict(nbins=-1), dict(nbins=1025), dict(lo=nan), dict(lo=inf), dict(inv_w=0.0), dict(inv_w=-1.0),
                    dict(inv_w=inf), dict(inv_w=nan), dict(rho_scale_exp=4097), dict(rho_scale_exp=-5000)):
            assert pdf(fn, spec=pdf_spec(**bad)) == 1, (name, bad)
    assert L.armon_hip_scalar_pdf_reset(None, 4, data) == 1
    for nbins, out in ((0, data), (1025, data), (4, None)):
        assert L.armon_hip_scalar_pdf_reset(ctx, nbins, out) == 1


# ---- the restated rule on hand-made fields ---------------------------------------------------------------------------------
def profile_of(phi, rho=None, axis="y", width=1, nbins=None, scale=SCALE, dx=0.5, dy=0.25, origin=(0, 0), N=None, name="f"):
    phi = np.asarray(phi, dtype=np.float64)
    rho = np.ones_like(phi) if rho is None else np.asarray(rho, dtype=np.float64)
    ax = mix.AXES[axis]
    N = phi.shape[1 - ax] if N is None else N
    nbins = -(-N // width) if nbins is None else nbins
    raw = mix.reference_record(axis, nbins, width, scale, rho, phi, origin=origin)
    return mix.MixingProfile(raw, (ax, nbins, width, dx, dy, N), scale, name, origin=(10.0, -2.0))


def test_a_uniform_half_is_fully_mixed_and_alternating_rows_are_not():
    P = profile_of(np.full((6, 8), 0.5))
    assert P.mixedness == 1.0 and P.integral_width == 6 * 0.25 * 0.25 and P.n.tolist() == [8] * 6
    assert P.variance.tolist() == [0.0] * 6 and P.phi.tolist() == [0.5] * 6 and P.minimum == P.maximum == 0.5
    stripes = np.zeros((6, 8))
    stripes[:, ::2] = 1.0                                       # every row alternates 0 / 1: the mean is 0.5, nothing is mixed
    P = profile_of(stripes)
    assert P.phi.tolist() == [0.5] * 6 and P.mixedness == 0.0 and P.integral_width == 6 * 0.25 * 0.25
    assert P.variance.tolist() == [0.25] * 6 and (P.minimum, P.maximum) == (0.0, 1.0)
    # a pure field: W = 0, and Θ is undefined
    P = profile_of(np.ones((3, 4)))
    assert P.integral_width == 0.0 and math.isnan(P.mixedness) and P.extent() is None


def test_the_integral_width_of_a_ramp_is_the_rational_sum_rounded_once():
    dy = 0.1                                                    # (no binary fraction: the products below are not exact in fp64)
    ramp = np.repeat(((np.arange(8) + 0.5) / 8)[:, None], 5, axis=1)
    P = profile_of(ramp, dy=dy)
    want = sum(Fraction(2 * b + 1, 16) * (1 - Fraction(2 * b + 1, 16)) * Fraction(dy) for b in range(8))
    assert P.phi.tolist() == [(b + 0.5) / 8 for b in range(8)] and P.integral_width == float(want)
    top = sum((Fraction(2 * b + 1, 16) - Fraction(2 * b + 1, 16) ** 2) * Fraction(dy) for b in range(8))
    assert P.mixedness == float(top / want) == 1.0              # no variance inside a row
    # bins of 3 rows: 3, 3 and 2 rows of the ramp, lengths 3 dy, 3 dy, 2 dy
    P = profile_of(ramp, dy=dy, width=3)
    means = [Fraction(3, 16), Fraction(9, 16), Fraction(14, 16)]
    assert P.n.tolist() == [15, 15, 10] and [Fraction(x) for x in P.phi.tolist()] == means
    want = sum(m * (1 - m) * rows * Fraction(dy) for m, rows in zip(means, (3, 3, 2)))
    assert P.integral_width == float(want) and P.lengths() == [3 * Fraction(dy), 3 * Fraction(dy), 2 * Fraction(dy)]


def test_the_content_is_the_exact_sum():
    rng = np.random.default_rng(11)
    rho, phi = rng.uniform(0.1, 10, (7, 9)), rng.uniform(-0.5, 1.5, (7, 9))
    dx, dy = 0.3, 0.7
    P = profile_of(phi, rho, dx=dx, dy=dy, axis="x")
    total = sum(prof.quantise(float(r) * float(f), SCALE[3]) for r, f in zip(rho.ravel(), phi.ravel()))
    assert sum(P.sums[3]) == total
    assert P.content == float(Fraction(total) * Fraction(2) ** SCALE[3] * Fraction(dx) * Fraction(dy))
    assert P.minimum == phi.min() and P.maximum == phi.max() and P.coord.tolist() == [10.0 + (b + 0.5) * dx for b in range(9)]
    # every decoded column against the rationals of its bin
    for b in range(9):
        S = [sum(prof.quantise(float(t), SCALE[j]) for t in col) * Fraction(2) ** SCALE[j]
             for j, col in enumerate(a[:, b] for a in mix.cell_terms(rho, phi))]
        assert P.phi[b] == float(S[1] / 7) and P.phi_favre[b] == float(S[3] / S[0]) and P.rho[b] == float(S[0] / 7)
        assert P.variance[b] == float(S[2] / 7 - (S[1] / 7) ** 2) and P.favre_variance[b] == float(S[4] / S[0] - (S[3] / S[0]) ** 2)
        assert P.phi_min[b] == phi[:, b].min() and P.phi_max[b] == phi[:, b].max()


def test_the_extent_of_a_step_and_an_empty_bin():
    col = np.array([0.0, 0.0, 0.005, 0.01, 0.3, 0.99, 0.995, 1.0, 1.0, 0.5])
    P = profile_of(np.repeat(col[:, None], 4, axis=1), dy=0.25)
    assert P.extent() == (-2.0 + 3 * 0.25, -2.0 + 10 * 0.25)     # 0.01 and 0.99 are inside (the fp64 values, compared exactly), the last row too
    assert P.extent(0.2, 0.6) == (-2.0 + 4 * 0.25, -2.0 + 10 * 0.25) and P.extent(0.31, 0.49) is None
    assert P.extent(0.996, 1.0) == (-2.0 + 7 * 0.25, -2.0 + 9 * 0.25)
    # bins of 4 rows over 10: the last bin holds 2 rows and ends at the domain's edge
    P4 = profile_of(np.repeat(col[:, None], 4, axis=1), dy=0.25, width=4)
    assert P4.extent(0.0, 1.0) == (-2.0, -2.0 + 10 * 0.25) and P4.n.tolist() == [16, 16, 8]
    # a bin no cell reaches (the record has more bins than the field has rows): NaN everywhere, skipped by the measures
    P = profile_of(np.full((3, 2), 0.5), nbins=5, N=5)
    assert P.n.tolist() == [2, 2, 2, 0, 0]
    for name in ("phi", "phi_favre", "variance", "favre_variance", "rho", "phi_min", "phi_max"):
        column = getattr(P, name)
        assert not np.isnan(column[:3]).any() and np.isnan(column[3:]).all(), name
    assert P.mixedness == 1.0 and P.integral_width == 3 * 0.25 * 0.25 and "nan" in P.report()
    # cells past the last bin are counted nowhere
    P = profile_of(np.full((6, 2), 0.5), nbins=2, width=2)
    assert P.n.tolist() == [4, 4] and P.n_bad.tolist() == [0, 0]


def test_bad_cells_count_in_their_plane_only():
    rho = np.array([[1.0, 2.0], [math.nan, 1.0], [1.0, 1.0]])
    phi = np.array([[0.5, math.inf], [0.5, 1e200], [0.25, -0.0]])
    P = profile_of(phi, rho)
    assert P.n.tolist() == [1, 0, 2] and P.n_bad.tolist() == [1, 2, 0]     # inf; NaN rho and phi² = inf; none
    assert np.array([P.phi_min[2]]).tobytes() == np.array([-0.0]).tobytes() and P.phi_max[2] == 0.25
    # |Q| >= 2^95 is bad too: 1.0 at the quantum 2^-95
    P = profile_of(np.full((1, 1), 0.5), scale=(-95, -60, -60, -60, -60))
    assert P.n.tolist() == [0] and P.n_bad.tolist() == [1] and not P.raw[0, 2:17].any()
    # the bounds pass sees every finite term
    b = mix.reference_bounds(rho, phi)
    assert np.array(b, dtype=np.uint64).view(np.float64).tolist() == [2.0, 1e200, 0.25, 1e200, 0.25]
    assert mix.reference_bounds(np.float32([[0.1]]), np.float32([[3.0]]))[3] == int(np.array([float(np.float32(0.1)) * 3.0]).view(np.uint64)[0])


def test_a_split_field_merges_to_the_whole_word_for_word():
    rng = np.random.default_rng(3)
    rho, phi = rng.uniform(0.1, 10, (13, 17)), rng.uniform(-0.5, 1.5, (13, 17))
    phi[4, 5], rho[9, 2] = math.nan, math.inf
    for axis, width in (("x", 1), ("y", 1), ("x", 3), ("y", 5), ("y", 50)):
        N = 17 if axis == "x" else 13
        whole = profile_of(phi, rho, axis=axis, width=width, origin=(100, 7), N=N + 200)
        merged = None
        for r0, r1 in ((0, 6), (6, 13)):
            for c0, c1 in ((0, 4), (4, 11), (11, 17)):
                part = profile_of(phi[r0:r1, c0:c1], rho[r0:r1, c0:c1], axis=axis, width=width, origin=(100 + c0, 7 + r0), N=N + 200)
                merged = part if merged is None else merged.merge(part)
        assert merged == whole and np.array_equal(merged.raw, whole.raw), (axis, width)
        assert int(whole.n_bad.sum()) == 2 and int(whole.n.sum()) == 13 * 17 - 2
    a = profile_of(phi, rho)
    for other in (profile_of(phi, rho, scale=(-60, -60, -61, -60, -60)), profile_of(phi, rho, width=2), profile_of(phi, rho, axis="x"),
                  profile_of(phi, rho, name="g"), profile_of(phi, rho, dy=0.5)):
        with pytest.raises(SolverException) as e:
            a.merge(other)
        assert e.value.category == "config"
        assert a != other


# ---- the histogram ---------------------------------------------------------------------------------------------------------
def pdf_of(phi, rho=None, lo=0.0, hi=1.0, nbins=64, s=-60):
    phi = np.asarray(phi, dtype=np.float64)
    rho = np.ones_like(phi) if rho is None else np.asarray(rho, dtype=np.float64)
    return mix.ScalarPDF(mix.reference_pdf(rho, phi, lo, mix.inv_width(lo, hi, nbins), nbins, s), lo, hi, nbins, s, "f")


def edge_values(nbins=64):
    """φ exactly at lo, at every edge, at hi, a step on both sides of each, and -0.0."""
    edges = np.arange(nbins + 1) / nbins
    return np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-0.0]])


def test_the_histogram_at_its_exact_edges():
    v = edge_values()
    P = pdf_of(v)
    # an edge belongs to the bin above it; the value just below to the bin below; hi itself is "above"; -0.0 is not < 0.0
    want = np.zeros(64, dtype=np.int64)
    want[:] += 1                                                # edges 0 .. 63
    want[:] += 1                                                # nextafter up of edges 0 .. 63
    want[:] += 1                                                # nextafter down of edges 1 .. 64
    want[0] += 1                                                # -0.0
    assert P.counts.tolist() == want.tolist()
    assert P.below[0] == 1 and P.above[0] == 2 and P.bad == 0   # below: nextafter(0, -inf); above: 1.0 and its successor
    assert int(P.counts.sum()) + P.below[0] + P.above[0] + P.bad == v.size
    assert P.edges.tolist() == (np.arange(65) / 64).tolist() and P.mass.tolist() == want.astype(float).tolist()
    assert P.density().sum() * (1 / 64) == 1.0 and P.mass_sums[3] == 3 << 60


def test_nan_and_inf_go_to_bad_and_the_mass_is_exact():
    rho = np.array([1.0, 0.1, math.nan, 2.0, 3.0, math.inf, 0.3, 1.0])
    phi = np.array([0.5, 0.5, 0.5, math.nan, math.inf, 0.2, -3.0, 7.0])
    P = pdf_of(phi, rho, nbins=4)
    assert P.bad == 4 and P.counts.tolist() == [0, 0, 2, 0] and P.below[0] == 1 and P.above[0] == 1
    assert P.mass_sums[2] == (1 << 60) + prof.quantise(0.1, -60) and P.below[1] == float(Fraction(prof.quantise(0.3, -60), 1 << 60))
    assert P.above[1] == 1.0
    assert pdf_of([0.5], [1.0], s=-95).bad == 1                 # |Q(rho)| reaches 2^95


def test_inexact_edges_follow_the_rule_not_the_nominal_edges():
    for nbins, lo, hi in ((10, 0.0, 1.0), (7, -0.3, 1.1), (1, 0.0, 1.0), (2, 0.0, 1.0), (1024, 0.0, 1.0)):
        inv_w = mix.inv_width(lo, hi, nbins)
        nominal = lo + np.arange(nbins + 1) * (hi - lo) / nbins
        v = np.concatenate([nominal, np.nextafter(nominal, -np.inf), np.nextafter(nominal, np.inf)])
        P = pdf_of(v, lo=lo, hi=hi, nbins=nbins)
        counts, below, above = [0] * nbins, 0, 0
        for x in v.tolist():                                    # the rule, one cell at a time in Python floats (IEEE fp64)
            if x < lo:
                below += 1
                continue
            fb = math.floor((x - lo) * inv_w)
            if not fb < nbins:
                above += 1
            else:
                counts[fb] += 1
        assert (P.counts.tolist(), P.below[0], P.above[0], P.bad) == (counts, below, above, 0), nbins
        assert sum(counts) + below + above == v.size
    P = pdf_of([0.0, 0.3, 0.999, 1.0, -1e-300], nbins=1)
    assert P.counts.tolist() == [3] and P.above[0] == 1 and P.below[0] == 1
    a, b = pdf_of([0.1, 0.7], nbins=4), pdf_of([0.1, 2.0, math.nan], nbins=4)
    m = a.merge(b)
    assert m.counts.tolist() == [2, 0, 1, 0] and m.above[0] == 1 and m.bad == 1 and m == pdf_of([0.1, 0.7, 0.1, 2.0, math.nan], nbins=4)
    for other in (pdf_of([0.1], nbins=5), pdf_of([0.1], nbins=4, s=-61), pdf_of([0.1], nbins=4, hi=2.0)):
        with pytest.raises(SolverException):
            a.merge(other)


# ---- files -----------------------------------------------------------------------------------------------------------------
def same_table(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and (a[k].tobytes() == b[k].tobytes() or np.array_equal(a[k], b[k], equal_nan=True)), k
        elif isinstance(a[k], tuple):
            assert len(a[k]) == len(b[k]) and all(x == y or (x != x and y != y) for x, y in zip(a[k], b[k])), k
        else:
            assert a[k] == b[k], k


def drawn_sample(seed, cycle, with_pdf=True):
    rng = np.random.default_rng(seed)
    rho, phi = rng.uniform(0.1, 10, (6, 5)), rng.uniform(-0.5, 1.5, (6, 5))
    profiles = {"heavy": profile_of(phi, rho, name="heavy", nbins=7, N=7), "dye": profile_of(phi * phi, rho, name="dye", width=4)}
    pdfs = {"heavy": pdf_of(phi, rho, nbins=16), "dye": pdf_of(phi * phi, rho, nbins=3, lo=-0.25, hi=2.0)} if with_pdf else None
    for k, r in list(profiles.items()) + list((pdfs or {}).items()):
        r.name, r.cycle, r.time = k, cycle, 0.1234567890123 * cycle
    return (cycle, 0.1234567890123 * cycle, profiles, pdfs)


def test_both_files_round_trip(tmp_path):
    for with_pdf in (True, False):
        cycle, time, profiles, pdfs = drawn_sample(5, 12, with_pdf)
        path = str(tmp_path / f"m_{with_pdf}.txt")
        aio.write_mixing_file(path, profiles, pdfs, 17)
        got_profiles, got_pdfs = aio.read_mixing_file(path)
        assert list(got_profiles) == ["heavy", "dye"] and (got_pdfs is None) == (not with_pdf)
        for k in profiles:
            same_table(got_profiles[k], profiles[k].table())
            if with_pdf:
                same_table(got_pdfs[k], pdfs[k].table())
        assert math.isnan(got_profiles["heavy"]["phi"][6]) and got_profiles["heavy"]["n"][6] == 0
    samples = [drawn_sample(s, 5 * s) for s in (1, 2, 3)]
    path = str(tmp_path / "series.txt")
    aio.write_mixing_series(path, samples, 17)
    t = aio.read_mixing_series(path)
    assert t["scalars"] == ["heavy", "dye"] and t["cycle"].tolist() == [5, 10, 15] and t["time"].tolist() == [s[1] for s in samples]
    for name in t["scalars"]:
        assert tuple(t[name]) == aio.MIXING_MEASURES
        for i, s in enumerate(samples):
            m = s[2][name].measures()
            for k in aio.MIXING_MEASURES:
                assert t[name][k][i] == m[k] or (math.isnan(m[k]) and math.isnan(t[name][k][i])), (name, k)
    assert len(open(path).read().splitlines()) == 2 + 3
    aio.write_mixing_series(path, [], 17)
    assert aio.read_mixing_series(path)["cycle"].size == 0
    # fewer digits: close, not equal
    aio.write_mixing_series(path, samples, 6)
    t6 = aio.read_mixing_series(path)
    assert np.allclose(t6["heavy"]["content"], t["heavy"]["content"], rtol=1e-6) and not np.array_equal(t6["heavy"]["content"], t["heavy"]["content"])


# ---- the run options -------------------------------------------------------------------------------------------------------
def tagged_problem(names=("heavy",)):
    from armon_amd import Problem, Scalar
    rho = np.ones((8, 8))
    zero = np.zeros((8, 8))
    tags = [Scalar(n, array=np.where(np.arange(8)[:, None] >= 4, 1.0, 0.0) * np.ones((8, 8))) for n in names]
    return Problem.from_arrays(rho, zero, zero, E=2.5 * rho, domain_size=(1.0, 1.0), scalars=tags)


def test_option_defaults_and_configuration_errors():
    p = ArmonParameters(test="Sod", N=(8, 8))
    assert (p.mixing_step, p.mixing_at_end, p.mixing_axis, p.mixing_bin_width, p.mixing_scalars, p.mixing_pdf_bins, p.mixing_pdf_range,
            p.mixing_file, p.state_mixing) == (0, False, "y", 1, None, 0, (0.0, 1.0), "mixing", False)
    for opts in (dict(mixing_step=2), dict(mixing_at_end=True), dict(mixing_scalars=["heavy"])):
        with pytest.raises(SolverException) as e:                # no scalars in this run
            ArmonParameters(test="Sod", N=(8, 8), **opts)
        assert e.value.category == "config", opts
    problem = tagged_problem(("heavy", "dye"))
    p = ArmonParameters(test=problem, N=(8, 8), mixing_step=3, mixing_axis="x", mixing_bin_width=2, mixing_scalars=["dye"],
                        mixing_pdf_bins=16, mixing_pdf_range=(-1, 2), output_dir="out", mixing_file="mix")
    assert p.state_mixing and p.mixing_scalars == ("dye",) and p.mixing_pdf_range == (-1.0, 2.0)
    assert mix.mixing_path(p, 12) == "out/mix_000012.txt" and mix.mixing_path(p) == "out/mix.txt"
    assert mix.make_spec(p, "x", 3) == (0, 3, 3, 0.125, 0.125, 8) and mix.make_spec(p, "y") == (1, 8, 1, 0.125, 0.125, 8)
    for bad in (dict(mixing_step=-1), dict(mixing_step=1.5), dict(mixing_step=True), dict(mixing_step="2"), dict(mixing_at_end=1),
                dict(mixing_axis="r"), dict(mixing_axis="Y"), dict(mixing_axis=1), dict(mixing_bin_width=0), dict(mixing_bin_width=-2),
                dict(mixing_bin_width=1.5), dict(mixing_bin_width=True), dict(mixing_scalars=["nobody"]), dict(mixing_scalars="heavy"),
                dict(mixing_scalars=[]), dict(mixing_scalars=["dye", "dye"]), dict(mixing_scalars=[3]), dict(mixing_pdf_bins=-1),
                dict(mixing_pdf_bins=1025), dict(mixing_pdf_bins=2.5), dict(mixing_pdf_bins=True), dict(mixing_pdf_range=(0.0,)),
                dict(mixing_pdf_range=(1.0, 0.0)), dict(mixing_pdf_range=(0.0, 0.0)), dict(mixing_pdf_range=(0.0, math.inf)),
                dict(mixing_pdf_range=(math.nan, 1.0)), dict(mixing_pdf_range=3), dict(mixing_file=""), dict(mixing_file="a/b"),
                dict(mixing_file=3)):
        with pytest.raises(SolverException) as e:
            ArmonParameters(test=problem, N=(8, 8), **bad)
        assert e.value.category == "config", bad
    for bad in (dict(axis="r"), dict(axis="y", width=0), dict(axis="y", width=1.5)):
        with pytest.raises(SolverException):
            mix.make_spec(p, **bad)


def test_the_options_are_refused_for_ranks(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    from armon_amd import Scalar
    ArmonParameters(test="Sod", N=(8, 8), use_MPI=True)
    for opts in (dict(mixing_step=2), dict(mixing_at_end=True)):
        with pytest.raises(SolverException) as e:                # (the scalars themselves are refused for ranks too, further on)
            ArmonParameters(test="Sod", N=(8, 8), use_MPI=True, scalars=[Scalar("heavy")], **opts)
        assert e.value.category == "config" and "use_MPI" in e.value.msg and "mixing_step" in e.value.msg


def test_graph_replay_steps_aside_and_stats_default():
    from armon_amd import solver
    src = open(solver.__file__).read()
    body = src[src.index("def graph_cycles_usable"):src.index("def time_loop_graph")]
    assert body.index("params.state_mixing") < body.index("params.scalar_names")     # asked on its own, before the scalars' own refusal

    def usable(**kw):
        p = ArmonParameters(test=tagged_problem(), N=(8, 8), graph_cycles=True, silent=5, **kw)
        p._device = types.SimpleNamespace(owns_ctx=True)
        p.scalar_names = ()                                     # (so that only the option under test can refuse)
        return graph_cycles_usable(p)
    assert usable(mixing_step=2) is False and usable(mixing_at_end=True) is False
    assert usable(mixing_axis="x", mixing_pdf_bins=8) is True   # the other options alone ask for nothing
    assert SolverStats(0.0, 0.0, 0, 0.0, 0, 0.0).mixing == []
