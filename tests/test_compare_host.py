"""State comparison, the parts that need no GPU: the per-cell rule restated in numpy (compare.cell_rule / diff_reference — the
listing's cell picker and the GPU tests' oracle), the merge, the decoding, the report, the options and the header check."""
import ctypes as C
import itertools
import types

import numpy as np
import pytest

import armon_amd
from armon_amd import checkpoint as ck
from armon_amd import compare as cmp
from armon_amd._lib import SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import SolverStats, graph_cycles_usable

NONE = (1 << 64) - 1


def bits64(v):
    return int(np.float64(v).view(np.uint64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_rule_on_hand_made_pairs(dtype):
    T = dtype
    eps, tiny = np.finfo(dtype).eps, np.finfo(dtype).smallest_subnormal
    U = np.uint64 if dtype is np.float64 else np.uint32
    quiet = 0x7ff8000000000000 if dtype is np.float64 else 0x7fc00000
    nan, inf = T(np.nan), T(np.inf)
    #            ours       ref        bits   out    d                  rel
    cases = [(T(0.0), T(-0.0), True, False, T(0), T(0)),                      # the sign of a zero: bits only
             (T(1.5), T(1.5), False, False, T(0), T(0)),
             (nan, T(1.0), True, True, nan, nan),                             # one NaN
             (T(1.0), nan, True, True, nan, nan),
             (nan, nan, False, False, T(0), T(0)),                            # two NaNs: equal
             (inf, inf, False, False, T(0), T(0)),                            # the same infinity: equal, d = 0 (not inf - inf)
             (inf, -inf, True, True, inf, nan),                               # opposite infinities: d = inf, inf / inf
             (inf, T(1.0), True, True, inf, nan),
             (tiny, T(0.0), True, True, tiny, T(1)),                          # a subnormal against zero: rel = 1
             (tiny, T(2) * tiny, True, True, tiny, T(0.5)),
             (T(1.0), T(1.0) + eps, True, True, eps, eps / (T(1.0) + eps))]   # 1 ulp, rtol = 0
    for a, b, bits, out, d, rel in cases:
        got = cmp.cell_rule(np.array([a]), np.array([b]), 0.0, 0.0)
        want_d = quiet if np.isnan(d) else int(np.array([d], dtype=dtype).view(U)[0])
        want_rel = quiet if np.isnan(rel) else int(np.array([rel], dtype=dtype).view(U)[0])
        assert (bool(got[0][0]), bool(got[1][0]), int(got[2][0]), int(got[3][0])) == (bits, out, want_d, want_rel), (a, b)
    # a negative-sign NaN is canonicalised too
    neg_nan = np.array([quiet | (1 << (63 if dtype is np.float64 else 31)) | 5], dtype=U).view(dtype)
    assert int(cmp.cell_rule(neg_nan, np.array([T(1)]), 0.0, 0.0)[2][0]) == quiet
    # exactly at the threshold: d <= max(atol, rtol m) holds with equality, and fails one ulp above
    a, b = T(1.0), T(1.0) + T(4) * eps                                        # d = 4 eps, m = 1 + 4 eps
    d, m = abs(a - b), max(abs(a), abs(b))
    rtol = float(d / m)
    while T(rtol) * m < d:                                                    # the smallest rtol whose product reaches d
        rtol = float(np.nextafter(T(rtol), T(1)))
    assert T(rtol) * m >= d and not cmp.cell_rule(np.array([a]), np.array([b]), rtol, 0.0)[1][0]
    below = float(np.nextafter(T(rtol), T(0)))
    if T(below) * m < d:
        assert cmp.cell_rule(np.array([a]), np.array([b]), below, 0.0)[1][0]
    assert not cmp.cell_rule(np.array([a]), np.array([b]), 0.0, float(d))[1][0]                      # atol == d: within
    assert cmp.cell_rule(np.array([a]), np.array([b]), 0.0, float(np.nextafter(d, T(0))))[1][0]       # one ulp less: out


def test_diff_reference_counts_positions_and_ties():
    ours = np.zeros((3, 4))
    ref = ours.copy()
    ref[0, 3] = 1e-3            # g = 3 (+ origin)
    ref[2, 1] = 1e-3            # g = 9: the same value later — the smaller position keeps the maximum
    ref[1, 2] = -0.0            # bits only
    r = cmp.diff_reference(ours, ref, 0.0, 0.0)
    assert r == (12, 3, 2, 3, bits64(1e-3), 3, bits64(1.0), 3)
    r = cmp.diff_reference(ours, ref, 0.0, 0.0, global_nx=10, origin=(5, 2))
    assert r[3] == 2 * 10 + 5 + 3 and r[5] == r[3] and r[0] == 12
    assert cmp.diff_reference(ours, ours, 0.0, 0.0) == (12, 0, 0, NONE, 0, NONE, 0, NONE)
    assert cmp.diff_reference(ours, ref, 0.0, 1e-3)[1:4] == (3, 0, NONE)                             # within atol: bits, not out


def drawn_records(rng, n):
    """Records with many ties: few distinct values and positions."""
    out = []
    for _ in range(n):
        def pair():
            v = int(rng.choice([0, 0, 5, 5, 9]))
            return (v, NONE if v == 0 else int(rng.choice([1, 2, 2, 7])))
        n_out = int(rng.integers(0, 3))
        out.append((int(rng.integers(1, 50)), int(rng.integers(0, 5)), n_out, NONE if n_out == 0 else int(rng.choice([0, 3, 3, 8])))
                   + pair() + pair())
    return out


def test_merge_is_associative_and_commutative_with_ties():
    rng = np.random.default_rng(7)
    recs = drawn_records(rng, 40) + [cmp.NEUTRAL]
    for x, y, z in itertools.islice(itertools.product(recs, repeat=3), 0, None, 97):
        assert cmp.merge_raw(x, y) == cmp.merge_raw(y, x)
        assert cmp.merge_raw(cmp.merge_raw(x, y), z) == cmp.merge_raw(x, cmp.merge_raw(y, z))
        assert cmp.merge_raw(x, cmp.NEUTRAL) == x
    # by hand: the larger value wins; on equal values the smaller position; sums and the minimum
    a = (10, 1, 1, 8, 5, 7, 9, 2)
    b = (4, 2, 1, 3, 5, 2, 5, 1)
    assert cmp.merge_raw(a, b) == (14, 3, 2, 3, 5, 2, 9, 2)
    # StateDiff.merge: the same on objects, listings united and cut to the smallest indices
    mk = lambda raw, cells: cmp.StateDiff({"u": cmp.VarDiff(raw, np.float64, 10, cells)}, limit=3)
    A = mk(a, [(8, 1.0, 2.0), (12, 1.0, 2.0)])
    B = mk(b, [(3, 0.0, 1.0), (9, 0.0, 1.0)])
    C_ = mk(cmp.NEUTRAL, [])
    assert A.merge(B) == B.merge(A) and A.merge(B).merge(C_) == A.merge(B.merge(C_))
    assert A.merge(B)["u"].raw == (14, 3, 2, 3, 5, 2, 9, 2) and [c[0] for c in A.merge(B)["u"].cells] == [3, 8, 9]
    assert A.different and not C_.different


def test_decoding_of_values_and_positions():
    v = cmp.VarDiff((100, 2, 1, 0, bits64(0.25), 37, bits64(np.inf), 99), np.float64, 10)
    assert (v.n_cells, v.n_bits, v.n_out) == (100, 2, 1)
    assert v.first_out == (1, 1)                       # g = 0: the first cell, 1-based like the reference's print-outs
    assert v.max_abs == 0.25 and v.max_abs_at == (8, 4)     # g = 37 = 3 * 10 + 7
    assert v.max_rel == np.inf and v.max_rel_at == (10, 10)
    w = cmp.VarDiff((4, 0, 0, NONE, 0, NONE, 0x7fc00000, 3), np.float32, 2)
    assert w.first_out is None and w.max_abs == 0.0 and w.max_abs_at is None and np.isnan(w.max_rel) and w.max_rel_at == (2, 2)


def test_report_layout():
    v = cmp.VarDiff((100, 3, 2, 12, bits64(0.5), 12, bits64(1.0), 12), np.float64, 10, [(12, 1.0, 1.5), (47, 0.0, 0.25)])
    quiet = cmp.VarDiff((100, 0, 0, NONE, 0, NONE, 0, NONE), np.float64, 10)
    text = cmp.StateDiff({"rho": quiet, "u": v}, limit=20).report("cycle 4").split("\n")
    assert text[0] == "At cycle 4:"
    assert text[1] == "  2 differences found in u"
    assert text[2] == f"   - (  3,  2): {1.0:12.5g} ≢ {1.5:12.5g} ({-0.5:12.5g})"            # io.compare_host's line
    assert text[3] == f"   - (  8,  5): {0.0:12.5g} ≢ {0.25:12.5g} ({-0.25:12.5g})"
    assert "max |Δu| = 0.5 at (3, 2)" in text[4] and "1 at (3, 2)" in text[4] and len(text) == 5
    assert not any("rho" in t for t in text)
    timed = cmp.StateDiff({"rho": quiet}, time=(0.5, 0.25)).report("end")
    assert timed.split("\n")[1].startswith("Time difference: ref t = 0.5") and cmp.StateDiff({"rho": quiet}, time=(0.5, 0.25)).different
    assert len(cmp.StateDiff({"u": v}, limit=1).report("x").split("\n")) == 4


class FakeTile:
    """What the lister needs of a tile, on the host: ``gather`` hands out rows of a padded array and counts them."""

    def __init__(self, ours, origin, global_nx, ghosts=2):
        ny, nx = ours.shape
        self.padded = np.full((ny + 2 * ghosts, nx + 2 * ghosts), np.nan)
        self.padded[ghosts:ghosts + ny, ghosts:ghosts + nx] = ours
        self.size = types.SimpleNamespace(ghosts=ghosts, size=(nx + 2 * ghosts, ny + 2 * ghosts))
        self.params = types.SimpleNamespace(N=(nx, ny), N_origin=(origin[0] + 1, origin[1] + 1), global_grid=(global_nx, None))
        self.gathers = 0

    def gather(self, names, start, stride, count):
        assert stride == 1
        self.gathers += 1
        return {names[0]: self.padded.reshape(-1)[start:start + count].copy()}


def list_bands(lister, tile, ours, ref, band_rows, rtol=0.0):
    """Walk a tile as the second pass does: the bands the lister wants, with numpy's per-row counts → bands looked at."""
    ny, nx = ours.shape
    _, out, _, _ = cmp.cell_rule(ours, ref, rtol, 0.0)
    g = np.arange(ny)[:, None] * 0 + out                                   # (bool) the out-of-tolerance cells
    ox, oy = tile.params.N_origin[0] - 1, tile.params.N_origin[1] - 1
    gs = (np.arange(ny)[:, None] + oy) * tile.params.global_grid[0] + np.arange(nx)[None, :] + ox
    lister.tile(tile.params, tile, [(nx * ny, int(out.sum()), int(out.sum()), int(gs[out].min()) if out.any() else NONE, 0, NONE, 0, NONE)])
    looked = 0
    for r0 in range(0, ny, band_rows):
        rows = min(band_rows, ny - r0)
        window = (0, r0, nx, rows)
        if not lister.wants(window):
            continue
        looked += 1
        lister.band(window, g[r0:r0 + rows].sum(axis=1)[None, :], lambda q, r, r0=r0: ref[r0 + r])
    return looked


def test_the_listing_is_bounded_by_the_limit_however_many_cells_differ():
    rng = np.random.default_rng(5)
    ours, ref = rng.normal(size=(64, 40)), rng.normal(size=(64, 40))           # every cell differs
    for limit, rows_needed in ((3, 1), (40, 1), (41, 2), (100, 3)):
        tile = FakeTile(ours, (0, 0), 40)
        lister = cmp._Lister(("u",), 0.0, 0.0, limit)
        assert list_bands(lister, tile, ours, ref, band_rows=8) == 1                # one band of eight, not all of them
        assert tile.gathers == lister.rows_fetched == rows_needed
        assert lister.cells["u"] == [(g, float(ref.reshape(-1)[g]), float(ours.reshape(-1)[g])) for g in range(limit)]
    # a few cells late in the tile: the bands before the first of them are never looked at, nor the ones after the last
    ref = ours.copy()
    planted = [(50, 3), (50, 39), (51, 0), (57, 7)]
    for iy, ix in planted:
        ref[iy, ix] += 1.0
    tile, lister = FakeTile(ours, (0, 0), 40), cmp._Lister(("u",), 0.0, 0.0, 3)
    assert list_bands(lister, tile, ours, ref, band_rows=8) == 1 and tile.gathers == 2
    assert [c[0] for c in lister.cells["u"]] == [50 * 40 + 3, 50 * 40 + 39, 51 * 40]
    # two tiles side by side (columns 0-19 and 20-39 of one domain), the right one first: the smallest indices win, in any
    # order of the pieces, and a tile that starts after the cells held is not walked at all
    ours, ref = rng.normal(size=(16, 40)), rng.normal(size=(16, 40))
    lister = cmp._Lister(("u",), 0.0, 0.0, 25)
    right, left = FakeTile(ours[:, 20:], (20, 0), 40), FakeTile(ours[:, :20], (0, 0), 40)
    list_bands(lister, right, ours[:, 20:], ref[:, 20:], band_rows=4)
    list_bands(lister, left, ours[:, :20], ref[:, :20], band_rows=4)
    assert [c[0] for c in lister.cells["u"]] == list(range(25))
    assert right.gathers == 2 and left.gathers == 1                                 # right: rows 0, 1 (20 + 5); left: row 0
    lister = cmp._Lister(("u",), 0.0, 0.0, 5)
    list_bands(lister, left, ours[:, :20], ref[:, :20], band_rows=4)
    lister.tile(right.params, right, [(320, 320, 320, 20, 0, NONE, 0, NONE)])
    assert not lister.wants((0, 0, 20, 16))


def test_option_defaults_and_configuration_errors():
    p = ArmonParameters(test="Sod", N=(8, 8))
    assert (p.compare_step, p.compare_dir, p.compare_file, p.compare_at_end, p.comparison_atol) == (0, None, "checkpoint", False, 0.0)
    assert p.use_fused_sweep and not p.state_compare and p.comparison_time_atol == 0.0
    p = ArmonParameters(test="Sod", N=(8, 8), compare_step=4, compare_dir="ref", compare_file="ck", compare_at_end=True,
                        comparison_atol={"rho": 1e-11, "u": 0})
    assert p.use_fused_sweep                                      # the fused sweep stays on
    assert cmp.compare_path(p, 12) == "ref/ck_000012.ckpt" and p.comparison_atol == {"rho": 1e-11, "u": 0.0}
    for bad in (dict(compare_step=2, compare_dir="d", compare=True), dict(compare_at_end=True, compare_dir="d", is_ref=True, compare=True),
                dict(compare_dir="d", compare=True), dict(compare_step=2), dict(compare_at_end=True), dict(compare_step=-1, compare_dir="d"),
                dict(compare_step=1.5, compare_dir="d"), dict(compare_step=True, compare_dir="d"), dict(compare_file="", compare_dir="d"),
                dict(comparison_atol=-1.0), dict(comparison_atol=float("nan")), dict(comparison_time_atol=-1.0),
                dict(comparison_time_atol=float("nan")), dict(comparison_time_atol="1")):
        with pytest.raises(SolverException) as e:
            ArmonParameters(test="Sod", N=(8, 8), **bad)
        assert e.value.category == "config", bad


def test_the_new_options_are_refused_for_ranks(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    ArmonParameters(test="Sod", N=(8, 8), use_MPI=True)
    with pytest.raises(SolverException) as e:
        ArmonParameters(test="Sod", N=(8, 8), use_MPI=True, compare_step=2, compare_dir="d")
    assert e.value.category == "config" and "use_MPI" in e.value.msg


def test_graph_replay_steps_aside_and_stats_default():
    def usable(**kw):
        p = ArmonParameters(test="Sod", N=(8, 8), graph_cycles=True, silent=5, **kw)
        p._device = types.SimpleNamespace(owns_ctx=True)
        return graph_cycles_usable(p)
    assert usable() is True
    assert usable(compare_step=2, compare_dir="d") is False
    assert usable(compare_at_end=True, compare_dir="d") is False
    assert usable(compare_dir="d") is False
    assert SolverStats(0.0, 0.0, 0, 0.0, 0, 0.0).state_diffs == []


def test_header_compatibility_names_the_field():
    base = dict(test="Sod", N=(16, 16))
    mine = ArmonParameters(**base)
    for field, other in (("N", dict(N=(8, 10))), ("data_type", dict(data_type=np.float32))):
        h = ck.bit_options(ArmonParameters(**{**base, **other}))
        with pytest.raises(SolverException) as e:
            cmp.check_comparable(mine, h["N"], h["data_type"], "the checkpoint x.ckpt")
        assert e.value.category == "config" and field in e.value.msg
    # every bit-deciding option may differ: that is what a comparison is for
    for other in (dict(scheme="Godunov"), dict(exact_arithmetic=True), dict(use_fused_sweep=False), dict(nghost=6),
                  dict(riemann_limiter="superbee"), dict(tile_of=(1, (2, 2)))):
        h = ck.bit_options(ArmonParameters(**{**base, **other}))
        cmp.check_comparable(mine, h["N"], h["data_type"], "x")


def test_new_entry_points_are_bound_and_refuse_a_null_context():
    from armon_amd._lib import SIGNATURES, StateDiff
    assert C.sizeof(StateDiff) == 64
    for name in ("state_compare", "state_compare_f32", "state_diff_reset"):
        assert "armon_hip_" + name in SIGNATURES
    L = armon_amd.lib()
    vars_ = (C.c_void_p * 1)()
    for fn in (L.armon_hip_state_compare, L.armon_hip_state_compare_f32):
        assert fn(None, 16, 4, 8, 8, 1, vars_, 0, 0, 8, 8, 0, 8, None, 0.0, 0.0, None, None) == 1
    assert L.armon_hip_state_diff_reset(None, 1, None) == 1
