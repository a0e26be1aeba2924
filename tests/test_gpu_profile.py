"""In-situ profiles on the GPU: armon_hip_profile / armon_hip_profile_bounds and the Python surface over them
(BlockGrid.profile, TileGroup.profile, the profile_* options).

The oracle is profile.reference_record: profile.cell_terms / quantise / limbs applied cell by cell to the downloaded real
cells. Everything is compared WORD FOR WORD — the 24 words of every bin — never within a tolerance: every addend is rounded
once to an integer and integer sums have no order. The pressure the oracle bins is the library's own staged EOS kernel
applied to the state (existing tests pin that kernel to the CPU oracle); the profile kernel reads no p vector."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
DTYPES = ["float64", "float32"]
CASES = ["Sod", "Sedov", "Bizarrium"]
SMALL = [((37, 39), 5), ((64, 24), 4), ((300, 21), None), ((130, 1), None), ((1, 130), None)]     # (N, nghost): see the issue's table
BIG = (777, 150)

_states = {}


def state_of(test, N, dtype, **kw):
    """A grid 6 fused cycles into ``test``, with p = the staged EOS kernel of that state. Cached: many cases share one run."""
    import armon_amd
    from armon_amd.solver import update_EOS
    from armon_amd.solver import BlockGrid, init_test
    key = (test, N, dtype, tuple(sorted(kw.items())))
    if key not in _states:
        kw = {k: v for k, v in kw.items() if v is not None}
        if min(N) >= 4:
            params = armon_amd.ArmonParameters(test=test, N=N, data_type=dtype, maxcycle=6, silent=5, return_data=True, **kw)
            grid = armon_amd.armon(params).data
        else:
            # The solver refuses to sweep an axis of fewer than 4 cells (its mirror boundary needs them), so a one-row or
            # one-column block cannot be advanced: it is given row 11 / column 11 of a 24-wide run 6 cycles in instead.
            wide = (N[0], 24) if N[1] == 1 else (24, N[1])
            donor = real_fields(state_of(test, wide, dtype, **kw), STATE)
            params = armon_amd.ArmonParameters(test=test, N=N, data_type=dtype, silent=5, **kw)
            grid = BlockGrid(params)
            init_test(params, grid)
            host = grid.device_to_host(STATE)
            for k in STATE:
                grid.real_view(host[k])[...] = donor[k][11:12, :] if N[1] == 1 else donor[k][:, 11:12]
            grid.host_to_device(host)
        update_EOS(params, grid)                    # writes p, c, g only: the state the profile reads is untouched
        _states[key] = grid
    return _states[key]


@pytest.fixture(scope="module", autouse=True)
def release_states():
    yield
    _states.clear()


def real_fields(grid, names=STATE + ("p",)):
    host = grid.device_to_host(names)
    return {k: grid.real_view(host[k]).copy() for k in names}


def set_wgs(grid, n):
    dev = grid.params.device
    assert dev._L.armon_hip_set_tuning(dev.ctx, b"PROFILE_WGS", int(n)) == 0
    assert dev.get_tuning("PROFILE_WGS") == int(n)


def geometry(spec):
    return dict(width=spec[3], cx=spec[4], cy=spec[5], dx=spec[6], dy=spec[7], inv_dr=spec[8])


def oracle_record(P, f, origin=(0, 0), skip=None):
    """The record of the fields ``f`` under the spec and scale of the profile ``P``, by the host rule."""
    from armon_amd import profile as prof
    return prof.reference_record(P.spec[0], P.nbins, P.scale_exp, f["rho"], f["u"], f["v"], f["E"], f["p"] if P.with_p else None,
                                 origin=origin, skip=skip, **geometry(P.spec))


def same_words(P, want, what):
    got = P.raw
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        b, w = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words differ, first in bin {b} word {w}: {int(got[b, w]):#x} != {int(want[b, w]):#x}")
    assert not got[:, 21:].any()                                       # reserved words stay zero


def off_centre(params):
    """A centre that is no cell centre, a third of the way into the domain."""
    return (params.origin[0] + 0.3713 * params.domain_size[0], params.origin[1] + 0.6291 * params.domain_size[1])


def configurations(params):
    """(kind, keywords): widths 1, 7 and one wider than the grid; R with the default and an off-centre centre, rings of 1, 2.5
    and 40 cells, and bins cut short so that far cells are skipped."""
    dx = float(params.cell_size(0))
    wide = max(params.N) + 50
    out = [(k, dict(width=w)) for k in "xy" for w in (1, 7, wide)]
    out += [("r", {}), ("r", dict(centre=off_centre(params))), ("r", dict(dr=dx)), ("r", dict(dr=2.5 * dx, centre=off_centre(params))),
            ("r", dict(dr=40 * dx)), ("r", dict(bins=5, dr=1.5 * dx)), ("x", dict(width=3, bins=4)), ("y", dict(width=1, with_p=False))]
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", CASES)
@pytest.mark.parametrize("N,nghost", SMALL)
def test_exact_against_the_host_rule(N, nghost, test, dtype):
    grid = state_of(test, N, dtype, nghost=nghost)
    set_wgs(grid, 0)
    f = real_fields(grid)
    for kind, kw in configurations(grid.params):
        P = grid.profile(kind, **kw)
        same_words(P, oracle_record(P, f), (kind, kw))
        skipped = N[0] * N[1] - int(P.n.sum()) - int(P.n_bad.sum())
        assert (skipped == 0 or "bins" in kw) and int(P.n_bad.sum()) == 0, (kind, kw, skipped)


@pytest.mark.parametrize("kind", ["x", "y", "r"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", CASES)
def test_exact_when_every_workgroup_walks_many_tiles(test, dtype, kind):
    """777 x 150 with PROFILE_WGS = 3: 7 (4 in fp32) spans x 5 row blocks = 35 (20) tiles for 3 workgroups, a ragged last span,
    a ragged last row block, and table bases that change inside a workgroup's run."""
    grid = state_of(test, BIG, dtype)
    set_wgs(grid, 3)
    try:
        kw = dict(width=16) if kind != "r" else dict(centre=off_centre(grid.params), dr=2.5 * float(grid.params.cell_size(0)))
        P = grid.profile(kind, **kw)
    finally:
        set_wgs(grid, 0)
    same_words(P, oracle_record(P, real_fields(grid)), (kind, kw))
    assert int(P.n.sum()) == BIG[0] * BIG[1]


@pytest.mark.parametrize("wgs", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nghost", [4, 5])
@pytest.mark.parametrize("test", ["Sedov", "Sod"])
def test_exact_when_rings_leave_the_lds_table(test, nghost, dtype, wgs):
    """Rings four times finer than a cell (dr = dx / 4) around an off-centre centre, on 300 x 40: a span of 128 (fp64) or 256
    (fp32) columns crosses 500 to 1000 rings where the LDS table holds 264, so most lane records go straight to bins_dev
    (asserted on the bins of every tile below); the default bins skip no cell. nghost 4 takes the 16-B path, 5 the element
    path. With PROFILE_WGS = 1 one workgroup walks every tile and the table's first bin changes with every tile."""
    from armon_amd import profile as prof
    N = (300, 40)
    grid = state_of(test, N, dtype, nghost=nghost)
    params = grid.params
    set_wgs(grid, wgs)
    try:
        P = grid.profile("r", centre=off_centre(params), dr=float(params.cell_size(0)) / 4)
    finally:
        set_wgs(grid, 0)
    f = real_fields(grid)
    # a tile's table starts at or below the tile's smallest bin and holds 264: a cell 264 bins above that is outside it
    b, _ = prof.cell_terms("r", f["rho"], f["u"], f["v"], f["E"], None, np.arange(N[0])[None, :], np.arange(N[1])[:, None], **geometry(P.spec))
    span = 128 if dtype == "float64" else 256
    for y in range(0, N[1], 32):
        for x in range(0, N[0], span):
            tile = b[y:y + 32, x:x + span]
            assert (tile >= tile.min() + 264).any() or tile.shape[1] < 64, (x, y)
    same_words(P, oracle_record(P, f), (test, nghost, dtype, wgs))
    assert int(P.n.sum()) == N[0] * N[1] and int(P.n_bad.sum()) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_windows_knobs_and_repeats_change_no_word(dtype):
    from armon_amd import profile as prof
    grid = state_of("Sedov", (300, 21), dtype)
    params = grid.params
    tile = (params, grid)
    for kind, kw in (("x", dict(width=7)), ("y", dict(width=2)), ("r", dict(dr=2.5 * float(params.cell_size(0))))):
        set_wgs(grid, 0)
        whole = grid.profile(kind, **kw)
        assert grid.profile(kind, **kw) == whole                       # two calls
        # two half-windows split at an odd column (the second one starts off the 16-B grid), and at an odd row
        for windows in ([(0, 0, 131, 21), (131, 0, 169, 21)], [(0, 0, 300, 5), (0, 5, 300, 16)],
                        [(0, 0, 1, 21), (1, 0, 299, 11), (1, 11, 299, 10)]):
            parts = prof.profile_state([tile] * len(windows), kind, windows=windows, **kw)
            assert parts.scale_exp == whole.scale_exp
            same_words(parts, whole.raw, (kind, windows))
        try:
            for wgs in (1, 3):
                set_wgs(grid, wgs)
                same_words(grid.profile(kind, **kw), whole.raw, (kind, "PROFILE_WGS", wgs))
        finally:
            set_wgs(grid, 0)


@pytest.mark.parametrize("native_cycle", [True, False])
@pytest.mark.parametrize("N", [(97, 61), (100, 60)])
def test_tile_groups_give_the_single_block_record(N, native_cycle):
    """Exact arithmetic: the tiles hold the single block's bits (asserted), so the merged record must be the single block's,
    word for word, for every kind — an R centre inside one tile, a dr that lines up with no tile boundary."""
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    kw = dict(test="Sedov", N=N, maxcycle=6, silent=5, exact_arithmetic=True)
    ref = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **kw)).data
    single = real_fields(ref, STATE)
    dx = float(ref.params.cell_size(0))
    asks = [("x", dict(width=7)), ("y", dict(width=1)), ("r", {}), ("r", dict(centre=off_centre(ref.params), dr=1.7 * dx)),
            ("r", dict(centre=off_centre(ref.params), dr=3.3 * dx, bins=9, with_p=False))]
    want = [ref.profile(kind, **a) for kind, a in asks]
    for P in ((2, 2), (3, 1), (1, 3)):
        group = TileGroup(P, native_cycle=native_cycle, **kw)
        try:
            group.run()
            tiles = group.gather(STATE)
            for k in STATE:
                assert np.array_equal(tiles[k], single[k]), (P, k)     # the premise
            for (kind, a), w in zip(asks, want):
                got = group.profile(kind, **a)
                assert got.scale_exp == w.scale_exp and got.spec == w.spec
                same_words(got, w.raw, (P, kind, a))
        finally:
            group.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_field_under_another_ghost_width_gives_the_same_record(dtype):
    """The same real cells in a block with 6 ghost layers instead of 4: every row lands elsewhere."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test
    for N in ((97, 61), (100, 60)):
        grid = state_of("Sedov", N, dtype)
        f = real_fields(grid, STATE)
        params6 = armon_amd.ArmonParameters(test="Sedov", N=N, data_type=dtype, nghost=6, silent=5)
        other = BlockGrid(params6)
        init_test(params6, other)
        host = other.device_to_host(STATE)
        for k in STATE:
            other.real_view(host[k])[...] = f[k]
        other.host_to_device(host)
        for kind, kw in (("x", dict(width=3)), ("y", {}), ("r", dict(centre=off_centre(grid.params)))):
            a, b = grid.profile(kind, **kw), other.profile(kind, **kw)
            assert a.scale_exp == b.scale_exp
            same_words(b, a.raw, (N, kind))


def plant(grid, cells):
    """Write ``value`` into variable ``name`` at the real cell (ix, iy), for every (name, ix, iy, value)."""
    host = grid.device_to_host(STATE)
    for name, ix, iy, value in cells:
        grid.real_view(host[name])[iy, ix] = value
    grid.host_to_device(host)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["x", "r"])
def test_bad_cells_are_counted_and_left_out(kind, dtype):
    import armon_amd
    from armon_amd.solver import update_EOS
    params = armon_amd.ArmonParameters(test="Sedov", N=(64, 24), data_type=dtype, maxcycle=6, silent=5, return_data=True)
    grid = armon_amd.armon(params).data
    plant(grid, [("rho", 10, 3, math.nan), ("E", 41, 17, math.inf)])
    update_EOS(params, grid)
    f = real_fields(grid)
    skip = np.zeros((24, 64), dtype=bool)
    skip[3, 10] = skip[17, 41] = True
    P = grid.profile(kind, width=4) if kind == "x" else grid.profile(kind)
    assert int(P.n_bad.sum()) == 2 and int(P.n.sum()) == 64 * 24 - 2
    want = oracle_record(P, f, skip=skip)
    assert not want[:, 1].any()                                        # the oracle with those two cells left out has no bad cell
    got = P.raw.copy()
    got[:, 1] = 0
    assert np.array_equal(got, want)
    same_words(P, oracle_record(P, f), kind)                           # and with them in, it counts them where the kernel does


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_explicit_scale_too_small_for_rho_refuses_the_cells_above_it(dtype):
    import armon_amd
    grid = state_of("Sod", (64, 24), dtype)
    f = real_fields(grid)
    auto = grid.profile("x", width=4)
    # quanta of 2^-96: rho >= 0.5 reaches 2^95 quanta and is bad, Sod's low side (0.125 and the fan below 0.5) is not
    scale = (-96,) + auto.scale_exp[1:]
    P = grid.profile("x", width=4, scale_exp=scale)
    rho = f["rho"].astype(np.float64)
    assert P.scale_exp == scale and int(P.n_bad.sum()) == int((rho >= 0.5).sum()) and 0 < int(P.n_bad.sum()) < rho.size
    assert int(P.n.sum()) == int((rho < 0.5).sum())
    same_words(P, oracle_record(P, f), "scale")
    with pytest.raises(armon_amd.SolverException) as e:
        grid.profile("x", scale_exp=(0, 0, 0, 0))
    assert e.value.category == "config"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", CASES)
def test_bounds_are_the_largest_finite_terms(test, dtype):
    from armon_amd import profile as prof
    grid = state_of(test, (37, 39), dtype, nghost=5)
    params = grid.params
    f = real_fields(grid)
    gx, gy = np.arange(37)[None, :], np.arange(39)[:, None]
    for kind, kw in (("x", {}), ("y", {}), ("r", dict(centre=off_centre(params), bins=3))):      # cells past the last bin count too
        spec = prof.make_spec(params, kind, **kw)
        _, t = prof.cell_terms(kind, f["rho"], f["u"], f["v"], f["E"], f["p"], gx, gy, **geometry(spec))
        want = tuple(int(np.array([np.abs(a[np.isfinite(a)]).max()]).view(np.uint64)[0]) for a in t)
        assert prof.state_bounds([(params, grid)], spec) == want, kind
        assert grid.profile(kind, **kw).scale_exp == prof.default_scale(want)


def test_bounds_skip_what_is_not_finite():
    import armon_amd
    from armon_amd import profile as prof
    params = armon_amd.ArmonParameters(test="Sod", N=(64, 24), maxcycle=2, silent=5, return_data=True)
    grid = armon_amd.armon(params).data
    clean = prof.state_bounds([(params, grid)], prof.make_spec(params, "x"))
    plant(grid, [("rho", 5, 5, math.inf), ("u", 9, 2, math.nan)])
    assert prof.state_bounds([(params, grid)], prof.make_spec(params, "x")) == clean


@pytest.mark.parametrize("test,kind", [("Sod", "x"), ("Sod_y", "y")])
def test_a_one_dimensional_case_profiles_to_its_own_row(test, kind):
    """Sod varies along x only: every row is the same row (asserted), every rho is a multiple of the quantum (asserted), so the
    mean over a column is the column's value, bit for bit."""
    from armon_amd import profile as prof
    grid = state_of(test, (64, 24), "float64", exact_arithmetic=True)
    rho = real_fields(grid, ("rho",))["rho"]
    line = rho[0] if kind == "x" else rho[:, 0]
    assert np.array_equal(rho, np.broadcast_to(line if kind == "x" else line[:, None], rho.shape))
    P = grid.profile(kind, width=1)
    assert all(prof.quantise(float(x), P.scale_exp[0]) * quantum(P.scale_exp[0]) == exact(x) for x in line)
    assert P.rho.tobytes() == line.tobytes()
    assert P.rho_min.tobytes() == line.tobytes() and P.rho_max.tobytes() == line.tobytes()
    assert np.all(P.ut == 0.0) and P.n.tolist() == [rho.shape[0] if kind == "x" else rho.shape[1]] * len(line)


def quantum(s):
    return Fraction(2) ** s


def exact(x):
    return Fraction(float(x))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", ["Sod", "Sedov"])
def test_the_bins_hold_the_mass(test, dtype):
    """S_b S0 is the exact integer sum of quantise(rho); times the quantum and the cell area it is the mass conservation_vars
    returns, within (n + 2) eps S|rho| dx dy: the bound of an any-order sum of n terms in the run's type (tests/test_gpu_insitu.py)."""
    from armon_amd import profile as prof
    from armon_amd.solver import conservation_vars
    grid = state_of(test, (300, 21), dtype)
    params = grid.params
    rho = real_fields(grid, ("rho",))["rho"].astype(np.float64)
    n = rho.size
    for kind in "xyr":
        P = grid.profile(kind, width=7)
        s = P.scale_exp[0]
        total = sum(P.sums[0])
        assert total == sum(prof.quantise(float(x), s) for x in rho.ravel()), kind
        ds = exact(params.cell_size(0)) * exact(params.cell_size(1))
        mass, _ = conservation_vars(params, grid)
        bound = (n + 2) * float(np.finfo(params.data_type).eps) * float(np.abs(rho).sum()) * float(ds)
        err = abs(float(total * quantum(s) * ds - exact(mass)))
        print(f"{test} {dtype} {kind}: |mass - profile| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (kind, err, bound)


def test_sedov_stays_radial():
    """Sedov on a square grid around the default centre is symmetric under the reflections of the square, so the mass-weighted
    tangential velocity of a ring vanishes up to rounding: |ut| <= 1.3e-14 max|un| in every bin that has cells. The bound is
    10 x what the CPU oracle's own state shows at this size and cycle (96 x 96, 6 cycles, fp64: max|ut| = 5.50e-15 against
    max|un| = 4.362, a ratio of 1.26e-15, evaluated with profile.reference_record on the oracle's fields); the exact flavour
    computes the oracle's bits."""
    grid = state_of("Sedov", (96, 96), "float64", exact_arithmetic=True)
    P = grid.profile("r")
    has = P.n > 0
    un, ut = np.abs(P.un[has]), np.abs(P.ut[has])
    print(f"max|ut| = {ut.max():.3e}, max|un| = {un.max():.3e}, ratio {ut.max() / un.max():.3e}")
    assert has.sum() > 60 and un.max() > 1.0
    assert np.all(ut <= 1.3e-14 * un.max())


def same_table(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k
        else:
            assert a[k] == b[k], k


def test_end_to_end_files_stats_and_an_unchanged_run(tmp_path):
    import armon_amd
    from armon_amd import io as aio
    from armon_amd.multi_tile import TileGroup
    from armon_amd.solver import graph_cycles_usable
    base = dict(test="Sedov", N=(96, 96), maxcycle=9, silent=5, exact_arithmetic=True)
    plain = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **base))
    out = str(tmp_path / "single")
    stats = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, profile_step=3, profile_kind="r", output_dir=out, **base))
    assert sorted(os.listdir(out)) == ["profile_000003.txt", "profile_000006.txt", "profile_000009.txt"]
    assert [c for c, _ in stats.profiles] == [3, 6, 9]
    for cycle, P in stats.profiles:
        assert P.cycle == cycle and P.kind == "r" and int(P.n.sum()) == 96 * 96
        same_table(aio.read_profile_file(os.path.join(out, f"profile_{cycle:06d}.txt")), P.table())
    assert stats.data.state_digest() == plain.data.state_digest()      # taking profiles changed nothing
    assert stats.cycles == plain.cycles == 9 and stats.final_time == plain.final_time
    # profile_at_end adds the last one once: not after a cycle the step already covered, and after one it did not
    for step, cycles in ((3, [3, 6, 9]), (4, [4, 8, 9]), (0, [9])):
        d = str(tmp_path / f"end{step}")
        s = armon_amd.armon(armon_amd.ArmonParameters(profile_step=step, profile_at_end=True, profile_kind="x", profile_width=8, output_dir=d, **base))
        assert [c for c, _ in s.profiles] == cycles and len(os.listdir(d)) == len(cycles)
    # a tile group writes the same files
    tiled = str(tmp_path / "tiles")
    group = TileGroup((2, 2), profile_step=3, profile_kind="r", output_dir=tiled, **base)
    try:
        gstats = group.run()
        assert [c for c, _ in gstats.profiles] == [3, 6, 9]
        for (_, a), (_, b) in zip(gstats.profiles, stats.profiles):
            assert a == b
        for name in sorted(os.listdir(out)):
            assert open(os.path.join(tiled, name)).read() == open(os.path.join(out, name)).read(), name
        assert group.state_digest() == plain.data.state_digest()
    finally:
        group.close()
    # graph replay steps aside: the plain loop runs, with the same result
    g = armon_amd.ArmonParameters(return_data=True, graph_cycles=True, profile_step=3, profile_kind="r", output_dir=str(tmp_path / "graph"), **base)
    assert not graph_cycles_usable(g)
    gs = armon_amd.armon(g)
    assert [c for c, _ in gs.profiles] == [3, 6, 9] and gs.data.state_digest() == plain.data.state_digest()
    assert all(a == b for (_, a), (_, b) in zip(gs.profiles, stats.profiles))
