"""Exact solutions on the GPU: armon_hip_exact_norms / armon_hip_exact_fill and the Python surface over them
(BlockGrid.error_norms / fill_exact, TileGroup's, the error_norms_* and start_from_exact options).

The oracle is analytic.reference_record / analytic.stored_reference: the rule of include/armon_hip.h restated in numpy. Records
are compared WORD FOR WORD and filled states bit for bit, never within a tolerance: every addend is rounded once to an integer
and integer sums have no order."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
DTYPES = ["float64", "float32"]
# (N, nghost): unaligned rows and a partial span; aligned; more rows than a launch grid's y extent
SHAPES = [((131, 37), 4), ((131, 37), 5), ((256, 16), 4), ((8, 70000), 4)]

# |L1(tuned) - L1(exact)| / L1(exact), the largest over rho, un, p: Sod 400 x 8 to t = 0.2, fp64, measured once on an MI355X
# (DESIGN §4.7), and |L1(GPU fp32) - L1(fp32 oracle)| / L1(fp32 oracle) of the same run in fp32. The arithmetic is the same from
# run to run, so the tenfold margin covers no noise: it is there so that a change of the tuned flavour which moves the
# physics is seen.
TUNED_VS_EXACT_MEASURED = 4.774e-14
FP32_VS_ORACLE_MEASURED = 2.710e-4
MARGIN = 10.0


def grid_with_random_state(N, nghost, dtype, seed, test="Sod"):
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test
    params = armon_amd.ArmonParameters(test=test, N=N, nghost=nghost, data_type=dtype, silent=5)
    grid = BlockGrid(params)
    init_test(params, grid)
    rng = np.random.default_rng(seed)
    host = grid.device_to_host(STATE)
    for k, (lo, hi) in zip(STATE, ((0.1, 2.0), (-1.0, 1.0), (-1.0, 1.0), (1.5, 3.0))):
        grid.real_view(host[k])[...] = rng.uniform(lo, hi, (N[1], N[0])).astype(dtype)
    grid.host_to_device(host)
    return grid


def real_fields(grid):
    host = grid.device_to_host(STATE)
    return [grid.real_view(host[k]).copy() for k in STATE]


def solutions(params, seed=11):
    """RIEMANN-X, RIEMANN-Y, TABLE-R (the point blast, off the grid's centre) and TABLE-X with a random table."""
    from armon_amd import analytic as an
    rng = np.random.default_rng(seed)
    r = an.riemann_exact((1.0, 0.0, 1.0), (0.125, 0.0, 0.1), 1.4)
    sim = an.sedov_similarity(1.4, 2, 400)
    M = 37
    return {
        "riemann-x": an.ExactSolution(an.RIEMANN, "x", (0.5, 0.0), 1.4, time=0.17, riemann=r),
        "riemann-y": an.ExactSolution(an.RIEMANN, "y", (0.0, 0.4371), 1.4, time=0.12, riemann=r),
        "table-r": an.ExactSolution.table("r", 0.45, sim.g, 0.8 * sim.v, 0.64 * sim.pi, (1.0, 0.0, 1e-3), centre=(0.3713, 0.6291)),
        "table-x": an.ExactSolution.table("x", 0.8, rng.uniform(0.5, 2.0, M + 1), rng.uniform(-1.0, 1.0, M + 1), rng.uniform(0.2, 1.5, M + 1),
                                          (0.7, -0.3, 0.9), centre=(0.1, 0.0)),
    }


def same_words(got, want, what):
    got = got.raw if hasattr(got, "raw") else got
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k, w = bad[0]
        raise AssertionError(f"{what}: {len(bad)} words differ, first in variable {k} word {w}: {int(got[k, w]):#x} != {int(want[k, w]):#x}")
    assert not got[:, 13:].any()                                       # reserved words stay zero


def host_record(grid, solution, samples=1, coord_range=None, window=None, fields=None):
    from armon_amd import analytic as an
    s = an.spec_of(grid.params, solution, samples, coord_range)
    f = real_fields(grid) if fields is None else fields
    if window is None:
        return an.reference_record(s, *f)
    c0, r0, wx, wy = window
    return an.reference_record(s, *[a[r0:r0 + wy, c0:c0 + wx] for a in f], origin=(c0, r0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,nghost", SHAPES)
def test_records_and_fills_equal_the_host_rule(N, nghost, dtype):
    from armon_amd import analytic as an
    grid = grid_with_random_state(N, nghost, dtype, seed=N[0] + nghost)
    f = real_fields(grid)
    long_block = N[1] > 65535
    asks = [(name, samples) for name in ("riemann-x", "riemann-y", "table-r", "table-x") for samples in (1, 2)]
    if long_block:                                                     # the walk over the rows is what this shape is about
        asks = [("riemann-y", 1), ("table-r", 2), ("riemann-x", 1), ("table-x", 1)]
    sols = solutions(grid.params)
    gx, gy = np.arange(N[0])[None, :], np.arange(N[1])[:, None]
    for name, samples in asks:
        norms = grid.error_norms(sols[name], samples=samples)
        same_words(norms, host_record(grid, sols[name], samples, fields=f), (name, samples))
        assert norms.n == N[0] * N[1] and norms.n_bad == 0 and norms.rho.l1 > 0
    for name, samples in asks:                                         # (the state is overwritten from here on)
        grid.fill_exact(sols[name], samples=samples)
        want, keep = an.stored_reference(an.spec_of(grid.params, sols[name], samples), gx, gy, np.dtype(dtype))
        assert keep.all()
        for k, got, w in zip(STATE, real_fields(grid), want):
            assert got.tobytes() == w.tobytes(), (name, samples, k, int((got != w).sum()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_windows_ranges_and_bad_cells(dtype):
    grid = grid_with_random_state((131, 37), 4, dtype, seed=5)
    sols = solutions(grid.params)
    f = real_fields(grid)
    for name in ("riemann-x", "table-r"):
        whole = grid.error_norms(sols[name])
        # a strict sub-rectangle that starts off the 16-B grid, and windows that tile the block
        window = (3, 2, 100, 30)
        same_words(grid.error_norms(sols[name], window=window), host_record(grid, sols[name], window=window, fields=f), (name, window))
        parts = None
        for w in ((0, 0, 61, 37), (61, 0, 70, 11), (61, 11, 70, 26)):
            part = grid.error_norms(sols[name], window=w)
            parts = part if parts is None else parts.merge(part)
        same_words(parts, whole.raw, (name, "windows"))
        # a coordinate range that skips cells: they are counted nowhere
        rng = (-0.2, 0.1) if name == "riemann-x" else (0.05, 0.3)
        cut = grid.error_norms(sols[name], coord_range=rng)
        same_words(cut, host_record(grid, sols[name], coord_range=rng, fields=f), (name, rng))
        assert 0 < cut.n < whole.n and cut.n_bad == 0
    # one NaN and one infinity go to n_bad only
    host = grid.device_to_host(STATE)
    grid.real_view(host["rho"])[3, 10], grid.real_view(host["E"])[17, 41] = math.nan, math.inf
    grid.host_to_device(host)
    from armon_amd import analytic as an
    for name in ("riemann-x", "table-r"):
        norms = grid.error_norms(sols[name], samples=2)
        assert norms.n_bad == 2 and norms.n == 131 * 37 - 2
        same_words(norms, host_record(grid, sols[name], 2), (name, "bad"))
        skip = np.zeros((37, 131), dtype=bool)
        skip[3, 10] = skip[17, 41] = True
        clean = an.reference_record(an.spec_of(grid.params, sols[name], 2), *real_fields(grid), skip=skip)
        assert np.array_equal(norms.raw[:, 2:], clean[:, 2:]) and not clean[:, 1].any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_filled_state_is_at_distance_zero(dtype):
    grid = grid_with_random_state((131, 37), 5, dtype, seed=9)
    sols = solutions(grid.params)
    for name in ("riemann-x", "riemann-y", "table-r", "table-x"):
        for samples in (1, 2):
            grid.fill_exact(sols[name], samples=samples)
            norms = grid.error_norms(sols[name], samples=samples)
            assert norms.n == 131 * 37 and norms.n_bad == 0, (name, samples)
            assert not norms.raw[:, 2:12].any() and np.all(norms.raw[:, 12] == np.uint64(2 ** 64 - 1)), (name, samples)
            for var in ("rho", "un", "ut", "p"):
                v = getattr(norms, var)
                assert v.l1 == 0.0 and v.l2 == 0.0 and v.linf == 0.0 and v.bias == 0.0 and v.linf_at is None
    # a window only: the cells outside keep their values, the window is at distance 0
    before = real_fields(grid)
    window = (7, 3, 50, 20)
    grid.fill_exact(sols["table-x"], window=window)
    after = real_fields(grid)
    mask = np.zeros((37, 131), dtype=bool)
    mask[3:23, 7:57] = True
    for a, b in zip(before, after):
        assert np.array_equal(a[~mask], b[~mask])
    z = grid.error_norms(sols["table-x"], window=window)
    assert z.n == 1000 and not z.raw[:, 2:12].any()


@pytest.mark.parametrize("test", ["Sod_y", "Sedov"])
def test_tile_groups_give_the_single_block_record(test):
    """Exact arithmetic: the tiles hold the single block's bits (asserted), so the merged record is the single block's."""
    import armon_amd
    from armon_amd import analytic as an
    from armon_amd.multi_tile import TileGroup
    kw = dict(test=test, N=(150, 90), maxcycle=5, silent=5, exact_arithmetic=True)
    stats = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **kw))
    ref, t = stats.data, stats.final_time
    single = real_fields(ref)
    want = [ref.error_norms(time=t, samples=samples) for samples in (1, 2)]
    same_words(want[0], host_record(ref, an.reference_for(ref.params, t), fields=single), test)
    assert want[0].n == 150 * 90 and want[0].rho.l1 > 0
    for P in ((2, 2), (3, 1)):
        group = TileGroup(P, **kw)
        try:
            group.run()
            tiles = group.gather(STATE)
            for k, a in zip(STATE, single):
                assert np.array_equal(tiles[k], a), (P, k)             # the premise
            for samples, w in zip((1, 2), want):
                got = group.error_norms(time=t, samples=samples)
                assert got.scale_exp == w.scale_exp
                same_words(got, w.raw, (P, samples))
            # a window of the global grid that cuts through the tiles: each tile takes its part
            window = (40, 20, 75, 50)
            same_words(group.error_norms(time=t, window=window), ref.error_norms(time=t, window=window).raw, (P, window))
            # a filled group is at distance 0, and holds what the filled block holds
            group.fill_exact(time=t)
            assert not group.error_norms(time=t).raw[:, 2:12].any()
        finally:
            group.close()
    ref.fill_exact(time=t)
    assert not ref.error_norms(time=t).raw[:, 2:12].any()


def oracle_record(oracle, params, fields, time):
    from armon_amd import analytic as an
    nx, ny = params.N
    s = an.spec_of(params, an.reference_for(params, time))
    return an.reference_record(s, *[oracle.real_view(fields[k], nx, ny, params.nghost) for k in STATE])


@pytest.mark.parametrize("test,N,maxtime", [("Sod", (400, 8), 0.0), ("Sedov", (128, 128), 0.3)])
def test_end_to_end_against_the_oracle(oracle, tmp_path, test, N, maxtime):
    """The exact flavour computes the oracle's bits, so the norms of the run are the norms of the oracle's state, word for word."""
    import armon_amd
    from armon_amd import io as aio
    kw = dict(maxtime=maxtime) if maxtime else {}
    params = armon_amd.ArmonParameters(test=test, N=N, exact_arithmetic=True, error_norms_at_end=True, silent=5, output_dir=str(tmp_path), **kw)
    stats = armon_amd.armon(params)
    run, f = oracle.solve(test=test, N=N, **kw)
    assert stats.cycles == run.cycles and stats.final_time == run.final_time
    assert len(stats.error_norms) == 1
    cycle, time, norms = stats.error_norms[0]
    assert cycle == stats.cycles and time == stats.final_time and norms.cycle == cycle and norms.time == time
    same_words(norms, oracle_record(oracle, params, f, time), test)
    assert norms.n == N[0] * N[1] and norms.n_bad == 0
    print(norms.report())
    path = os.path.join(str(tmp_path), f"error_norms_{cycle:06d}.txt")
    assert os.listdir(str(tmp_path)) == [os.path.basename(path)]
    assert aio.read_error_norms_file(path) == norms.table()


def test_the_step_option_and_a_tile_group_write_the_same_files(tmp_path):
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    base = dict(test="Sod", N=(96, 16), maxcycle=9, silent=5, exact_arithmetic=True)
    plain = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **base))
    out = str(tmp_path / "single")
    stats = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, error_norms_step=4, error_norms_at_end=True, error_norms_samples=2,
                                                      output_dir=out, **base))
    assert sorted(os.listdir(out)) == ["error_norms_000004.txt", "error_norms_000008.txt", "error_norms_000009.txt"]
    assert [c for c, _, _ in stats.error_norms] == [4, 8, 9] and all(n.samples == 2 for _, _, n in stats.error_norms)
    assert stats.data.state_digest() == plain.data.state_digest() and stats.final_time == plain.final_time      # nothing else changed
    tiled = str(tmp_path / "tiles")
    group = TileGroup((2, 1), error_norms_step=4, error_norms_at_end=True, error_norms_samples=2, output_dir=tiled, **base)
    try:
        gstats = group.run()
        assert [c for c, _, _ in gstats.error_norms] == [4, 8, 9]
        for (_, _, a), (_, _, b) in zip(gstats.error_norms, stats.error_norms):
            assert a == b
        for name in sorted(os.listdir(out)):
            assert open(os.path.join(tiled, name)).read() == open(os.path.join(out, name)).read(), name
    finally:
        group.close()


def relative_l1_difference(a, b):
    return max(abs(getattr(a, v).l1 - getattr(b, v).l1) / getattr(b, v).l1 for v in ("rho", "un", "p"))


def test_the_tuned_arithmetic_stays_close_to_the_exact_one(tmp_path):
    import armon_amd
    kw = dict(test="Sod", N=(400, 8), error_norms_at_end=True, silent=5, output_dir=str(tmp_path))
    exact = armon_amd.armon(armon_amd.ArmonParameters(exact_arithmetic=True, **kw)).error_norms[0][2]
    tuned = armon_amd.armon(armon_amd.ArmonParameters(**kw)).error_norms[0][2]
    rel = relative_l1_difference(tuned, exact)
    print(f"tuned against exact arithmetic, Sod 400 x 8: relative difference of L1 = {rel:.3e}; L1(rho) = {tuned.rho.l1:.6e} / {exact.rho.l1:.6e}")
    assert not np.array_equal(tuned.raw, exact.raw)                    # another arithmetic: other norms
    assert rel <= MARGIN * TUNED_VS_EXACT_MEASURED


def test_fp32_stays_close_to_the_fp32_oracle(oracle, tmp_path):
    import armon_amd
    params = armon_amd.ArmonParameters(test="Sod", N=(400, 8), data_type="float32", error_norms_at_end=True, silent=5, output_dir=str(tmp_path))
    stats = armon_amd.armon(params)
    norms = stats.error_norms[0][2]
    from armon_amd import analytic as an
    run, f = oracle.solve(test="Sod", N=(400, 8), data_type=np.float32)
    want = an.ErrorNorms(oracle_record(oracle, params, f, float(run.final_time)), norms.scale_exp, 400)
    rel = relative_l1_difference(norms, want)
    print(f"fp32 GPU against the fp32 oracle, Sod 400 x 8: relative difference of L1 = {rel:.3e}; cycles {stats.cycles} / {run.cycles}; "
          f"L1(rho) = {norms.rho.l1:.6e} / {want.rho.l1:.6e}")
    assert norms.n == 3200 and norms.n_bad == 0
    assert rel <= MARGIN * FP32_VS_ORACLE_MEASURED


def test_start_from_exact(oracle, tmp_path):
    """Sod 200 x 8 started from the exact solution at t0 = 0.05 reaches maxtime with an L1(rho) not larger than the run started
    from the jump; the CPU oracle, started from the same filled state, says the same (checked first)."""
    import armon_amd
    from armon_amd import analytic as an
    N, t0 = (200, 8), 0.05
    params = armon_amd.ArmonParameters(test="Sod", N=N, silent=5)

    def l1_of(fields, time):
        return an.ErrorNorms(oracle_record(oracle, params, fields, time), an.reference_for(params, time).default_scale(), N[0]).rho.l1
    run, f = oracle.solve(test="Sod", N=N)
    from_jump = l1_of(f, float(run.final_time))
    _, g = oracle.solve(test="Sod", N=N, maxcycle=0)
    filled, _ = an.stored_reference(an.spec_of(params, an.reference_for(params, t0)), np.arange(N[0])[None, :], np.arange(N[1])[:, None])
    for k, a in zip(STATE, filled):
        oracle.real_view(g[k], N[0], N[1], 4)[...] = a
    run1, g = oracle.solve(test="Sod", N=N, fields=g, skip_init=True, maxtime=0.2 - t0)
    from_exact = l1_of(g, float(run1.final_time) + t0)
    print(f"oracle: L1(rho) = {from_jump:.4e} from the jump, {from_exact:.4e} from the exact state at t0 = {t0}")
    assert from_exact <= from_jump
    # the run starts at t0 with the filled state
    kw = dict(test="Sod", N=N, silent=5, exact_arithmetic=True, return_data=True, output_dir=str(tmp_path))
    start = armon_amd.armon(armon_amd.ArmonParameters(start_from_exact=t0, maxcycle=0, **kw))
    assert start.cycles == 0 and start.final_time == t0
    for got, want in zip(real_fields(start.data), filled):
        assert got.tobytes() == want.tobytes()
    a = armon_amd.armon(armon_amd.ArmonParameters(error_norms_at_end=True, **kw))
    b = armon_amd.armon(armon_amd.ArmonParameters(error_norms_at_end=True, start_from_exact=t0, **kw))
    la, lb = a.error_norms[0][2].rho.l1, b.error_norms[0][2].rho.l1
    print(f"GPU: L1(rho) = {la:.4e} from the jump ({a.cycles} cycles), {lb:.4e} from the exact state ({b.cycles} cycles, t = {b.final_time})")
    assert la == from_jump and b.final_time >= 0.2 and b.cycles < a.cycles
    assert lb <= la


def test_a_tile_group_started_from_the_exact_state_runs_like_the_single_block(tmp_path):
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    kw = dict(test="Sod_y", N=(64, 96), maxcycle=7, silent=5, exact_arithmetic=True, start_from_exact=0.04, error_norms_at_end=True)
    single = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, output_dir=str(tmp_path / "single"), **kw))
    group = TileGroup((1, 3), output_dir=str(tmp_path / "tiles"), **kw)
    try:
        stats = group.run()
        assert stats.cycles == single.cycles == 7 and stats.final_time == single.final_time > 0.04
        assert group.state_digest() == single.data.state_digest()
        assert stats.error_norms[0][2] == single.error_norms[0][2] and stats.error_norms[0][2].n == 64 * 96
    finally:
        group.close()


def test_a_run_past_the_solutions_validity_keeps_its_stats(tmp_path):
    """Sedov to its default maxtime of 1.0: R(1.0) = 1.02 has left the domain, so the hook at the end has no solution to compare
    with. The run completes, the cycle is listed without norms and no file is written for it."""
    import armon_amd
    stats = armon_amd.armon(armon_amd.ArmonParameters(test="Sedov", N=(32, 32), silent=5, error_norms_step=40, error_norms_at_end=True,
                                                      output_dir=str(tmp_path)))
    assert stats.final_time >= 1.0 and stats.error_norms[-1][0] == stats.cycles and stats.error_norms[-1][2] is None
    taken = [(c, n) for c, _, n in stats.error_norms if n is not None]
    assert taken and taken[0][0] == 40 and taken[0][1].n == 32 * 32
    assert sorted(os.listdir(str(tmp_path))) == [f"error_norms_{c:06d}.txt" for c, _ in taken]
