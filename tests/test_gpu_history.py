"""Run history on the device (csrc/history.hip) against the rule in Python (armon_amd/history.py): the record word for word on
random states, tile groups against the single block, the gauges against ``gather``, the asynchronous ring against samples
taken by hand, restart, and what the sums and extrema must satisfy on whole runs."""
import math
import os

import numpy as np
import pytest

from sweep_reference import draw_state

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
# (N, nghost, dtype)
SHAPES = [((130, 3), None, "float64"),      # two spans with a 2-cell tail
          ((258, 3), None, "float32"),      # the same for fp32 (a span is 256 columns)
          ((130, 3), 5, "float64"),         # misaligned rows: the element path
          ((130, 3), 5, "float32"),
          ((1, 1), None, "float64"),        # the degenerate case
          ((1, 1), None, "float32"),
          ((512, 600), None, "float64"),    # more (row, span) items than resident waves: the grid-stride walk
          ((512, 600), None, "float32"),
          ((3, 65540), None, "float64"),    # more rows than a launch grid's y extent
          ((3, 65540), None, "float32")]


def random_block(N, nghost, dtype, test, seed=7):
    """A block holding a random state with u and v of both signs, and the staged EOS kernel's p, c of it → (grid, fields): the
    real cells of rho, u, v, E, p, c in the data type."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test
    kw = {} if nghost is None else dict(nghost=nghost)
    params = armon_amd.ArmonParameters(test=test, N=N, data_type=dtype, silent=5, **kw)
    grid = BlockGrid(params)
    init_test(params, grid)
    f = draw_state(np.random.default_rng(seed), grid.size.n_cells, params.test.eos)
    grid.host_to_device({k: f[k].astype(dtype) for k in STATE})
    return grid, fields_of(grid)


def fields_of(grid):
    from armon_amd.solver import update_EOS
    update_EOS(grid.params, grid)                   # writes p, c, g only: the state the sample reads is untouched
    host = grid.device_to_host(STATE + ("p", "c"))
    return {k: grid.real_view(host[k]).copy() for k in host}


def oracle_record(f, scale_exp, **kw):
    from armon_amd import history as H
    return H.reference_record(f["rho"], f["u"], f["v"], f["E"], f["p"], f["c"], scale_exp=scale_exp, **kw)


def same_words(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} words differ, first word {bad[0]}: {int(got[bad[0]]):#x} != {int(want[bad[0]]):#x}")
    assert not got[36:].any()                       # reserved words stay zero


@pytest.mark.parametrize("test", ["Sod", "Bizarrium"])
@pytest.mark.parametrize("N,nghost,dtype", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_kernel_gives_the_record_of_the_host_rule_word_for_word(N, nghost, dtype, test):
    from armon_amd import history as H
    grid, f = random_block(N, nghost, dtype, test)
    rec, _ = grid.history_sample()
    assert rec.n + rec.n_bad == N[0] * N[1] and rec.n_bad == 0
    assert rec.scale_exp == H.default_scale(oracle_record(f, H.FIRST_SCALE))
    same_words(rec.raw, oracle_record(f, rec.scale_exp), "default scale")
    assert grid.history_sample()[0] == rec          # two calls
    # a coarser scale of the caller's, and one so fine that the larger cells are refused
    coarse = tuple(s + 30 for s in rec.scale_exp)
    same_words(grid.history_sample(scale_exp=coarse)[0].raw, oracle_record(f, coarse), "coarse scale")
    fine = (rec.scale_exp[0] - 18,) + rec.scale_exp[1:]       # the largest rho holds [2^77, 2^78) quanta by default: now 2^95 or more
    got = grid.history_sample(scale_exp=fine)[0]
    same_words(got.raw, oracle_record(f, fine), "fine scale")
    assert got.n_bad > 0 and got.n + got.n_bad == N[0] * N[1]
    # the decoded values are the state's
    rho = f["rho"].astype(np.float64)
    assert rec.rho_max == rho.max() and rec.rho_min == rho.min()
    iy, ix = np.unravel_index(np.argmax(rho), rho.shape)
    assert rec.at["rho_max"] == (ix, iy)
    assert abs(rec.mass - rho.sum() * rec.ds) <= rho.size * 2.0 ** -52 * rec.mass
    u, v = f["u"].astype(np.float64), f["v"].astype(np.float64)
    assert rec.speed_max == math.sqrt((u * u + v * v).max()) and rec.kinetic >= 0 and rec.momentum_x != 0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_nan_an_inf_and_tied_extrema(dtype):
    from armon_amd import history as H
    grid, _ = random_block((70, 9), None, dtype, "Sod")
    host = grid.device_to_host(STATE)
    real = {k: grid.real_view(host[k]) for k in STATE}
    real["rho"][2, 3] = math.nan
    real["E"][4, 5] = math.inf
    real["rho"][7, 66] = real["rho"][1, 40] = 5.0           # two equal maxima: the lower index g = 1 * 70 + 40 wins
    real["rho"][8, 1] = real["rho"][3, 69] = 0.01           # two equal minima: g = 3 * 70 + 69
    for iy, ix in ((0, 69), (6, 0)):                        # two equal speed maxima (E = 20 keeps e = 7.5 and the sound speed real)
        real["u"][iy, ix], real["v"][iy, ix], real["E"][iy, ix] = 3.0, -4.0, 20.0
    grid.host_to_device(host)
    f = fields_of(grid)
    rec, _ = grid.history_sample()
    assert rec.n_bad == 2 and rec.n == 70 * 9 - 2
    same_words(rec.raw, oracle_record(f, rec.scale_exp), "planted cells")
    assert rec.rho_max == 5.0 and rec.at["rho_max"] == (40, 1) and rec.at["rho_min"] == (69, 3)
    assert rec.speed_max == 5.0 and rec.at["speed_max"] == (69, 0)
    # the record of the other cells is untouched by the two bad ones: the oracle with them replaced by good cells of no
    # weight in any extremum differs in the sums of those two cells only
    clean = {k: a.copy() for k, a in f.items()}
    for k in STATE + ("p", "c"):
        clean[k][2, 3], clean[k][4, 5] = f[k][0, 0], f[k][0, 0]
    twice = oracle_record(clean, rec.scale_exp)
    one = oracle_record({k: a[:1, :1] for k, a in f.items()}, rec.scale_exp, global_nx=70)
    sums = rec.raw[2:20].view(np.int64) + 2 * one[2:20].view(np.int64)
    assert np.array_equal(sums, twice[2:20].view(np.int64)) and np.array_equal(rec.raw[20:36], twice[20:36])


def plant_state(dst, src_fields):
    """The real cells of ``src_fields`` into the block ``dst`` (another ghost width: every row lands elsewhere)."""
    host = dst.device_to_host(STATE)
    for k in STATE:
        dst.real_view(host[k])[...] = src_fields[k]
    dst.host_to_device(host)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_another_ghost_width_and_windows_give_the_same_record(dtype):
    import armon_amd
    from armon_amd import history as H
    from armon_amd.solver import BlockGrid, init_test
    grid, f = random_block((130, 7), None, dtype, "Sod")
    rec, _ = grid.history_sample()
    for g in (5, 6):
        params = armon_amd.ArmonParameters(test="Sod", N=(130, 7), data_type=dtype, nghost=g, silent=5)
        other = BlockGrid(params)
        init_test(params, other)
        plant_state(other, f)
        same_words(other.history_sample(scale_exp=rec.scale_exp)[0].raw, rec.raw, f"nghost = {g}")
    # the windows of one block, through the C ABI: split at an odd column and at a row
    import ctypes as C
    p, dev = grid.params, grid.params.device
    s = H.Sampler([(p, grid)], capacity=4, scale_exp=rec.scale_exp)
    try:
        windows = [(0, 0, 67, 7), (67, 0, 63, 7), (0, 0, 130, 2), (0, 2, 130, 5)]
        for slot, (c0, r0, wx, wy) in enumerate(windows):
            assert p.fn("history_sample")(dev.ctx, s.handles[0], slot, C.byref(s.spec), grid.size.size[0], grid.size.ghosts, 130, 7,
                                          *[C.c_void_p(grid.data[k].ptr) for k in STATE], c0, r0, wx, wy, c0, r0) == 0
        raw, _ = s.read(0, 4)
        same_words(H.merge_raw(raw[0], raw[1]), rec.raw, "two column windows")
        same_words(H.merge_raw(raw[3], raw[2]), rec.raw, "two row windows")
        same_words(raw[1], oracle_record({k: a[:, 67:] for k, a in f.items()}, rec.scale_exp, origin=(67, 0), global_nx=130), "right window")
        # what the library refuses: a slot outside the ring, a window outside the block, a gauge outside the window
        L = dev._L
        args = [C.byref(s.spec), grid.size.size[0], grid.size.ghosts, 130, 7, *[C.c_void_p(grid.data[k].ptr) for k in STATE]]
        assert p.fn("history_sample")(dev.ctx, s.handles[0], 4, *args, 0, 0, 130, 7, 0, 0) == 1 and b"slot" in L.armon_hip_last_error()
        assert p.fn("history_sample")(dev.ctx, s.handles[0], -1, *args, 0, 0, 130, 7, 0, 0) == 1
        assert p.fn("history_sample")(dev.ctx, s.handles[0], 0, *args, 1, 0, 130, 7, 0, 0) == 1
        assert L.armon_hip_history_set_gauges(dev.ctx, s.handles[0], (C.c_int64 * 1)(5), 1) == 1          # the handle holds no gauge
        rec_buf = np.empty((5, H.WORDS), dtype=np.uint64)
        assert L.armon_hip_history_read(dev.ctx, s.handles[0], 2, 3, rec_buf.ctypes.data_as(C.c_void_p), None) == 1
        h = C.c_void_p()
        assert L.armon_hip_history_create(dev.ctx, 0, 0, C.byref(h)) == 1 and L.armon_hip_history_create(dev.ctx, 4, 65, C.byref(h)) == 1
    finally:
        s.close()
    g1 = H.Sampler([(p, grid)], capacity=1, gauges=[(0.5, 0.5)], scale_exp=rec.scale_exp)
    try:
        cell = (C.c_int64 * 1)(130 * 7)
        assert dev._L.armon_hip_history_set_gauges(dev.ctx, g1.handles[0], cell, 1) == 0
        with pytest.raises(armon_amd.SolverException):
            g1.enqueue(0)                                   # the cell lies outside the window: refused before any launch
    finally:
        g1.close()


@pytest.mark.parametrize("nghost", [4, 6])
def test_tile_groups_give_the_single_block_record_and_gauges(nghost):
    """Exact arithmetic: the tiles hold the single block's bits (asserted), so the merged record must be the single block's,
    word for word. Gauges on the first and on the last real cell of a tile, of the domain, and inside a tile: bit-equal to the
    cell's values, p being the EOS of the cell."""
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    N = (50, 38)
    kw = dict(test="Sedov", N=N, maxcycle=6, silent=5, exact_arithmetic=True, nghost=nghost)
    ref = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **kw)).data
    single = fields_of(ref)
    dx, dy = 2.0 / N[0], 2.0 / N[1]
    cells = [(0, 0), (49, 37), (24, 18), (25, 19), (12, 12), (25, 0), (24, 37), (37, 9), (16, 12), (17, 13)]    # tile corners of (2,2), (4,2), (1,3)
    gauges = [(-1.0 + (gx + 0.5) * dx, -1.0 + (gy + 0.5) * dy) for gx, gy in cells]
    want, want_g = ref.history_sample(gauges=gauges)
    same_words(want.raw, oracle_record(single, want.scale_exp), "single block")
    for i, (gx, gy) in enumerate(cells):
        for j, k in enumerate(STATE + ("p",)):
            assert want_g[i, j] == np.float64(single[k][gy, gx]), (i, k)
    # gather of the cell on the device gives the same bits
    g, pitch = ref.size.ghosts, ref.size.size[0]
    for i, (gx, gy) in enumerate(cells[:3]):
        got = ref.gather(STATE, (g + gy) * pitch + g + gx, 1, 1)
        assert [float(got[k][0]) for k in STATE] == list(want_g[i, :4])
    for P in ((2, 2), (1, 3), (4, 2)):
        group = TileGroup(P, **kw)
        try:
            group.run()
            tiles = group.gather(STATE)
            for k in STATE:
                assert np.array_equal(tiles[k], single[k]), (P, k)      # the premise
            got, got_g = group.history_sample(gauges=gauges)
            assert got.scale_exp == want.scale_exp
            same_words(got.raw, want.raw, P)
            assert got == want and np.array_equal(got_g.view(np.uint64), want_g.view(np.uint64)), P
        finally:
            group.close()


def run_sod(tmp, name, **kw):
    import armon_amd
    # (maxtime: the default of 0.2 ends this grid's run after 28 cycles; the cycle count is to decide)
    opts = dict(test="Sod", N=(64, 16), maxcycle=40, maxtime=10.0, silent=5, return_data=True, output_dir=str(tmp / name))
    opts.update(kw)
    return armon_amd.armon(armon_amd.ArmonParameters(**opts))


GAUGES = [(0.25, 0.5), (0.51, 0.03), (1.0, 1.0)]


def test_asynchrony_changes_nothing(tmp_path):
    """40 cycles sampled every cycle through a ring of 8 slots — five flushes, every slot reused — against the same run sampled
    by hand, synchronously, after every cycle; and against the run with no history at all."""
    import armon_amd
    from armon_amd import history as H
    from armon_amd import io as aio
    from armon_amd.solver import BlockGrid, cycle_ends, init_test, solver_cycle
    stats = run_sod(tmp_path, "ring", history_step=1, history_capacity=8, history_gauges=GAUGES)
    hist = stats.history
    assert stats.cycles == 40 and hist.cycle == list(range(41)) and hist.dt[0] == 0.0 and all(d > 0 for d in hist.dt[1:])
    assert hist.time[-1] == stats.final_time and int(hist.n_bad.sum()) == 0 and hist.gauge_cells == ((16, 8), (32, 0), (63, 15))
    assert np.array_equal(np.cumsum(np.array(hist.dt)), np.array(hist.time))        # (the clock adds the steps in this order)
    plain = run_sod(tmp_path, "plain")
    assert stats.data.state_digest() == plain.data.state_digest() and plain.history is None
    assert (stats.final_time, stats.last_dt) == (plain.final_time, plain.last_dt)
    # by hand
    params = armon_amd.ArmonParameters(test="Sod", N=(64, 16), maxcycle=40, maxtime=10.0, silent=5)
    grid = BlockGrid(params)
    init_test(params, grid)
    gdt = grid.global_dt
    by_hand = H.History(*hist._meta())
    rec, gv = grid.history_sample(gauges=GAUGES, scale_exp=hist.scale_exp)
    by_hand.append(0, 0.0, 0.0, rec.raw, gv)
    while gdt.cycle < 40:
        solver_cycle(params, grid, last_cycle=cycle_ends(params, gdt))
        dt = float(gdt.current_dt)
        gdt.next_cycle()
        rec, gv = grid.history_sample(gauges=GAUGES, scale_exp=hist.scale_exp)
        by_hand.append(gdt.cycle, float(gdt.time), dt, rec.raw, gv)
    assert by_hand == hist
    assert H.default_scale(hist.raw[0]) == hist.scale_exp               # the scale came from the initial state
    # the file holds the same rows
    t = aio.read_history_file(os.path.join(str(tmp_path / "ring"), "history.txt"))
    want = hist.table()
    assert set(t) == set(want) and all(np.array_equal(t[k], want[k]) for k in t)
    # a coarser step: the initial row, every third cycle, and the cycle the run stopped at
    third = run_sod(tmp_path, "third", history_step=3, history_capacity=8, history_gauges=GAUGES).history
    assert third.cycle == list(range(0, 40, 3)) + [40]
    rows = [hist.cycle.index(c) for c in third.cycle]
    assert np.array_equal(third.raw, hist.raw[rows]) and np.array_equal(third.gauge_values, hist.gauge_values[rows])
    assert third.dt[1] == hist.dt[3] and third.time == [hist.time[r] for r in rows]


def test_a_restart_continues_the_file(tmp_path):
    import armon_amd
    whole = run_sod(tmp_path, "run", maxcycle=30, history_step=1, history_capacity=8, history_gauges=GAUGES, checkpoint_step=15)
    path = os.path.join(str(tmp_path / "run"), "history.txt")
    text = open(path).read()
    ckpt = os.path.join(str(tmp_path / "run"), "checkpoint_000015.ckpt")
    again = run_sod(tmp_path, "run", maxcycle=30, history_step=1, history_capacity=8, history_gauges=GAUGES, restart_from=ckpt)
    assert open(path).read() == text
    assert again.history.cycle == list(range(16, 31)) and again.history.scale_exp == whole.history.scale_exp
    assert np.array_equal(again.history.raw, whole.history.raw[16:]) and again.data.state_digest() == whole.data.state_digest()
    with pytest.raises(armon_amd.SolverException) as e:
        run_sod(tmp_path, "run", maxcycle=30, history_step=1, history_gauges=GAUGES[:2], restart_from=ckpt)
    assert e.value.category == "config" and "gauge2" in e.value.msg
    assert open(path).read() == text                        # a refused restart leaves the file alone


@pytest.mark.parametrize("test", ["Sod", "Sedov", "Bizarrium"])
def test_whole_runs_conserve_and_refuse_no_cell(test, tmp_path):
    """100 x 100 over the golden run length with the default scale: no bad cell in any row; kinetic >= 0; the mass is
    conservation_vars' within n_cells 2^-52 relative (the worst case of the floating-point sum it is compared with). Sod moves
    along x only: momentum_y is exactly 0 in every row."""
    import armon_amd
    from armon_amd.solver import conservation_vars
    params = armon_amd.ArmonParameters(test=test, N=(100, 100), maxcycle=1000, silent=5, return_data=True, history_step=1,
                                       output_dir=str(tmp_path))
    stats = armon_amd.armon(params)
    hist = stats.history
    assert len(hist) == stats.cycles + 1 and int(hist.n_bad.sum()) == 0 and (hist.n == 100 * 100).all()
    assert (hist.kinetic >= 0).all() and (test == "Bizarrium" or hist.kinetic[0] == 0.0)
    assert all(abs(a - (b - c)) <= 2.0 ** -50 * abs(b) for a, b, c in zip(hist.internal, hist.energy, hist.kinetic))
    mass, energy = conservation_vars(params, stats.data)
    assert abs(hist.mass[-1] - mass) <= 100 * 100 * 2.0 ** -52 * mass
    assert abs(hist.energy[-1] - energy) <= 2 * 100 * 100 * 2.0 ** -52 * abs(energy)      # (rho E: one more rounding per addend)
    if test == "Sod":
        assert (hist.momentum_y == 0).all() and (hist.momentum_x[1:] > 0).all()
        assert np.abs(hist.mass - hist.mass[0]).max() <= 1e-12 and (hist.mach_max[1:] > 0).all()
    if test == "Sedov":
        assert hist.records[0].at["e_max"] in ((49, 49), (50, 50), (49, 50), (50, 49))     # the blast sits at the centre
