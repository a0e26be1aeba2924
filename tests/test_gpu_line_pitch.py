"""armon_hip_sweep_pair — the X and the Y sweep of a Sequential cycle with the state between them in rows of whole 128-B lines
(the Y march then loads its rows non-temporally) — against the same cycles run as two plain armon_hip_sweep calls on the
standard layout: after 3 cycles the four state arrays are equal bit for bit over the WHOLE caller's arrays, ghosts included, p
is equal, and so is every CFL step on the way. The intermediate vectors of the pair are filled with NaNs beforehand, padding
included: nothing of it may reach a result, and the padding is still NaN afterwards.

Shapes, the smallest at which each path can go wrong: 64 x 40 (pitch 72: odd rows half a line off, the headline shape's case),
56 x 40 (pitch 64: whole lines already, the intermediate's pitch is the block's), 61 x 37 (odd pitch: the Y march's store
exchange runs on the output while its input is line-aligned; the X sweep reads rows of every phase), 300 x 1100 with 64-row
runs (several workgroups per row, the shifted last one included, 18 runs per column)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CYCLES = 3
STATE = ("rho", "u", "v", "E")
SHAPES = [(64, 40, 0), (56, 40, 0), (61, 37, 0), (300, 1100, 64)]                 # nx, ny, ARMON_Y_SEG
FLAVOURS = {                                                                       # test case, exact arithmetic, ghosts
    "Sod": ("Sod", False, 4), "Sod_circ": ("Sod_circ", False, 4), "Sedov": ("Sedov", False, 4),
    "Sod-exact": ("Sod", True, 4), "Bizarrium": ("Bizarrium", False, 4), "Sod-g5": ("Sod", False, 5),
}


@pytest.fixture(scope="module")
def dev():
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.wait()
    d.close()


def _bits(a):
    return a.view(np.uint64)


def _whole(dev, vec):
    """The whole allocation of a vector, padding included."""
    out = np.empty(vec.capacity_bytes // 8)
    assert dev._L.armon_hip_memcpy(dev.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(vec.ptr), vec.capacity_bytes, 2) == 0
    return out


def _fill_whole(dev, vec, value):
    host = np.full(vec.capacity_bytes // 8, value)
    assert dev._L.armon_hip_memcpy(dev.ctx, C.c_void_p(vec.ptr), host.ctypes.data_as(C.c_void_p), vec.capacity_bytes, 1) == 0


def _run(dev, test, exact, g, nx, ny, pair):
    """CYCLES cycles from the test case's initial state → (state arrays + p on the host, the CFL steps, the grid)."""
    import armon_amd
    from armon_amd.blocking import Axis
    from armon_amd.solver import BlockGrid, init_test, sweep_desc
    # (placement_min_bytes = 0: the solver keeps blocks too small to be placed on the plain layout, vectors without padding)
    params = armon_amd.ArmonParameters(test=test, N=(nx, ny), nghost=g, silent=5, exact_arithmetic=exact, ctx=dev.ctx,
                                       placement_min_bytes=0)
    grid = BlockGrid(params)
    init_test(params, grid, tune=False)
    for f in STATE:
        _fill_whole(dev, grid.alt[f], np.nan)
    grid.data["p"].copy_from_host(np.full(grid.data["p"].n, np.nan))
    dx, dy = params.cell_size(0), params.cell_size(1)
    # the first step is far below any CFL bound (Bizarrium's sound speed is thousands of m/s, Sedov's centre is hot); the next
    # ones are half the CFL step the previous cycle's Y sweep has just reduced
    dt, dts = 1e-7 * min(dx, dy), []
    L = dev._L
    for cycle in range(CYCLES):
        d_x = sweep_desc(params, grid, Axis.X, dt, dx)
        grid.swap_state()
        d_y = sweep_desc(params, grid, Axis.Y, dt, dy, emit_p=cycle == CYCLES - 1, emit_dt=True)
        grid.swap_state()
        if pair:
            rc = L.armon_hip_sweep_pair(dev.ctx, C.byref(d_x), C.byref(d_y), grid.alt["rho"].capacity_bytes)
            assert rc == 0, L.armon_hip_last_error()
        else:
            for d in (d_x, d_y):
                assert L.armon_hip_sweep(dev.ctx, C.byref(d)) == 0, L.armon_hip_last_error()
        dev.wait()
        dts.append(float(grid.dt_scalar.to_host()[0]))
        dt = 0.5 * dts[-1]
    return {f: grid.data[f].to_host() for f in STATE + ("p",)}, dts, grid


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("nx,ny,seg", SHAPES, ids=[f"{s[0]}x{s[1]}" for s in SHAPES])
def test_pair_gives_the_bits_of_two_plain_sweeps(dev, nx, ny, seg, flavour):
    from armon_amd.blocking import line_pitch
    test, exact, g = FLAVOURS[flavour]
    assert dev._L.armon_hip_set_tuning(dev.ctx, b"ARMON_Y_SEG", seg) == 0
    try:
        want, want_dts, _ = _run(dev, test, exact, g, nx, ny, pair=False)
        got, got_dts, grid = _run(dev, test, exact, g, nx, ny, pair=True)
        if seg:
            assert dev.y_run_rows() == seg and ny > 2 * seg and nx + g % 16 > 256      # several runs, several workgroups per row
    finally:
        assert dev._L.armon_hip_set_tuning(dev.ctx, b"ARMON_Y_SEG", 0) == 0
    assert all(np.isfinite(want_dts)) and want_dts[0] > 0
    assert got_dts == want_dts, (got_dts, want_dts)
    pitch, rows = nx + 2 * g, ny + 2 * g
    for f in STATE + ("p",):
        assert want[f].size == pitch * rows
        bad = np.flatnonzero(_bits(got[f]) != _bits(want[f]))
        assert bad.size == 0, (f"{f}: {bad.size} elements of the caller's array differ, first at flat index {bad[0]} "
                               f"(row {bad[0] // pitch}, column {bad[0] % pitch}): {got[f][bad[0]]!r} != {want[f][bad[0]]!r}")
        real = want[f].reshape(rows, pitch)[g:g + ny, g:g + nx]
        assert np.isfinite(real).all(), f"{f}: the reference run itself is not finite"
    # the intermediate: real cells written at the line pitch, everything else — ghosts and padding — still the NaN it was
    P = line_pitch(nx, g)
    assert P % 16 == 0 and pitch <= P < pitch + 16
    for f in STATE:
        mid = _whole(dev, grid.alt[f])
        assert mid.size >= P * rows
        plane = mid[:P * rows].reshape(rows, P)
        assert np.isfinite(plane[g:g + ny, g:g + nx]).all(), f"{f}: real cells of the intermediate not written at pitch {P}"
        outside = np.ones(mid.size, dtype=bool)
        outside[:P * rows].reshape(rows, P)[g:g + ny, g:g + nx] = False
        assert np.isnan(mid[outside]).all(), f"{f}: the X sweep of the pair wrote outside the real cells of the intermediate"


def test_pair_refuses_what_it_cannot_run(dev):
    """Too small an intermediate, a remote Y side, a partial sweep, arrays that do not chain: errors, not launches."""
    import armon_amd
    from armon_amd.blocking import Axis
    from armon_amd.solver import BlockGrid, init_test, sweep_desc
    params = armon_amd.ArmonParameters(test="Sod", N=(64, 40), silent=5, ctx=dev.ctx, placement_min_bytes=0)
    grid = BlockGrid(params)
    init_test(params, grid, tune=False)
    L, cap = dev._L, grid.alt["rho"].capacity_bytes

    def descs():
        d_x = sweep_desc(params, grid, Axis.X, 1e-4, params.cell_size(0))
        grid.swap_state()
        d_y = sweep_desc(params, grid, Axis.Y, 1e-4, params.cell_size(1), emit_dt=True)
        grid.swap_state()
        return d_x, d_y

    d_x, d_y = descs()
    assert L.armon_hip_sweep_pair(dev.ctx, C.byref(d_x), C.byref(d_y), grid.alt["rho"].nbytes) == 1
    assert b"intermediate" in L.armon_hip_last_error()
    d_x, d_y = descs()
    d_y.bc_high = 0
    assert L.armon_hip_sweep_pair(dev.ctx, C.byref(d_x), C.byref(d_y), cap) == 1 and b"remote" in L.armon_hip_last_error()
    d_x, d_y = descs()
    d_y.out_lo, d_y.out_hi = 0, 8
    assert L.armon_hip_sweep_pair(dev.ctx, C.byref(d_x), C.byref(d_y), cap) == 1 and b"whole sweeps" in L.armon_hip_last_error()
    d_x, d_y = descs()
    d_y.u_in, d_y.v_in = d_y.v_in, d_y.u_in
    assert L.armon_hip_sweep_pair(dev.ctx, C.byref(d_x), C.byref(d_y), cap) == 1 and b"must read" in L.armon_hip_last_error()
    d_x, d_y = descs()
    assert L.armon_hip_sweep_pair(dev.ctx, C.byref(d_x), C.byref(d_y), cap) == 0, L.armon_hip_last_error()
    dev.wait()


@pytest.mark.parametrize("graph", [False, True], ids=["host-driven", "graph"])
def test_solver_runs_its_cycles_through_the_pair(graph):
    """A whole run of the solver (which takes the pair for a lone block with Sequential splitting that is large enough to be
    placed: placement_min_bytes = 0 here) against the same run with
    kernel callbacks installed, which keeps it on the two plain sweeps: same cycles, same last dt, same bits."""
    import armon_amd
    from armon_amd.solver import pair_cycle

    class Count:
        def __init__(self):
            self.names = []

        def start(self, name):
            self.names.append(name)

        def end(self, name):
            pass

    runs = []
    for cbs in ([], [Count()]):
        params = armon_amd.ArmonParameters(test="Sod_circ", N=(64, 40), maxcycle=12, silent=5, return_data=True,
                                           graph_cycles=graph and not cbs, placement_min_bytes=0)
        params.kernel_callbacks = cbs
        stats = armon_amd.armon(params)
        assert pair_cycle(params, stats.data) == (not cbs)
        runs.append((stats, stats.data.device_to_host(STATE + ("p",))))
    (a, fa), (b, fb) = runs
    assert b.data.params.kernel_callbacks[0].names.count("sweep_y") == 12          # the plain path really ran
    assert a.cycles == b.cycles == 12 and a.last_dt == b.last_dt
    for f in STATE + ("p",):
        assert np.array_equal(_bits(fa[f]), _bits(fb[f])), f
