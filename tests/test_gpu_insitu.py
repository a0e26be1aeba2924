"""In-situ reduced output on the GPU: armon_hip_coarsen / armon_hip_gather_strided and the Python surface over them
(BlockGrid.coarsen, TileGroup.coarsen, output_coarsen, write_slices_files).

The host restatements below are written here (numpy, block sums in longdouble). The value bounds are derived, not measured:
products and sums of n terms in the run's type, in any order, are off by at most (n + 2) eps S|term| (eps = machine epsilon
= twice the unit roundoff), so |rho_c - ref| <= (n + 2) eps S(rho) / n, likewise p, and for the quotients
|q_c - ref| <= (2 n + 6) eps S|rho q| / S(rho).

That model holds while nothing underflows, and test_coarse_values_within_the_derived_bound applies it as it stands to every
test case, type, grid and factor of its list. One combination of the odd-pitch grid is outside the model: Sedov in fp32 on
777 x 1000 has, after 6 cycles, velocities of a few 1e-45 — a handful of SUBNORMAL units — ahead of the blast, and a coarse
u of ~1e-44 cannot be stored in fp32 to within 1e-48 whatever computes it (measured: error 2.6e-46 = 0.19 subnormal units
where the relative bound is 6.8e-49, factors 16x16 and 7x3). That combination is checked by a test of its own,
test_subnormal_velocities_stay_within_half_a_subnormal_unit, whose bound adds the underflow term of the same standard model,
fl(a op b) = (a op b)(1 + d) + h with |h| <= tiny / 2, tiny = the type's smallest subnormal: one h for the final division and,
for the quotients, one per product, divided by S(rho).

With output_coarsen left at 0 nothing of the existing output path changes; that the full-grid files stay what they were is
checked by the untouched tests/test_gpu_solver.py::test_write_output_in_reference_format and
::test_animation_frames_and_slices (output, frames and the three slice files against the fields themselves)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E", "p")
DTYPES = ["float64", "float32"]
LD = np.longdouble

_states = {}


def state_of(test, N, dtype, **kw):
    """A grid a few fused cycles into ``test`` (p materialised by the last cycle). Cached: many cases share one run."""
    import armon_amd
    key = (test, N, dtype, tuple(sorted(kw.items())))
    if key not in _states:
        params = armon_amd.ArmonParameters(test=test, N=N, data_type=dtype, maxcycle=6, silent=5, return_data=True, **kw)
        _states[key] = armon_amd.armon(params).data
    return _states[key]


@pytest.fixture(scope="module", autouse=True)
def release_states():
    yield
    _states.clear()


def real_fields(grid, names=STATE):
    host = grid.device_to_host(names)
    return {k: grid.real_view(host[k]).copy() for k in names}


def block_sums(a, fx, fy):
    """Sum of every fx x fy block (partial at the high ends) of a (ny, nx) longdouble array -> (cny, cnx)."""
    ny, nx = a.shape
    return np.add.reduceat(np.add.reduceat(a, np.arange(0, ny, fy), axis=0), np.arange(0, nx, fx), axis=1)


def host_coarsen(f, fx, fy, underflow=False):
    """Reference planes and the derived error bound of each, in longdouble, from the real cells ``f`` (dict of (ny, nx)).
    ``underflow``: add the absolute term of gradual underflow to the bounds (see the head of this file)."""
    eps = LD(np.finfo(f["rho"].dtype).eps)
    tiny = LD(np.finfo(f["rho"].dtype).smallest_subnormal) if underflow else LD(0)
    ld = {k: v.astype(LD) for k, v in f.items()}
    n = block_sums(np.ones_like(ld["rho"]), fx, fy)
    s_rho = block_sums(ld["rho"], fx, fy)
    ref = {"rho": s_rho / n}
    bound = {"rho": (n + 2) * eps * block_sums(np.abs(ld["rho"]), fx, fy) / n + tiny / 2}
    if "p" in ld:
        ref["p"] = block_sums(ld["p"], fx, fy) / n
        bound["p"] = (n + 2) * eps * block_sums(np.abs(ld["p"]), fx, fy) / n + tiny / 2
    for q in ("u", "v", "E"):
        ref[q] = block_sums(ld["rho"] * ld[q], fx, fy) / s_rho
        bound[q] = (2 * n + 6) * eps * block_sums(np.abs(ld["rho"] * ld[q]), fx, fy) / s_rho + tiny * (n / s_rho + 1) / 2
    return ref, bound, n


def check_values(grid, factor, f=None, underflow=False):
    from armon_amd.parameters import coarse_shape
    fx, fy = factor
    f = real_fields(grid) if f is None else f
    ny, nx = f["rho"].shape
    planes = grid.coarsen(factor)
    ref, bound, _n = host_coarsen(f, min(fx, nx), min(fy, ny), underflow)
    cnx, cny = coarse_shape((nx, ny), factor)
    for k in STATE:
        got = planes[k]
        assert got.shape == (cny, cnx) and got.dtype == f[k].dtype, (k, got.shape, got.dtype)
        err = np.abs(got.astype(LD) - ref[k])
        worst = np.unravel_index(np.argmax(err - bound[k]), err.shape)
        print(f"{k}: max err {float(err.max()):.3e}, at the worst cell err {float(err[worst]):.3e} <= bound {float(bound[k][worst]):.3e}")
        assert np.all(err <= bound[k]), (k, factor, worst, float(err[worst]), float(bound[k][worst]))
    # x, y: the stored coordinates of the first cell each coarse cell covers
    xy = real_fields(grid, ("x", "y"))
    assert np.array_equal(planes["x"], xy["x"][::min(fy, ny), ::min(fx, nx)])
    assert np.array_equal(planes["y"], xy["y"][::min(fy, ny), ::min(fx, nx)])
    return planes


# the issue's cases, then factors that take the other launch forms: fy > 64 (row chunks), fx not a power of two, fx > 64,
# fx > 256 (columns 256 apart added first), and an odd row pitch (777 + 8: no 16-byte loads in fp64)
CASES = [
    ((1024, 1024), (16, 16)),
    ((1000, 777), (16, 16)),
    ((1000, 777), (7, 3)),
    ((1000, 777), (64, 8)),
    ((1000, 777), (1, 1)),
    ((1000, 777), (2048, 1024)),
    ((1000, 777), (4096, 100000)),
    ((1000, 777), (16, 100)),
    ((1000, 777), (100, 16)),
    ((1000, 777), (128, 2)),
    ((1000, 777), (300, 5)),
    ((1000, 777), (1, 200)),
    ((1000, 777), (2, 64)),
]
ODD_PITCH_CASES = [((777, 1000), (16, 16)), ((777, 1000), (7, 3)), ((777, 1000), (1, 1))]
case_id = lambda v: "x".join(str(i) for i in v)


@pytest.mark.parametrize("N,factor", CASES, ids=case_id)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", ["Sod", "Sedov", "Bizarrium"])
def test_coarse_values_within_the_derived_bound(test, dtype, N, factor):
    check_values(state_of(test, N, dtype), factor)


@pytest.mark.parametrize("N,factor", ODD_PITCH_CASES, ids=case_id)
@pytest.mark.parametrize("test,dtype", [("Sod", "float64"), ("Sod", "float32"), ("Sedov", "float64"),
                                        ("Bizarrium", "float64"), ("Bizarrium", "float32")])
def test_coarse_values_on_an_odd_row_pitch(test, dtype, N, factor):
    """Rows of 785 elements: no 16-byte loads in fp64, and none in fp32 either. Same bound. (Sedov in fp32 on this grid has
    subnormal velocities: next test.)"""
    check_values(state_of(test, N, dtype), factor)


@pytest.mark.parametrize("N,factor", ODD_PITCH_CASES, ids=case_id)
def test_subnormal_velocities_stay_within_half_a_subnormal_unit(N, factor):
    check_values(state_of("Sedov", N, "float32"), factor, underflow=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", ["Sod", "Sedov", "Bizarrium"])
def test_factor_one_is_exact(test, dtype):
    grid = state_of(test, (1000, 777), dtype)
    f = real_fields(grid)
    planes = grid.coarsen(1)
    assert planes["rho"].tobytes() == f["rho"].tobytes()
    assert planes["p"].tobytes() == f["p"].tobytes()
    assert planes["rho"].shape == (777, 1000)


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_p(dtype):
    grid = state_of("Sedov", (1000, 777), dtype)
    for factor in ((16, 16), (7, 3)):
        with_p, without = grid.coarsen(factor), grid.coarsen(factor, with_p=False)
        assert "p" not in without
        for k in ("rho", "u", "v", "E", "x", "y"):
            assert without[k].tobytes() == with_p[k].tobytes(), (factor, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", ["Sod", "Sedov", "Bizarrium"])
def test_two_calls_give_the_same_bits(test, dtype):
    grid = state_of(test, (1000, 777), dtype)
    for factor in ((16, 16), (7, 3), (64, 8), (2048, 1024), (300, 5)):
        a, b = grid.coarsen(factor), grid.coarsen(factor)
        for k in STATE:
            assert a[k].tobytes() == b[k].tobytes(), (factor, k)


TILE_FACTORS = [(8, 8), (16, 3), (6, 6), (3, 16), (48, 48), (1, 1), (24, 2)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("P", [(2, 2), (4, 2)])
def test_tile_group_equals_the_single_block(P, dtype):
    """Exact arithmetic: the tiles hold the single block's bits, the factor is aligned with the tiles — the assembled planes
    must be the single block's, every bit (the kernel's summation order does not depend on where a coarse cell is stored)."""
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    kw = dict(test="Sedov", N=(192, 96), maxcycle=8, silent=5, exact_arithmetic=True, data_type=dtype)
    ref = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **kw)).data
    group = TileGroup(P, **kw)
    try:
        group.run()
        tiles = group.gather()
        single = real_fields(ref)
        for k in STATE:
            assert np.array_equal(tiles[k], single[k]), k            # the premise
        for factor in TILE_FACTORS:
            a, b = group.coarsen(factor), ref.coarsen(factor)
            for k in STATE + ("x", "y"):
                assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (factor, k)
        with pytest.raises(armon_amd.SolverException) as e:
            group.coarsen((5, 8))                                    # tiles start at multiples of 48 or 96 along x
        assert e.value.category == "config" and "tile boundaries" in e.value.msg
    finally:
        group.close()


def test_tile_group_takes_the_option_and_refuses_a_misaligned_one():
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    kw = dict(test="Sod", N=(192, 96), maxcycle=2, silent=5)
    with pytest.raises(armon_amd.SolverException) as e:
        TileGroup((2, 2), output_coarsen=(64, 8), **kw)                # 96 % 64 != 0
    assert e.value.category == "config" and "tile boundaries" in e.value.msg
    group = TileGroup((2, 2), output_coarsen=(32, 8), **kw)
    try:
        group.run()
        planes = group.coarsen()
        assert planes["rho"].shape == (12, 6)
    finally:
        group.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_field_under_another_ghost_width_gives_the_same_bits(dtype):
    """The same real cells in a block with 5 ghost layers instead of 4: every row lands on another alignment (and the 16-byte
    loads give way to element-wide ones) — the coarse planes must not change by a bit."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test
    for N in ((1000, 777), (777, 1000)):
        grid = state_of("Sedov", N, dtype)
        f = real_fields(grid)
        params5 = armon_amd.ArmonParameters(test="Sedov", N=N, data_type=dtype, nghost=5, silent=5)
        other = BlockGrid(params5)
        init_test(params5, other)
        host = other.device_to_host(STATE)
        for k in STATE:
            other.real_view(host[k])[...] = f[k]
        other.host_to_device(host)
        for factor in ((16, 16), (7, 3), (64, 8), (1, 1), (2, 64), (300, 5), (2048, 1024)):
            a, b = grid.coarsen(factor), other.coarsen(factor)
            for k in STATE:
                assert a[k].tobytes() == b[k].tobytes(), (N, factor, k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", ["Sod", "Sedov", "Bizarrium"])
def test_coarse_planes_conserve_mass_and_energy(test, dtype):
    """S n rho_c ds and S n rho_c E_c ds over the coarse cells against conservation_vars: both are any-order sums of N
    positive terms in the run's type, so they agree to 2 N eps relative (derived, loose on purpose)."""
    from armon_amd.solver import conservation_vars
    grid = state_of(test, (1000, 777), dtype)
    params = grid.params
    N = 1000 * 777
    eps = float(np.finfo(params.data_type).eps)
    mass, energy = conservation_vars(params, grid)
    ds = LD(params.cell_size(0)) * LD(params.cell_size(1))
    for factor in ((16, 16), (7, 3), (64, 8), (1, 1), (2048, 1024)):
        planes = grid.coarsen(factor)
        n = block_sums(np.ones((777, 1000), dtype=LD), min(factor[0], 1000), min(factor[1], 777))
        m = (n * planes["rho"].astype(LD) * ds).sum()
        e = (n * planes["rho"].astype(LD) * planes["E"].astype(LD) * ds).sum()
        print(f"{factor}: |dM|/M = {float(abs(m - mass) / mass):.3e}, |dE|/E = {float(abs(e - energy) / energy):.3e}, bound {2 * N * eps:.3e}")
        assert abs(m - LD(mass)) <= 2 * N * eps * abs(mass), (factor, float(m), mass)
        assert abs(e - LD(energy)) <= 2 * N * eps * abs(energy), (factor, float(e), energy)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ghost_cells_are_not_read(dtype):
    """The device of the reference's uninit_vars_propagation test: poison every ghost cell, get the same planes."""
    import armon_amd
    for N in ((1000, 777), (777, 1000)):
        params = armon_amd.ArmonParameters(test="Sedov", N=N, data_type=dtype, maxcycle=6, silent=5, return_data=True)
        grid = armon_amd.armon(params).data
        factors = ((16, 16), (7, 3), (64, 8), (1, 1), (2048, 1024), (300, 5), (16, 100))
        before = [grid.coarsen(f) for f in factors]
        host = grid.device_to_host(STATE)
        g = params.nghost
        for k in STATE:
            a = host[k].reshape(N[1] + 2 * g, N[0] + 2 * g)
            keep = a[g:g + N[1], g:g + N[0]].copy()
            a[...] = 1e100 if dtype == "float64" else 1e30
            a[g:g + N[1], g:g + N[0]] = keep
        grid.host_to_device(host)
        for f, b in zip(factors, before):
            a = grid.coarsen(f)
            for k in STATE:
                assert a[k].tobytes() == b[k].tobytes(), (N, f, k)


def test_bad_arguments_are_refused_before_any_launch():
    import ctypes as C
    import armon_amd
    grid = state_of("Sod", (1000, 777), "float64")
    dev, L = grid.params.device, armon_amd.lib()
    out = dev.empty(5 * 1000 * 777, np.float64)
    P = lambda k: C.c_void_p(grid.data[k].ptr)
    ok = (dev.ctx, 1008, 4, 1000, 777, 16, 16, P("rho"), P("u"), P("v"), P("E"), P("p"), C.c_void_p(out.ptr))

    def call(**change):
        names = ("ctx", "row_length", "nghost", "nx", "ny", "fx", "fy", "rho", "u", "v", "E", "p", "out")
        return L.armon_hip_coarsen(*[change.get(n, a) for n, a in zip(names, ok)])

    assert call() == 0
    assert call(p=None) == 0                                         # p is optional
    for bad in (dict(fx=0), dict(fy=0), dict(fx=-4), dict(rho=None), dict(E=None), dict(out=None), dict(ctx=None),
                dict(row_length=1007), dict(nx=0), dict(ny=-1), dict(nghost=-1)):
        assert call(**bad) == 1, bad                                 # ARMON_ERR_INVALID_ARG
        assert L.armon_hip_last_error()
    n = grid.size.n_cells
    vars_ = (C.c_void_p * 2)(grid.data["rho"].ptr, grid.data["u"].ptr)
    gs = lambda *a: L.armon_hip_gather_strided(dev.ctx, *a)
    assert gs(n, 2, vars_, 0, 1, 10, C.c_void_p(out.ptr)) == 0
    assert gs(n, 2, vars_, n - 1, 1, 1, C.c_void_p(out.ptr)) == 0
    assert gs(n, 2, vars_, 5, 7, 0, C.c_void_p(out.ptr)) == 0        # nothing to do
    for bad in ((n, 0, vars_, 0, 1, 10), (n, 9, vars_, 0, 1, 10), (n, 2, vars_, -1, 1, 10), (n, 2, vars_, 0, 0, 10),
                (n, 2, vars_, n - 5, 1, 6), (n, 2, vars_, 0, 1008, 786), (n, 2, vars_, n, 1, 1), (n, 2, None, 0, 1, 10),
                (n, 2, (C.c_void_p * 2)(grid.data["rho"].ptr, None), 0, 1, 10)):
        assert gs(*bad, C.c_void_p(out.ptr)) == 1, bad[3:]
    assert gs(n, 2, vars_, 0, 1, 10, None) == 1
    dev.wait()
    out.free()


def write_slices_by_hand(params, grid, file_name):
    """The three slice files from whole fields on the host: the row j = g + Ny//2, the column i = g + Nx//2, the diagonal
    (y0 + k, x0 + k), in the cell format of the output files."""
    from armon_amd import io as aio
    host = grid.device_to_host(aio.SAVED_VARS)
    g, (nx, ny) = params.nghost, params.N
    sx = nx + 2 * g
    if params.write_ghosts:
        (x0, x1), (y0, y1) = (0, nx + 2 * g), (0, ny + 2 * g)
    else:
        (x0, x1), (y0, y1) = (g, g + nx), (g, g + ny)
    cols = [host[v].reshape(-1, sx) for v in aio.SAVED_VARS]
    w = params.output_precision
    fmt = ", ".join([f"%#{w + 7}.{w}e"] * len(cols)) + "\n"
    jm, im = g + ny // 2, g + nx // 2
    cells = {"X": [(jm, i) for i in range(x0, x1)], "Y": [(j, im) for j in range(y0, y1)],
             "diag": [(y0 + k, x0 + k) for k in range(min(x1 - x0, y1 - y0))]}
    paths = {}
    for tag, picks in cells.items():
        paths[tag] = os.path.join(params.output_dir, f"{file_name}_{tag}")
        with open(paths[tag], "w") as f:
            f.write("".join(fmt % tuple(c[j, i] for c in cols) for j, i in picks))
    return paths


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ghosts", [False, True], ids=["real", "ghosts"])
@pytest.mark.parametrize("test", ["Sod", "Sedov"])
def test_slices_come_from_the_gather_kernel(tmp_path, monkeypatch, test, ghosts, dtype):
    import armon_amd
    from armon_amd import io as aio
    from armon_amd.solver import BlockGrid
    params = armon_amd.ArmonParameters(test=test, N=(123, 77), data_type=dtype, maxcycle=6, silent=5, return_data=True,
                                       write_ghosts=ghosts, output_dir=str(tmp_path))
    grid = armon_amd.armon(params).data
    expected = write_slices_by_hand(params, grid, "hand")

    def no_full_fields(self, names=None):
        raise AssertionError("device_to_host called")

    with monkeypatch.context() as m:
        m.setattr(BlockGrid, "device_to_host", no_full_fields)
        paths = aio.write_slices_files(params, grid, "dev")
    assert [os.path.basename(p) for p in paths] == ["dev_X", "dev_Y", "dev_diag"]
    for tag, path in zip(("X", "Y", "diag"), paths):
        got, want = open(path, "rb").read(), open(expected[tag], "rb").read()
        assert len(want) > 0 and got == want, tag


def test_end_to_end_coarse_output_and_frames(tmp_path, monkeypatch):
    import armon_amd
    from armon_amd import io as aio
    from armon_amd.device import DeviceArray
    from armon_amd.solver import BlockGrid
    N, factor = (1000, 777), (8, 8)
    cnx, cny = 125, 98
    params = armon_amd.ArmonParameters(test="Sedov", N=N, output_coarsen=factor, write_output=True, animation_step=5,
                                       maxcycle=20, silent=5, return_data=True, output_dir=str(tmp_path), output_file="run")
    full = params.block_size.n_cells
    to_host = DeviceArray.to_host

    def no_full_fields(self, names=None):
        raise AssertionError("device_to_host called")

    def small_copies_only(self, out=None):
        assert self.n < full, "a full field crossed to the host"
        return to_host(self, out)

    with monkeypatch.context() as m:
        m.setattr(BlockGrid, "device_to_host", no_full_fields)
        m.setattr(DeviceArray, "to_host", small_copies_only)
        stats = armon_amd.armon(params)
    assert stats.cycles == 20
    cells = lambda path: sum(1 for line in open(path) if line.strip())
    assert cells(tmp_path / "run") == cnx * cny
    frames = sorted(os.listdir(tmp_path / "anim"))
    assert frames == ["run_000", "run_001", "run_002", "run_003"]            # after cycles 1, 6, 11, 16
    for name in frames:
        assert cells(tmp_path / "anim" / name) == cnx * cny
        assert open(tmp_path / "anim" / name).read().count("\n\n") == cny - 1
    back = aio.read_coarse_file(params, "run")
    planes = stats.data.coarsen(factor)
    w = params.output_precision
    for k in aio.SAVED_VARS:
        assert back[k].shape == (cny, cnx)
        formatted = np.array([float(f"%#{w + 7}.{w}e" % val) for val in planes[k].ravel()]).reshape(cny, cnx)
        assert np.array_equal(back[k], formatted), k
    # the first frame is the state after cycle 1: the coarse output of a run that stops there
    p1 = armon_amd.ArmonParameters(test="Sedov", N=N, output_coarsen=factor, write_output=True, maxcycle=1, silent=5,
                                   output_dir=str(tmp_path), output_file="stop1")
    armon_amd.armon(p1)
    assert open(tmp_path / "stop1", "rb").read() == open(tmp_path / "anim" / "run_000", "rb").read()
