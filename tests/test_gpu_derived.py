"""Derived flow fields on the GPU: armon_hip_derive and the Python surface over it (BlockGrid.derive, TileGroup.derive, the
image_* options, the PNG frames).

The per-cell rule is restated in numpy by ``derived.reference_planes`` (float64 or float32 throughout, same operation order);
the kernel has to give its bits. At factor 1 a MAX or MIN plane IS the per-cell value; a MEAN plane is ``(0 + d) / 1``, which
differs from ``d`` only where ``d`` is -0. A MEAN at a larger factor is held to the bound that holds for ANY summation order
plus one division: ``|mean - exact| <= (n + 1) u mean|d|`` with n the cells covered, u the unit roundoff of the type and the
exact mean taken with ``math.fsum``; the order itself is pinned by ``derive(["rho"]) == coarsen()["rho"]``, bit for bit.

The raw-call tests build random states (rho in [0.5, 2], u, v in [-1, 1], internal energy in [1, 3]: non-zero velocities and
gradients everywhere, p > 0) in blocks whose every ghost cell is NaN unless a test says otherwise, so that a ghost cell read
where none may be read turns up in the result.

NaN propagation: a derivative at cell i reads i-1 and i+1, not i. So one NaN in an interior cell makes the stencil quantities
NaN in the coarse cells that cover one of its four neighbours; with factors >= 2 along both axes that is the same set as "the
coarse cells that cover the NaN cell or one of its four neighbours" (the coarse cell of the NaN cell always holds one of them),
which the test asserts for those factors; at factor 1 it is the four neighbours alone. speed, e, vorticity and divergence do not
read rho: they are checked with the NaN in all four fields of the cell, rho / p / mach / grad_rho also with the NaN in rho alone
(then the other four keep every bit)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
ALL = ("rho", "p", "e", "speed", "mach", "grad_rho", "vorticity", "divergence")
POINTWISE, STENCIL = ALL[:5], ALL[5:]
READS_RHO = ("rho", "p", "mach", "grad_rho")
MODES = ("mean", "max", "min")
GAMMA = 1.4
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (127, 3), (128, 65), (129, 64), (257, 130)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def dev():
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.close()


def random_state(nx, ny, dtype, seed):
    """rho, u, v, E as (ny, nx) arrays of ``dtype``."""
    rng = np.random.default_rng([seed, nx, ny])
    T = np.dtype(dtype).type
    rho = rng.uniform(0.5, 2.0, (ny, nx)).astype(dtype)
    u = rng.uniform(-1.0, 1.0, (ny, nx)).astype(dtype)
    v = rng.uniform(-1.0, 1.0, (ny, nx)).astype(dtype)
    e = rng.uniform(1.0, 3.0, (ny, nx)).astype(dtype)
    return rho, u, v, (e + T(0.5) * (u * u + v * v)).astype(dtype)


def ghosted(a, g, pitch=None, fill=np.nan):
    ny, nx = a.shape
    pitch = nx + 2 * g if pitch is None else pitch
    out = np.full((ny + 2 * g, pitch), fill, dtype=a.dtype)
    out[g:g + ny, g:g + nx] = a
    return out


def coarse_shape(nx, ny, fx, fy):
    return -(-nx // min(fx, nx)), -(-ny // min(fy, ny))


def make_spec(names, modes, neighbours=0, dx=0.01, dy=0.02, gamma=GAMMA, eos=0):
    from armon_amd._lib import DeriveSpec
    from armon_amd import derived
    s = DeriveSpec()
    s.nq = len(names)
    for k, (q, m) in enumerate(zip(names, modes)):
        s.quantity[k], s.reduce[k] = derived.QUANTITIES.index(q), derived.REDUCTIONS.index(m)
    s.eos, s.neighbours, s.gamma, s.dx, s.dy = eos, neighbours, gamma, dx, dy
    return s


def raw_derive(dev, blocks, g, nx, ny, factor=(1, 1), names=ALL, modes="mean", **spec):
    """armon_hip_derive on the ghosted 2-D host arrays ``blocks`` = (rho, u, v, E) → dict name → (cny, cnx) plane."""
    dtype = blocks[0].dtype
    suffix = "_f32" if dtype == np.float32 else ""
    modes = (modes,) * len(names) if isinstance(modes, str) else modes
    pitch = blocks[0].shape[1]
    cnx, cny = coarse_shape(nx, ny, *factor)
    arrays = [dev.from_host(b.ravel()) for b in blocks]
    out = dev.from_host(np.full(len(names) * cnx * cny, -777.0, dtype=dtype))
    try:
        s = make_spec(names, modes, **spec)
        rc = getattr(dev._L, "armon_hip_derive" + suffix)(dev.ctx, pitch, g, nx, ny, factor[0], factor[1],
                                                         *[C.c_void_p(a.ptr) for a in arrays], C.byref(s), C.c_void_p(out.ptr))
        assert rc == 0, dev._L.armon_hip_last_error()
        dev.wait()
        planes = out.to_host().reshape(len(names), cny, cnx)
    finally:
        for a in arrays + [out]:
            a.free()
    return {q: planes[k].copy() for k, q in enumerate(names)}


def reference(state, dtype, dx=0.01, dy=0.02):
    from armon_amd import derived
    T = np.dtype(dtype).type
    return derived.reference_planes(*state, T(dx), T(dy), GAMMA)


# ---- factor 1 is exact -----------------------------------------------------------------------------------------------------
def check_factor_one(dev, state, g, pitch=None):
    ny, nx = state[0].shape
    dtype = state[0].dtype
    ref = reference(state, dtype)
    blocks = [ghosted(a, g, pitch) for a in state]
    for mode in MODES:
        got = raw_derive(dev, blocks, g, nx, ny, modes=mode)
        for q in ALL:
            want = ref[q] if mode != "mean" else (np.zeros_like(ref[q]) + ref[q])      # the mean of one value: (0 + d) / 1
            assert same_bits(got[q], want), (q, mode, nx, ny, np.argwhere(bits(got[q]) != bits(want))[:4].tolist())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_factor_one_equals_the_numpy_reference_bit_for_bit(dev, dtype, shape):
    # ghost width 4: rows start on a 16-B boundary when nx is a multiple of the lane width, and do not otherwise
    check_factor_one(dev, random_state(shape[0], shape[1], dtype, 1), 4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape, g, pitch", [((128, 65), 3, 135), ((257, 130), 5, None), ((128, 65), 1, None), ((256, 9), 0, None)],
                         ids=["odd-padded-pitch", "odd-pitch-nghost5", "nghost1", "nghost0"])
def test_factor_one_with_an_odd_row_pitch_and_other_ghost_widths(dev, dtype, shape, g, pitch):
    check_factor_one(dev, random_state(shape[0], shape[1], dtype, 2), g, pitch)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("test", ["Bizarrium", "Sod_circ"])
def test_p_and_mach_are_those_of_the_staged_eos(dtype, test):
    import armon_amd
    from armon_amd import solver as S
    params = armon_amd.ArmonParameters(test=test, N=(129, 70), data_type=dtype, maxcycle=5, silent=5, return_data=True)
    grid = armon_amd.armon(params).data
    got = grid.derive(["p", "mach", "speed"], reduce="max")
    S.update_EOS(params, grid)                          # the staged kernel: p, c (and g) of the state as it stands
    host = grid.device_to_host(("u", "v", "p", "c"))
    u, v, p, c = (grid.real_view(host[k]).copy() for k in ("u", "v", "p", "c"))
    assert np.abs(u).max() > 0
    with np.errstate(all="ignore"):
        speed = np.sqrt(u * u + v * v)
        assert same_bits(got["p"], p)
        assert same_bits(got["speed"], speed)
        assert same_bits(got["mach"], speed / c)


# ---- factors ---------------------------------------------------------------------------------------------------------------
FACTORS = [(2, 2), (64, 64), (4, 3), (3, 5), (128, 70), (1000, 1000)]
_runs = {}


def run_state(test, N, dtype, **kw):
    import armon_amd
    key = (test, N, dtype, tuple(sorted(kw.items())))
    if key not in _runs:
        params = armon_amd.ArmonParameters(test=test, N=N, data_type=dtype, maxcycle=6, silent=5, return_data=True, **kw)
        _runs[key] = armon_amd.armon(params).data
    return _runs[key]


@pytest.fixture(scope="module", autouse=True)
def release_runs():
    yield
    _runs.clear()


@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_mean_rho_is_coarsens_rho_bit_for_bit(dtype, factor):
    grid = run_state("Sod_circ", (257, 130), dtype)
    mine, theirs = grid.derive(["rho"], factor), grid.coarsen(factor, with_p=False)
    assert same_bits(mine["rho"], theirs["rho"])
    assert np.array_equal(mine["x"], theirs["x"]) and np.array_equal(mine["y"], theirs["y"])


def block_reduce(op, a, fx, fy):
    ny, nx = a.shape
    return op.reduceat(op.reduceat(a, np.arange(0, ny, min(fy, ny)), axis=0), np.arange(0, nx, min(fx, nx)), axis=1)


@pytest.mark.parametrize("factor", FACTORS, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_max_min_and_mean_over_the_factor_one_planes(dev, dtype, factor):
    nx, ny = 257, 130
    state = random_state(nx, ny, dtype, 3)
    blocks = [ghosted(a, 4) for a in state]
    cells = raw_derive(dev, blocks, 4, nx, ny, modes="max")                     # the per-cell values themselves
    for mode, op in (("max", np.maximum), ("min", np.minimum)):
        got = raw_derive(dev, blocks, 4, nx, ny, factor, modes=mode)
        for q in ALL:
            assert np.array_equal(got[q], block_reduce(op, cells[q], *factor)), (q, mode)
    got = raw_derive(dev, blocks, 4, nx, ny, factor, modes="mean")
    unit = np.finfo(dtype).eps / 2
    fx, fy = min(factor[0], nx), min(factor[1], ny)
    for q in ALL:
        d = cells[q].astype(np.float64)
        for J in range(got[q].shape[0]):
            for I in range(got[q].shape[1]):
                cov = d[J * fy:(J + 1) * fy, I * fx:(I + 1) * fx].ravel().tolist()
                n = len(cov)
                exact, mean_abs = math.fsum(cov) / n, math.fsum(abs(x) for x in cov) / n
                err = abs(float(got[q][J, I]) - exact)
                assert err <= (n + 1) * unit * mean_abs, (q, I, J, n, err, (n + 1) * unit * mean_abs)


# ---- determinism and layout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_and_two_ghost_widths_give_the_same_bits(dev, dtype):
    nx, ny = 257, 130
    state = random_state(nx, ny, dtype, 4)
    for factor in ((1, 1), (4, 3), (64, 64), (128, 70)):
        for mode in MODES:
            first = raw_derive(dev, [ghosted(a, 4) for a in state], 4, nx, ny, factor, modes=mode)
            again = raw_derive(dev, [ghosted(a, 4) for a in state], 4, nx, ny, factor, modes=mode)
            other = raw_derive(dev, [ghosted(a, 5) for a in state], 5, nx, ny, factor, modes=mode)
            for q in ALL:
                assert same_bits(first[q], again[q]), (q, factor, mode)
                assert same_bits(first[q], other[q]), (q, factor, mode)


def test_mixed_reductions_in_one_call(dev):
    nx, ny = 130, 67
    state = random_state(nx, ny, "float64", 5)
    blocks = [ghosted(a, 4) for a in state]
    names, modes = ("grad_rho", "mach", "vorticity", "rho"), ("max", "min", "mean", "max")
    got = raw_derive(dev, blocks, 4, nx, ny, (4, 3), names, modes)
    for q, m in zip(names, modes):
        assert same_bits(got[q], raw_derive(dev, blocks, 4, nx, ny, (4, 3), (q,), m)[q]), (q, m)


# ---- tiles -----------------------------------------------------------------------------------------------------------------
def tile_block(state, x0, y0, nx, ny, g, bits_set, deep=np.nan):
    """The ghosted block of the window [x0, x0 + nx) x [y0, y0 + ny) of a global state: the first ghost layer of the flagged
    sides holds the neighbour's cells, every other ghost cell (deeper layers, corners, unflagged sides) is ``deep``."""
    out = []
    for a in state:
        b = ghosted(a[y0:y0 + ny, x0:x0 + nx], g, fill=deep)
        if bits_set & 1:
            b[g:g + ny, g - 1] = a[y0:y0 + ny, x0 - 1]
        if bits_set & 2:
            b[g:g + ny, g + nx] = a[y0:y0 + ny, x0 + nx]
        if bits_set & 4:
            b[g - 1, g:g + nx] = a[y0 - 1, x0:x0 + nx]
        if bits_set & 8:
            b[g + ny, g:g + nx] = a[y0 + ny, x0:x0 + nx]
        out.append(b)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [1, 4])
def test_a_window_with_flagged_sides_gives_the_whole_domains_bits(dev, dtype, g):
    """Every combination of neighbours, cut from one global state; only the first ghost layer of the flagged sides is not NaN."""
    NX, NY = 300, 140
    state = random_state(NX, NY, dtype, 6)
    ref = reference(state, dtype)
    xs, ys = [(0, 128), (128, 129), (257, 43)], [(0, 64), (64, 65), (129, 11)]
    for ix, (x0, nx) in enumerate(xs):
        for iy, (y0, ny) in enumerate(ys):
            nb = (1 if ix > 0 else 0) | (2 if ix < 2 else 0) | (4 if iy > 0 else 0) | (8 if iy < 2 else 0)
            got = raw_derive(dev, tile_block(state, x0, y0, nx, ny, g, nb), g, nx, ny, modes="max", neighbours=nb)
            for q in ALL:
                assert same_bits(got[q], ref[q][y0:y0 + ny, x0:x0 + nx]), (q, ix, iy)


@pytest.mark.parametrize("test", ["Sod_circ", "Sedov"])
@pytest.mark.parametrize("P", [(2, 2), (3, 1)], ids=["2x2", "3x1"])
def test_tile_groups_equal_the_single_block_bit_for_bit(test, P):
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    opts = dict(test=test, N=(48, 40), maxcycle=8, silent=5, exact_arithmetic=True)
    single = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **opts)).data
    tg = TileGroup(P, **opts)
    try:
        tg.run()
        assert tg.state_digest() == single.state_digest()
        for factor in ((1, 1), (4, 4)):
            for mode in MODES:
                a, b = single.derive(ALL, factor, mode), tg.derive(ALL, factor, mode)
                for q in ALL + ("x", "y"):
                    assert same_bits(np.ascontiguousarray(a[q]), np.ascontiguousarray(b[q])), (q, factor, mode)
        assert np.abs(a["vorticity"]).max() > 0 and np.abs(a["divergence"]).max() > 0
        with pytest.raises(armon_amd.SolverException) as e:
            tg.derive(["rho"], (7, 7))
        assert e.value.category == "config"
        assert tg.state_digest() == single.state_digest()
    finally:
        tg.close()


# ---- ghost cells -----------------------------------------------------------------------------------------------------------
def poison(grid, keep=0):
    """NaN in every ghost cell of rho, u, v, E of ``grid`` but the first layer's strips of the sides in ``keep`` (bits)."""
    g, (nx, ny) = grid.size.ghosts, grid.size.real_size
    host = grid.device_to_host(("rho", "u", "v", "E"))
    for k, a in host.items():
        b = a.reshape(grid.size.size[1], grid.size.size[0])
        saved = b.copy()
        b[...] = np.nan
        b[g:g + ny, g:g + nx] = saved[g:g + ny, g:g + nx]
        if keep & 1:
            b[g:g + ny, g - 1] = saved[g:g + ny, g - 1]
        if keep & 2:
            b[g:g + ny, g + nx] = saved[g:g + ny, g + nx]
        if keep & 4:
            b[g - 1, g:g + nx] = saved[g - 1, g:g + nx]
        if keep & 8:
            b[g + ny, g:g + nx] = saved[g + ny, g:g + nx]
    grid.host_to_device(host)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_single_block_reads_no_ghost_cell(dtype):
    import armon_amd
    params = armon_amd.ArmonParameters(test="Sedov", N=(130, 67), data_type=dtype, maxcycle=6, silent=5, return_data=True)
    grid = armon_amd.armon(params).data
    before = {f: grid.derive(ALL, f, "max") for f in ((1, 1), (4, 3), (64, 64))}
    poison(grid)
    for f, want in before.items():
        got = grid.derive(ALL, f, "max")
        for q in ALL:
            assert same_bits(got[q], want[q]), (q, f)


def test_a_tile_reads_only_the_first_layer_of_its_neighbours():
    from armon_amd import derived
    from armon_amd.blocking import Axis, sides_along
    from armon_amd.multi_tile import TileGroup
    from armon_amd.solver import STATE_VARS
    tg = TileGroup((2, 2), test="Sod_circ", N=(48, 40), maxcycle=6, silent=5)
    try:
        tg.run()
        want = {f: tg.derive(ALL, f) for f in ((1, 1), (4, 4))}
        tiles = tg._tiles_at_rest()
        for axis in (Axis.X, Axis.Y):
            tg.exchange(sides_along(axis), STATE_VARS)
        tg.wait()
        for p, g in tiles:
            nb = derived.tile_neighbours(p)
            assert nb not in (0, 15)                    # every tile of a 2 x 2 group has two neighbours
            poison(g, keep=nb)                          # layers >= 2, the four corners, the sides without a neighbour
        for f in want:
            got = derived.derive_state(tiles, ALL, f)
            for q in ALL:
                assert same_bits(got[q], want[f][q]), (q, f)
    finally:
        tg.close()


# ---- NaN -------------------------------------------------------------------------------------------------------------------
def covering(cells, fx, fy):
    return {(i // fx, j // fy) for i, j in cells}


@pytest.mark.parametrize("factor", [(1, 1), (2, 2), (4, 3), (64, 64), (70, 70)], ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_nan_cell_reaches_exactly_the_coarse_cells_that_read_it(dev, dtype, factor):
    nx, ny, ci, cj = 140, 75, 67, 33                    # an interior cell whose neighbours lie in other coarse cells for 4 x 3
    fx, fy = factor
    state = random_state(nx, ny, dtype, 7)
    around = [(ci - 1, cj), (ci + 1, cj), (ci, cj - 1), (ci, cj + 1)]
    hit = {"point": covering([(ci, cj)], fx, fy), "stencil": covering(around, fx, fy)}
    if fx >= 2 and fy >= 2:
        assert hit["stencil"] == covering(around + [(ci, cj)], fx, fy)
    canonical = bits(np.array([np.nan], dtype=dtype))[0]
    for fields in ((0,), (0, 1, 2, 3)):
        dirty = [a.copy() for a in state]
        for k in fields:
            dirty[k][cj, ci] = -np.nan if k == 0 else np.nan       # (a NaN of another sign still comes out canonical)
        for mode in MODES:
            clean = raw_derive(dev, [ghosted(a, 4) for a in state], 4, nx, ny, factor, modes=mode)
            got = raw_derive(dev, [ghosted(a, 4) for a in dirty], 4, nx, ny, factor, modes=mode)
            for q in ALL:
                reads = len(fields) == 4 or q in READS_RHO
                want = hit["point" if q in POINTWISE else "stencil"] if reads else set()
                nan_at = {(int(I), int(J)) for J, I in np.argwhere(np.isnan(got[q]))}
                assert nan_at == want, (q, mode, fields)
                mask = np.isnan(got[q])
                assert (bits(got[q])[mask] == canonical).all(), (q, mode)
                assert np.array_equal(bits(got[q])[~mask], bits(clean[q])[~mask]), (q, mode)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(dev):
    nx, ny, g = 20, 10, 2
    state = random_state(nx, ny, "float64", 8)
    blocks = [ghosted(a, g) for a in state]
    pitch = nx + 2 * g
    arrays = [dev.from_host(b.ravel()) for b in blocks]
    sentinel = np.full(8 * nx * ny, -777.0)
    out = dev.from_host(sentinel)
    L = dev._L

    def call(spec=None, null_spec=False, **kw):
        a = dict(pitch=pitch, g=g, nx=nx, ny=ny, fx=1, fy=1, ptrs=[C.c_void_p(x.ptr) for x in arrays], out=C.c_void_p(out.ptr),
                 spec=C.byref(spec if spec is not None else make_spec(ALL, ("mean",) * 8)))
        a.update(kw)
        if null_spec:
            a["spec"] = None
        return L.armon_hip_derive(dev.ctx, a["pitch"], a["g"], a["nx"], a["ny"], a["fx"], a["fy"], *a["ptrs"], a["spec"], a["out"])

    def spec_with(**fields):
        s = make_spec(ALL, ("mean",) * 8)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return s

    try:
        assert call() == 0
        dev.wait()
        assert not np.array_equal(out.to_host(), sentinel)
        out.copy_from_host(sentinel)
        refused = [dict(null_spec=True), dict(out=None)]
        for k in range(4):
            ptrs = [C.c_void_p(x.ptr) for x in arrays]
            ptrs[k] = None
            refused.append(dict(ptrs=ptrs))
        refused += [dict(fx=0), dict(fy=0), dict(fx=-1), dict(nx=0), dict(ny=0), dict(g=-1), dict(pitch=nx + 2 * g - 1),
                    dict(nx=1 << 31)]
        for kw in refused:
            assert call(**kw) == 1, kw
        specs = [dict(nq=0), dict(nq=9), dict(nq=-1), dict(quantity=(3, 8)), dict(quantity=(0, -1)), dict(reduce=(7, 3)),
                 dict(reduce=(0, -1)), dict(eos=2), dict(eos=-1), dict(neighbours=16), dict(neighbours=-1)]
        for name in ("dx", "dy"):
            specs += [{name: 0.0}, {name: -0.5}, {name: float("nan")}, {name: float("inf")}]
        for fields in specs:
            assert call(spec_with(**fields)) == 1, fields
            assert b"" != L.armon_hip_last_error()
        # a flagged side needs a ghost layer
        bare = [dev.from_host(a.ravel()) for a in state]
        try:
            for nb in (1, 2, 4, 8, 15):
                assert call(spec_with(neighbours=nb), g=0, pitch=nx, ptrs=[C.c_void_p(x.ptr) for x in bare]) == 1, nb
            assert call(g=0, pitch=nx, ptrs=[C.c_void_p(x.ptr) for x in bare]) == 0
            dev.wait()
            out.copy_from_host(sentinel)
        finally:
            for a in bare:
                a.free()
        # fp32 entry point: the same checks (a cell size that is not > 0 once converted is refused too)
        assert L.armon_hip_derive_f32(dev.ctx, pitch, g, nx, ny, 1, 1, *[C.c_void_p(x.ptr) for x in arrays],
                                      C.byref(spec_with(dx=1e-60)), C.c_void_p(out.ptr)) == 1
        assert L.armon_hip_derive_f32(dev.ctx, pitch, g, nx, ny, 1, 1, *[C.c_void_p(x.ptr) for x in arrays],
                                      C.byref(spec_with(nq=9)), C.c_void_p(out.ptr)) == 1
        dev.wait()
        assert np.array_equal(out.to_host(), sentinel)
    finally:
        for a in arrays + [out]:
            a.free()


def test_python_surface_refuses_bad_requests():
    import armon_amd
    grid = run_state("Sod_circ", (257, 130), "float64")
    for args in ((["nope"],), (["rho"], 0), (["rho"], 1, "sum"), ([],), (["rho", "rho"],), (["rho"], 1, {"p": "max"})):
        with pytest.raises(armon_amd.SolverException) as e:
            grid.derive(*args)
        assert e.value.category == "config"
    d = grid.derive("mach", (8, 4), {"mach": "max"})
    assert set(d) == {"mach", "x", "y"} and d["mach"].shape == (33, 33) and d["x"].shape == (33, 33)


# ---- a run is not disturbed, end to end ------------------------------------------------------------------------------------
def test_frames_do_not_disturb_a_run(tmp_path):
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    opts = dict(test="Sedov", N=(64, 64), maxcycle=20, silent=5)
    frames = dict(image_step=3, image_quantity=["grad_rho", "vorticity", "mach"], image_coarsen=2)
    for k, extra in enumerate((dict(), dict(graph_cycles=True))):
        plain = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **opts, **extra))
        shot = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, output_dir=str(tmp_path / f"b{k}"), **opts, **extra, **frames))
        assert shot.cycles == plain.cycles == 20 and shot.final_time == plain.final_time
        assert shot.data.state_digest() == plain.data.state_digest()
        assert len(shot.images) == 6 * 3 and plain.images == [] and all(os.path.exists(p) for p in shot.images)
    digests = []
    for extra in (dict(), dict(output_dir=str(tmp_path / "tiles"), **frames)):
        tg = TileGroup((2, 2), **opts, **extra)
        try:
            stats = tg.run()
            digests.append((stats.cycles, stats.final_time, tg.state_digest(), len(stats.images)))
        finally:
            tg.close()
    assert digests[0][:3] == digests[1][:3]
    assert (digests[0][3], digests[1][3]) == (0, 18)


def test_end_to_end_frames(tmp_path):
    import armon_amd
    from armon_amd import derived
    from armon_amd.io import read_png_gray8
    out = str(tmp_path / "run")
    stats = armon_amd.armon(armon_amd.ArmonParameters(test="Sedov", N=(96, 64), maxcycle=12, image_step=5, image_at_end=True,
                                                      image_quantity=["grad_rho", "vorticity"], image_coarsen=2, output_dir=out,
                                                      silent=5, return_data=True))
    want = [os.path.join(out, f"image_{q}_{c:06d}.png") for c in (5, 10, 12) for q in ("grad_rho", "vorticity")]
    assert stats.images == want and sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in want)
    for p in want:
        assert read_png_gray8(p).shape == (32, 48)
    planes = stats.data.derive(["grad_rho", "vorticity"], 2, {"grad_rho": "max"})
    assert planes["grad_rho"].shape == (32, 48)
    assert np.array_equal(read_png_gray8(want[-2]), derived.render(planes["grad_rho"], transfer="schlieren"))
    assert np.array_equal(read_png_gray8(want[-1]), derived.render(planes["vorticity"]))
    assert len(np.unique(read_png_gray8(want[-2]))) > 4                       # a picture, not a blank sheet
