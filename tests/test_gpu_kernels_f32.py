"""GPU parity of every staged `_f32` entry point against the fp32 CPU oracle, through the C ABI, and of the forms, layouts
and grid-stride loops that tests/test_gpu_kernels.py (fp64, ghost width 4) never selects.

Bar: BIT-EXACT against the oracle of the same precision, on EVERY array handed to the kernel — outputs and inputs, ghost cells
included — so that a cell written outside the range fails like a wrong cell inside it. The fp32 x forms of acoustic_GAD and
advection_second_order lay a wave over 48 results + 8 + 8 halo lanes and shift their strips by the position of the first cell
within its 16-float sector: every one of the 16 positions, and rows on either side of a wave (48), a workgroup (192) and two
workgroups, are run here.
"""
import ctypes as C

import numpy as np
import pytest

import staged_reference as S
from oracle import oracle as O
from staged_reference import Precision, as_tuple, conv

pytestmark = pytest.mark.gpu

SHAPES = [(37, 29), (128, 3), (5, 70), (257, 64)]
GHOSTS = [4, 5]
F32, F64 = np.float32, np.float64
BOTH = [pytest.param(F32, id="f32"), pytest.param(F64, id="f64")]
ADV = ("us", "rho", "u", "v", "E", "work_1", "work_2", "work_3", "work_4")
FLUX = ("us", "ps", "rho", "u", "p", "c")
BCV = ("rho", "u", "v", "p", "c", "g", "E")


@pytest.fixture(scope="module")
def dev():
    import armon_amd
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def L():
    import armon_amd
    return armon_amd.lib()


def check_kernel(P, dev, f, name, r, pre, arrays, post=(), pitch=None, lead=0):
    """Run ``name`` of the oracle on a copy of the host fields ``f`` and of the library on an upload of them — ``lead``
    elements into each allocation — and compare EVERY field in full."""
    want = {k: a.copy() for k, a in f.items()}
    size = P.dtype().itemsize
    d = {k: dev.from_host(np.concatenate([np.zeros(lead, a.dtype), a])) for k, a in f.items()}
    P.ref(name)(r, *pre, *(O.ptr(want[k]) for k in arrays), *post)
    rc = P.hip(name)(dev.ctx, conv(r), *pre, *(C.c_void_p(d[k].ptr + lead * size) for k in arrays), *post)
    assert rc == 0, (name, P.L.armon_hip_last_error())
    for k in f:
        got = d[k].to_host()
        assert not got[:lead].any(), f"{name}: {k}: written below the array"
        S.assert_bits_equal(got[lead:], want[k], f"{name}: {k}", pitch or r.col_step, as_tuple(r))
    return want


def step_ranges(nx, ny, g, axis, w=2):
    """The ranges of one sweep (ref src/parameters.jl:992-1025), as tests/test_gpu_kernels.ranges_for at any ghost width."""
    dr = lambda bl, tr: O.domain_range(nx, ny, g, bl, tr)
    if axis == 0:
        return dict(s=1, fluxes=dr((-w, 0), (w + 1, 0)), cell_update=dr((-w, 0), (w, 0)), advection=dr((0, 0), (1, 0)),
                    real=dr((0, 0), (0, 0)))
    return dict(s=nx + 2 * g, fluxes=dr((0, -w), (0, w + 1)), cell_update=dr((0, -w), (0, w)), advection=dr((0, 0), (0, 1)),
                real=dr((0, 0), (0, 0)))


def along(names, axis):
    """The array list of a kernel with the velocity along the sweep axis in place of ``u``."""
    return tuple(("u" if axis == 0 else "v") if k == "u" else k for k in names)


# ---- every `_f32` kernel, at the shapes, axes and (two) ghost widths of the fp64 file --------------------------------------
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_perfect_gas_EOS_f32(dev, L, shape, g):
    nx, ny = shape
    P = Precision(L, F32)
    check_kernel(P, dev, S.rand_fields(nx, ny, g, F32, 1), "perfect_gas_EOS", O.domain_range(nx, ny, g), (1.4,),
                 ("rho", "E", "u", "v", "p", "c", "g"))


@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bizarrium_EOS_f32(dev, L, shape, g):
    nx, ny = shape
    P = Precision(L, F32)
    check_kernel(P, dev, S.rand_fields(nx, ny, g, F32, 2, eos="bizarrium"), "bizarrium_EOS", O.domain_range(nx, ny, g), (),
                 ("rho", "u", "v", "E", "p", "c", "g"))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_acoustic_f32(dev, L, shape, g, axis):
    nx, ny = shape
    R = step_ranges(nx, ny, g, axis)
    check_kernel(Precision(L, F32), dev, S.rand_fields(nx, ny, g, F32, 3), "acoustic", R["fluxes"], (R["s"],), along(FLUX, axis))


@pytest.mark.parametrize("limiter", [0, 1, 2])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_acoustic_GAD_f32(dev, L, shape, g, axis, limiter):
    nx, ny = shape
    R = step_ranges(nx, ny, g, axis)
    check_kernel(Precision(L, F32), dev, S.rand_fields(nx, ny, g, F32, 4), "acoustic_GAD", R["fluxes"],
                 (R["s"], 1e-3, 1.0 / nx), along(FLUX, axis), (limiter,))


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cell_update_f32(dev, L, shape, g, axis):
    nx, ny = shape
    R = step_ranges(nx, ny, g, axis)
    check_kernel(Precision(L, F32), dev, S.rand_fields(nx, ny, g, F32, 5), "cell_update", R["cell_update"],
                 (R["s"], 1.0 / nx, 1e-3), along(("us", "ps", "rho", "u", "E"), axis))


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_advection_f32(dev, L, shape, g, axis, order):
    nx, ny = shape
    R = step_ranges(nx, ny, g, axis)
    f = S.rand_fields(nx, ny, g, F32, 6)
    if order == 1:
        check_kernel(Precision(L, F32), dev, f, "advection_first_order", R["advection"], (R["s"], 1e-3), ADV)
    else:
        check_kernel(Precision(L, F32), dev, f, "advection_second_order", R["advection"], (R["s"], 1.0 / nx, 1e-3), ADV)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_euler_projection_f32(dev, L, shape, g, axis):
    nx, ny = shape
    R = step_ranges(nx, ny, g, axis)
    check_kernel(Precision(L, F32), dev, S.rand_fields(nx, ny, g, F32, 7), "euler_projection", R["real"],
                 (R["s"], 1.0 / nx, 1e-3), ADV)


def side_geometry(nx, ny, g, side):
    from armon_amd.blocking import BlockSize, Side, axis_of
    bs = BlockSize((nx + 2 * g, ny + 2 * g), g)
    sd = Side(side)
    low = sd in (Side.Left, Side.Bottom)
    incr = bs.stride_along(axis_of(sd)) * (-1 if low else 1)
    factors = (-1., 1.) if sd in (Side.Left, Side.Right) else (1., -1.)
    return bs, sd, incr, factors


def oracle_range(r):
    return O.Range(r.col_start, r.col_step, r.col_len, r.row_start, r.row_len)


@pytest.mark.parametrize("side", [1, 2, 3, 4])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_boundary_conditions_f32(dev, L, shape, g, side):
    nx, ny = shape
    bs, sd, incr, (uf, vf) = side_geometry(nx, ny, g, side)
    r = oracle_range(bs.border_domain(sd).to_c())
    check_kernel(Precision(L, F32), dev, S.rand_fields(nx, ny, g, F32, 8), "boundary_conditions", r, (incr, g, uf, vf), BCV,
                 pitch=nx + 2 * g)


@pytest.mark.parametrize("test", ["Sod", "Sod_circ", "Bizarrium", "Sedov", "DebugIndexes"])
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_init_test_f32(dev, L, shape, g, test):
    """The whole block, as the solver initialises it, and a part of it on arrays that hold something else: all 16 arrays in
    full. The block is a tile of a larger grid (a non-zero global position), so that the global index matters."""
    from armon_amd._lib import BlockDataPtrs
    nx, ny = shape
    P = Precision(L, F32)
    T = P.dtype
    n = (nx + 2 * g) * (ny + 2 * g)
    rng = np.random.default_rng(12)
    start = {k: rng.uniform(-3, 3, n).astype(F32) for k in O.FIELDS}
    domain = O.DEFAULTS[test]["domain"]
    gN = (C.c_int64 * 2)(nx + 7, ny + 9)
    gpos = (C.c_int64 * 2)(3, 5)
    dX = (P.real * 2)(float(T(domain[0]) / T(nx + 7)), float(T(domain[1]) / T(ny + 9)))
    origin = (P.real * 2)(*O.DEFAULTS[test]["origin"])
    sedov_r = float(T(np.hypot(dX[0], dX[1]) / np.sqrt(2.)))           # ref src/tests.jl:15-19
    for r in (O.domain_range(nx, ny, g, (-g, -g), (g, g)), O.domain_range(nx, ny, g, (-1, -2), (2, 1))):
        want = {k: a.copy() for k, a in start.items()}
        d = {k: dev.from_host(a) for k, a in start.items()}
        bd_h = O.block_data(want)
        bd_d = BlockDataPtrs(*(d[k].ptr for k in O.FIELDS))
        P.ref("init_test")(r, O.TESTS[test], nx + 2 * g, ny + 2 * g, g, C.byref(gpos), C.byref(gN), C.byref(origin), C.byref(dX),
                           sedov_r, C.byref(bd_h))
        assert P.hip("init_test")(dev.ctx, conv(r), O.TESTS[test], nx + 2 * g, ny + 2 * g, g, C.byref(gpos), C.byref(gN),
                                  C.byref(origin), C.byref(dX), sedov_r, C.byref(bd_d)) == 0, L.armon_hip_last_error()
        for k in O.FIELDS:
            S.assert_bits_equal(d[k].to_host(), want[k], f"init_test {test}: {k}", nx + 2 * g, as_tuple(r))


# ---- the fp32 x forms: 16 strip origins, rows around one wave's, one workgroup's and two workgroups' results --------------
def x_strip_case(length, rows, shift):
    """A block of ghost width 2 whose rows hold ``length`` results from cell 2 + shift on: two stencil cells on the left, up to
    15 of shift, two stencil cells and one spare on the right."""
    nx, ny, g = length + 16, rows, 2
    pitch = nx + 2 * g
    r = O.Range(g * pitch, pitch, rows, 2 + shift, length)
    assert r.row_start - 2 >= 0 and r.row_start + length - 1 + 2 < pitch
    return nx, ny, g, r


@pytest.mark.parametrize("rows", [1, 4, 5])
@pytest.mark.parametrize("length", [47, 48, 49, 191, 193, 400])
def test_f32_x_forms_at_every_strip_origin(dev, L, length, rows):
    """47 / 48 / 49 results: a partial wave, a full one, a full one + 1; 191 / 193: a partial workgroup and one + 1;
    400: more than two workgroups per row. 1, 4 and 5 rows: blockIdx.y walks rows."""
    P = Precision(L, F32)
    origins = set()
    for shift in range(16):
        nx, ny, g, r = x_strip_case(length, rows, shift)
        origins.add((r.col_start + r.row_start) & 15)
        f = S.rand_fields(nx, ny, g, F32, 100 + shift)
        check_kernel(P, dev, f, "acoustic_GAD", r, (1, 1e-3, 1.0 / length), FLUX, (shift % 3,))
        check_kernel(P, dev, f, "advection_second_order", r, (1, 1.0 / length, 1e-3), ADV)
    assert origins == set(range(16))


@pytest.mark.parametrize("name", ["acoustic_GAD", "advection_second_order"])
def test_f32_x_forms_on_arrays_four_bytes_into_an_allocation(dev, L, name):
    P = Precision(L, F32)
    nx, ny, g, r = x_strip_case(193, 4, 5)
    f = S.rand_fields(nx, ny, g, F32, 77)
    if name == "acoustic_GAD":
        check_kernel(P, dev, f, name, r, (1, 1e-3, 1.0 / 193), FLUX, (1,), lead=1)
    else:
        check_kernel(P, dev, f, name, r, (1, 1.0 / 193, 1e-3), ADV, lead=1)


@pytest.mark.parametrize("nx,ny,g,lo,hi,axis,limiter,seed", S.draw_range_cases(4242, 40, F32))
def test_f32_flux_kernels_on_drawn_ranges(dev, L, nx, ny, g, lo, hi, axis, limiter, seed):
    """test_gpu_kernels.test_flux_kernels_on_random_ranges in fp32, at ghost widths 2 .. 6, with cases that between them start
    on every position of a sector and have rows on both sides of 48, 192 and 384 results (asserted by the generator)."""
    P = Precision(L, F32)
    f = S.rand_fields(nx, ny, g, F32, seed)
    bl, tr = ((lo, 0), (hi, 0)) if axis == 0 else ((0, lo), (0, hi))
    r = O.domain_range(nx, ny, g, bl, tr)
    assert as_tuple(r) == S.range_of(nx, ny, g, lo, hi, axis)
    s = 1 if axis == 0 else nx + 2 * g
    dt, dx = 1e-3, 1.0 / max(nx, ny)
    check_kernel(P, dev, f, "acoustic_GAD", r, (s, dt, dx), along(FLUX, axis), (limiter,))
    check_kernel(P, dev, f, "advection_second_order", r, (s, dx, dt), ADV)


# ---- form 0: the reference's own shape of acoustic_GAD and advection_second_order ------------------------------------------
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", [(37, 29), (257, 64), (300, 7)])
def test_reference_shape_form_on_one_row_and_on_every_other_row(dev, L, shape, g, dtype):
    """A sweep along y over ONE row of cells (col_len == 1), and over every other row (col_step = 2 · pitch with s = pitch):
    neither is the march along y (s == col_step, several rows) nor lanes along the sweep (s == 1)."""
    nx, ny = shape
    P = Precision(L, dtype)
    pitch = nx + 2 * g
    f = S.rand_fields(nx, ny, g, dtype, 21)
    dt, dx = 1e-3, 1.0 / ny
    one_row = O.domain_range(nx, ny, g, (0, ny // 2), (0, ny // 2 + 1 - ny))
    assert one_row.col_len == 1 and one_row.row_len == nx
    rows = list(range(2, ny - 2, 2))                      # real rows 2, 4, ...: rows r - 2 .. r + 2 are real rows too
    alternate = O.Range((g + 2) * pitch, 2 * pitch, len(rows), g, nx)
    assert len(rows) >= 1 and rows[-1] + 2 <= ny - 1
    for r in (one_row, alternate):
        for limiter in (0, 1, 2):
            check_kernel(P, dev, f, "acoustic_GAD", r, (pitch, dt, dx), along(FLUX, 1), (limiter,), pitch=pitch)
        check_kernel(P, dev, f, "advection_second_order", r, (pitch, dx, dt), ADV, pitch=pitch)


# ---- pack_to_array / unpack_from_array: the layout at other ghost widths, variable counts and face sizes -------------------
def encoded_fields(n, nvars, dtype):
    """Variable v holds v · 2^20 + cell index: every value is exact in fp32 (below 2^24) and tells where it came from."""
    assert n < 2 ** 20 and nvars * 2 ** 20 <= 2 ** 24
    return [(np.arange(n) + v * 2 ** 20).astype(dtype) for v in range(nvars)]


def pointer_table(pointers):
    return (C.c_void_p * len(pointers))(*pointers)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("nvars", [1, 3, 8])
@pytest.mark.parametrize("g", [2, 3, 5, 6])
@pytest.mark.parametrize("shape", [(21, 13), (300, 7), (7, 300)])
def test_pack_unpack_layout(dev, L, shape, g, nvars, dtype):
    """i_arr = ((itr % nghost) · face + itr / nghost) · nvars (ref src/halo_exchange.jl:187-216) mixes the ghost width, the
    face size and the number of variables: all three vary here, over faces of one workgroup and of several, on all four sides."""
    from armon_amd.blocking import BlockSize, Side
    nx, ny = shape
    P = Precision(L, dtype)
    bs = BlockSize((nx + 2 * g, ny + 2 * g), g)
    for sd in Side:
        host = encoded_fields(bs.n_cells, nvars, dtype)
        d = [dev.from_host(a) for a in host]
        face = bs.real_face_size(sd)
        send = oracle_range(bs.border_domain(sd, single_strip=False).to_c())
        recv = oracle_range(bs.ghost_domain(sd, single_strip=False).to_c())
        assert send.col_len * send.row_len == face * g == recv.col_len * recv.row_len
        buf_h = np.full(face * g * nvars, -1, dtype)
        buf_d = dev.from_host(buf_h)
        vars_h, vars_d = pointer_table([a.ctypes.data for a in host]), pointer_table([a.ptr for a in d])
        P.ref("pack_to_array")(send, g, face, O.ptr(buf_h), nvars, vars_h)
        assert P.hip("pack_to_array")(dev.ctx, conv(send), g, face, C.c_void_p(buf_d.ptr), nvars, vars_d) == 0
        S.assert_bits_equal(buf_d.to_host(), buf_h, f"packed buffer, {sd.name}")
        assert len(np.unique(buf_h)) == buf_h.size and buf_h.min() >= 0          # a bijection that fills the buffer
        P.ref("unpack_from_array")(recv, g, face, O.ptr(buf_h), nvars, vars_h)
        assert P.hip("unpack_from_array")(dev.ctx, conv(recv), g, face, C.c_void_p(buf_d.ptr), nvars, vars_d) == 0
        for v in range(nvars):
            S.assert_bits_equal(d[v].to_host(), host[v], f"variable {v} after unpack, {sd.name}", nx + 2 * g, as_tuple(recv))
        S.assert_bits_equal(buf_d.to_host(), buf_h, f"buffer after unpack, {sd.name}")


@pytest.mark.parametrize("dtype", BOTH)
def test_pack_refuses_nine_variables(dev, L, dtype):
    from armon_amd.blocking import BlockSize, Side
    P = Precision(L, dtype)
    bs = BlockSize((21 + 8, 13 + 8), 4)
    a = dev.zeros(bs.n_cells, dtype)
    buf = dev.zeros(13 * 4 * 9, dtype)
    table = pointer_table([a.ptr] * 9)
    send = bs.border_domain(Side.Left, single_strip=False).to_c()
    for name in ("pack_to_array", "unpack_from_array"):
        assert P.hip(name)(dev.ctx, send, 4, 13, C.c_void_p(buf.ptr), 9, table) == 1
        assert b"nvars" in L.armon_hip_last_error()
    assert not a.to_host().any() and not buf.to_host().any()


def test_grid_stride_loops_of_pack_unpack_and_boundary_conditions(dev, L):
    """A bottom face of 600 000 columns, ghost width 4: 2.4 M cells per exchange and 600 000 border cells, both more than the
    n_cu · 8 workgroups of 256 threads that linear_grid launches at most (524 288 threads on 256 CUs) — every thread of
    k_pack and k_boundary_conditions goes round its loop more than once. fp64, 7 variables, index-encoded."""
    from armon_amd.blocking import BlockSize, Side
    nx, ny, g, nvars = 600_000, 1, 4, 7
    P = Precision(L, F64)
    bs = BlockSize((nx + 2 * g, ny + 2 * g), g)
    n = bs.n_cells
    host = [(np.arange(n, dtype=F64) + v * 2. ** 23) for v in range(nvars)]
    d = [dev.from_host(a) for a in host]
    face = bs.real_face_size(Side.Bottom)
    send = oracle_range(bs.border_domain(Side.Bottom, single_strip=False).to_c())
    recv = oracle_range(bs.ghost_domain(Side.Bottom, single_strip=False).to_c())
    assert face == nx and send.col_len * send.row_len == face * g > 256 * 8 * 256
    buf_h = np.full(face * g * nvars, -1.)
    buf_d = dev.from_host(buf_h)
    vars_h, vars_d = pointer_table([a.ctypes.data for a in host]), pointer_table([a.ptr for a in d])
    P.ref("pack_to_array")(send, g, face, O.ptr(buf_h), nvars, vars_h)
    assert P.hip("pack_to_array")(dev.ctx, conv(send), g, face, C.c_void_p(buf_d.ptr), nvars, vars_d) == 0
    S.assert_bits_equal(buf_d.to_host(), buf_h, "packed buffer")
    assert buf_h.min() >= 0
    P.ref("unpack_from_array")(recv, g, face, O.ptr(buf_h), nvars, vars_h)
    assert P.hip("unpack_from_array")(dev.ctx, conv(recv), g, face, C.c_void_p(buf_d.ptr), nvars, vars_d) == 0
    for v in range(nvars):          # before the mirror below overwrites the same ghost rows
        S.assert_bits_equal(d[v].to_host(), host[v], f"variable {v} after unpack", nx + 2 * g, as_tuple(recv))
    border = oracle_range(bs.border_domain(Side.Bottom).to_c())
    assert border.col_len * border.row_len == nx > 256 * 8 * 256
    incr = -(nx + 2 * g)
    P.ref("boundary_conditions")(border, incr, g, 1., -1., *(O.ptr(a) for a in host))
    assert P.hip("boundary_conditions")(dev.ctx, conv(border), incr, g, 1., -1., *(C.c_void_p(a.ptr) for a in d)) == 0
    for v in range(nvars):
        S.assert_bits_equal(d[v].to_host(), host[v], f"variable {v}", nx + 2 * g)
