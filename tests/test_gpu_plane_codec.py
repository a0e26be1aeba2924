"""armon_hip_plane_encode / armon_hip_plane_decode on the GPU against the codec restated from its specification
(tests/xorplane_restated.py; never armon.jl_amd/plane_codec.py): the bytes of every chunk, its size, the bytes it must leave
alone, the full and the sub-window decode. Everything here is exact: the codec is lossless, so "equals" means every bit.
No test feeds the decoder an inconsistent stream: the host check (plane_codec.check_chunk) owns that."""
import ctypes as C

import numpy as np
import pytest

import xorplane_restated as xr

pytestmark = pytest.mark.gpu

COLS = (1, 63, 64, 65, 100, 128, 257)
ROWS = (1, 15, 16, 17, 52)
POISON = 0xA5


@pytest.fixture(scope="module")
def dev():
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.wait()
    d.close()


@pytest.fixture(scope="module")
def sedov():
    """rho, u, v, E of Sedov 100 x 76 after 13 cycles, per data type: a state no oracle had a hand in."""
    import armon_amd
    out = {}
    for dtype in ("float64", "float32"):
        stats = armon_amd.armon(armon_amd.ArmonParameters(test="Sedov", N=(100, 76), maxcycle=13, data_type=dtype, silent=5,
                                                          return_data=True))
        grid = stats.data
        host = grid.device_to_host(("rho", "u", "v", "E"))
        out[dtype] = [grid.real_view(host[f]).copy() for f in ("rho", "u", "v", "E")]
    return out


def fn(dev, name, dtype):
    return getattr(dev._L, "armon_hip_" + name + ("_f32" if np.dtype(dtype) == np.float32 else ""))


def ok(dev, rc):
    assert rc == 0, dev._L.armon_hip_last_error()


def encode(dev, planes, slack=64):
    """``planes`` [nplanes][R][C] through armon_hip_plane_encode into a poisoned buffer → (the bytes of every plane's
    capacity, the sizes)."""
    planes = np.ascontiguousarray(planes)
    nplanes, R, C_ = planes.shape
    item = planes.dtype.itemsize
    bound = dev._L.armon_hip_plane_encode_bound(item, R, C_)
    assert bound == xr.shape_of(R, C_, item)[3]
    cap = bound + slack
    src, out, sizes = dev.from_host(planes.reshape(-1)), dev.empty(nplanes * cap, np.uint8), dev.zeros(8, np.uint64)
    try:
        out.fill_bytes(POISON)
        ok(dev, fn(dev, "plane_encode", planes.dtype)(dev.ctx, C.c_void_p(src.ptr), nplanes, R, C_, C.c_void_p(out.ptr), cap,
                                                      C.c_void_p(sizes.ptr)))
        dev.wait()
        return out.to_host().reshape(nplanes, cap), [int(v) for v in sizes.to_host()[:nplanes]]
    finally:
        for a in (src, out, sizes):
            a.free()


def decode(dev, chunk, R, C_, dtype, window=None):
    """The sub-window (col0, row0, snx, sny) of the chunk (default: all of it) → array [sny][snx], poisoned before."""
    col0, row0, snx, sny = window or (0, 0, C_, R)
    src, out, status = dev.from_host(np.frombuffer(chunk, dtype=np.uint8)), dev.empty(snx * sny, dtype), dev.zeros(2, np.uint32)
    try:
        out.fill_bytes(POISON)
        ok(dev, fn(dev, "plane_decode", dtype)(dev.ctx, C.c_void_p(src.ptr), len(chunk), R, C_, col0, row0, snx, sny,
                                               C.c_void_p(out.ptr), C.c_void_p(status.ptr)))
        dev.wait()
        assert status.to_host()[0] == 0
        return out.to_host().reshape(sny, snx)
    finally:
        for a in (src, out, status):
            a.free()


def contents(sedov, dtype, nplanes, R, C_):
    tiled = [np.tile(p, (-(-R // 76), -(-C_ // 100)))[:R, :C_] for p in sedov[dtype][:nplanes]]
    return {"sedov": np.stack(tiled),
            "constant": np.full((nplanes, R, C_), 1.0 / 3.0, dtype=dtype),
            "random": np.stack([xr.random_bits(dtype, (R, C_), 31 * R + C_ + q) for q in range(nplanes)]),
            "special": np.stack([xr.special_values(dtype, (R, C_), 17 * R + C_ + q) for q in range(nplanes)])}


def check_encode(dev, planes, what):
    """Every plane's chunk equals the restated encoder's bytes, the size is reported, nothing after it is touched → chunks."""
    got, sizes = encode(dev, planes)
    chunks = []
    for q, plane in enumerate(planes):
        want, _ = xr.encode_fast(plane)
        assert sizes[q] == len(want), (what, q)
        assert got[q, :sizes[q]].tobytes() == want, (what, q)
        assert (got[q, sizes[q]:] == POISON).all(), (what, q)
        chunks.append(want)
    return chunks


@pytest.mark.parametrize("nplanes", [1, 4])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_encode_and_decode(dev, sedov, dtype, nplanes):
    item = np.dtype(dtype).itemsize
    for R in ROWS:
        for C_ in COLS:
            G, n, table, bound = xr.shape_of(R, C_, item)
            for name, planes in contents(sedov, dtype, nplanes, R, C_).items():
                chunks = check_encode(dev, planes, (name, R, C_))
                if name == "constant":
                    assert all(len(c) == 2 * table for c in chunks)
                if name == "random" and C_ % 64 == 0:
                    assert all(len(c) == bound for c in chunks), (R, C_)      # every bit-plane of every group is hit
                q = nplanes - 1                                               # (the decoder takes one chunk at a time)
                assert decode(dev, chunks[q], R, C_, dtype).tobytes() == planes[q].tobytes(), (name, R, C_)


WINDOWS = ((37, 21, 40, 30), (0, 0, 100, 76), (63, 15, 2, 2), (64, 16, 1, 1), (99, 75, 1, 1), (0, 31, 100, 2), (50, 0, 1, 76),
           (1, 17, 98, 14), (60, 47, 40, 29))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sub_window_decodes(dev, sedov, dtype):
    """Windows of the 100 x 76 chunk that cross group (64 columns) and row-block (16 rows) edges, start inside a row block,
    and a single cell: each equals the slice, and a decode starts at the first row of the row block that holds its first row."""
    for name, plane in (("sedov", sedov[dtype][3]), ("special", xr.special_values(dtype, (76, 100), 9))):
        chunk, _ = xr.encode_fast(plane)
        for col0, row0, snx, sny in WINDOWS:
            got = decode(dev, chunk, 76, 100, dtype, (col0, row0, snx, sny))
            assert got.tobytes() == np.ascontiguousarray(plane[row0:row0 + sny, col0:col0 + snx]).tobytes(), (name, col0, row0, snx, sny)


def test_one_tall_chunk(dev):
    """65541 rows x 3 columns: more groups than a launch grid's y extent had rows, one group per row."""
    R, C_ = 65541, 3
    rng = np.random.default_rng(4)
    plane = np.cumsum(rng.integers(-2, 3, size=(R, C_)), axis=0).astype(np.float64) * 0.125
    plane[40000:40010] = xr.special_values("float64", (10, C_), 1)
    (chunk,) = check_encode(dev, plane[None], "tall")
    assert decode(dev, chunk, R, C_, "float64").tobytes() == plane.tobytes()
    got = decode(dev, chunk, R, C_, "float64", (1, 65530, 2, 11))
    assert got.tobytes() == np.ascontiguousarray(plane[65530:, 1:]).tobytes()


def test_argument_refusals(dev):
    """ARMON_ERR_INVALID_ARG, decided on the host: nothing is launched, so the poisoned buffers stay as they are."""
    L = dev._L
    R, C_ = 17, 65
    bound = L.armon_hip_plane_encode_bound(8, R, C_)
    src, out, sizes = dev.zeros(R * C_, np.float64), dev.empty(bound + 8, np.uint8), dev.empty(8, np.uint64)
    dense, status = dev.empty(R * C_, np.float64), dev.zeros(2, np.uint32)
    try:
        out.fill_bytes(POISON)
        sizes.fill_bytes(POISON)
        dense.fill_bytes(POISON)
        enc = lambda ctx=dev.ctx, s=src.ptr, np_=1, r=R, c=C_, o=out.ptr, cap=bound, z=sizes.ptr: L.armon_hip_plane_encode(
            ctx, C.c_void_p(s) if s else None, np_, r, c, C.c_void_p(o) if o else None, cap, C.c_void_p(z) if z else None)
        for bad in (dict(ctx=None), dict(s=0), dict(o=0), dict(z=0), dict(np_=0), dict(np_=9), dict(r=0), dict(c=0), dict(r=-3),
                    dict(cap=bound - 8), dict(cap=bound + 4), dict(cap=0)):
            assert enc(**bad) == 1, bad
        dec = lambda ctx=dev.ctx, ch=out.ptr, nb=bound, r=R, c=C_, w=(0, 0, C_, R), o=dense.ptr, st=status.ptr: L.armon_hip_plane_decode(
            ctx, C.c_void_p(ch) if ch else None, nb, r, c, *w, C.c_void_p(o) if o else None, C.c_void_p(st) if st else None)
        tables = 2 * xr.shape_of(R, C_, 8)[2]
        for bad in (dict(ctx=None), dict(ch=0), dict(o=0), dict(st=0), dict(r=0), dict(c=0), dict(nb=tables - 8), dict(w=(0, 0, 0, 1)),
                    dict(w=(0, 0, 1, 0)), dict(w=(-1, 0, 2, 2)), dict(w=(0, -1, 2, 2)), dict(w=(1, 0, C_, 1)), dict(w=(0, 1, 1, R)),
                    dict(w=(C_, 0, 1, 1)), dict(w=(0, R, 1, 1))):
            assert dec(**bad) == 1, bad
        dev.wait()
        assert (out.to_host() == POISON).all() and (dense.to_host().view(np.uint8) == POISON).all()
        assert (sizes.to_host().view(np.uint8) == POISON).all() and status.to_host()[0] == 0
    finally:
        for a in (src, out, sizes, dense, status):
            a.free()
