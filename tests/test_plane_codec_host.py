"""The lossless plane codec of packed checkpoints and file version 2, the parts that need no GPU: the numpy reference
(armon.jl_amd/plane_codec.py) against the codec restated from its specification (tests/xorplane_restated.py), the chunk and
index checks, and ``checkpoint.expand`` on a file assembled here by hand."""
import json
import struct

import numpy as np
import pytest

from armon_amd import checkpoint as ck
from armon_amd import plane_codec as pc
from armon_amd._lib import SolverException
from armon_amd.parameters import ArmonParameters

import xorplane_restated as xr

COLS = (1, 63, 64, 65, 100)
ROWS = (1, 15, 16, 17, 33)
DTYPES = ("float64", "float32")


def test_the_pinned_example():
    data = pc.encode_reference(np.array([[1.0, 1.0, 2.0]]))
    want = bytes.fromhex("000000000000f03f" "000000000000f07f") + (4).to_bytes(8, "little") * 11
    assert len(want) == 104 and data == want
    assert int.from_bytes(data[8:16], "little") == 0x7ff0000000000000
    assert xr.encode(np.array([[1.0, 1.0, 2.0]]))[0] == want
    assert pc.decode_reference(data, 1, 3, "float64").tobytes() == np.array([[1.0, 1.0, 2.0]]).tobytes()
    assert pc.chunk_size(data, 1, 3, 8) == 104 == pc.chunk_size(np.array([0x7ff0000000000000], dtype=np.uint64))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", ROWS)
def test_round_trips(R, dtype):
    item = np.dtype(dtype).itemsize
    for C in COLS:
        G, n, table, bound = xr.shape_of(R, C, item)
        assert pc.groups(R, C) == (G, n) and pc.table_bytes(R, C, item) == table and pc.bound(R, C, item) == bound
        for name, plane in (("special", xr.special_values(dtype, (R, C), 100 * R + C)),
                            ("constant", np.full((R, C), -3.25, dtype=dtype)),
                            ("random", xr.random_bits(dtype, (R, C), 7 * R + C))):
            data = pc.encode_reference(plane)
            want, masks = xr.encode(plane)
            assert data == want, (name, R, C)
            assert pc.chunk_size(data, R, C, item) == len(data) == pc.chunk_size(np.array(masks, dtype=xr.bit_patterns(plane).dtype))
            pc.check_chunk(data, R, C, item)
            back = pc.decode_reference(data, R, C, dtype)
            assert back.dtype == np.dtype(dtype) and back.shape == (R, C)
            assert back.tobytes() == plane.tobytes(), (name, R, C)      # NaN payloads, -0.0: every bit
            assert len(data) <= bound
            if name == "constant":
                assert len(data) == 2 * table
            if name == "random" and all(m == (1 << 8 * item) - 1 for m in masks):
                assert len(data) == bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_random_bits_reach_the_bound(dtype):
    """Whole groups of random bits hit every bit-plane: the chunk is exactly as long as the bound."""
    item = np.dtype(dtype).itemsize
    plane = xr.random_bits(dtype, (17, 128), 3)
    data = pc.encode_reference(plane)
    assert len(data) == pc.bound(17, 128, item) == 2 * xr.pad8(34 * item) + 8 * 8 * item * 34
    assert pc.decode_reference(data, 17, 128, dtype).tobytes() == plane.tobytes()


def test_check_chunk_rejects_a_damaged_chunk():
    plane = xr.special_values("float64", (17, 65), 5)
    data = pc.encode_reference(plane)
    n, table = 34, 34 * 8
    pc.check_chunk(data, 17, 65, 8)
    flipped = bytearray(data)
    flipped[table + 3] ^= 0x10                                          # one bit of the mask of group 0
    for bad in (bytes(flipped), data[:-8], data + bytes(8), data[:2 * table - 1]):
        with pytest.raises(ValueError):
            pc.check_chunk(bad, 17, 65, 8)
        with pytest.raises(ValueError):
            pc.decode_reference(bad, 17, 65, "float64")
    f32 = pc.encode_reference(xr.special_values("float32", (17, 65), 5))
    with pytest.raises(ValueError):
        pc.check_chunk(f32, 17, 65, 8)


# ---- file version 2, assembled by hand ---------------------------------------------------------------------------------------
NX, NY = 100, 20
WINDOWS = ((0, 0, 60, 17), (0, 17, 60, 3), (60, 0, 40, 20))             # two "tiles", the first saved in two bands


def planes_of(dtype):
    rng = np.random.default_rng(11)
    smooth = np.add.outer(np.arange(NY), np.arange(NX)).astype(dtype)
    return [np.ones((NY, NX), dtype=dtype), smooth, rng.standard_normal((NY, NX)).astype(dtype), xr.special_values(dtype, (NY, NX), 2)]


def preamble(version, header):
    text = json.dumps(header, sort_keys=True).encode()
    return b"ARMONCKP" + struct.pack("<II", version, len(text)) + text + b" " * (4096 - len(text))


def assemble(dtype, raw_planes=(2,)):
    """→ (the bytes of the version-2 file, those of the version-1 file of the same state, the index records)."""
    params = ArmonParameters(test="Sedov", N=(NX, NY), data_type=dtype)
    planes = planes_of(dtype)
    header = dict(ck.bit_options(params))
    header.update(version=1, planes=["rho", "u", "v", "E"], cycle=3, time=ck.hexfloat(0.25), current_dt=ck.hexfloat(1e-3),
                  next_cycle_dt=ck.hexfloat(2e-3), pending_dt=None, digests={f: f"{k:016x}" for k, f in enumerate(("rho", "u", "v", "E"))})
    body, records, at = b"", [], 16 + 4096
    for col0, row0, wnx, wny in WINDOWS:
        for q, plane in enumerate(planes):
            cut = np.ascontiguousarray(plane[row0:row0 + wny, col0:col0 + wnx])
            chunk = cut.tobytes() if q in raw_planes else xr.encode(cut)[0]
            records.append([q, 0 if q in raw_planes else 1, col0, row0, wnx, wny, at, len(chunk)])
            chunk += bytes(-len(chunk) % 8)
            body += chunk
            at += len(chunk)
    packed = dict(header, codec="xorplane16", index_offset=at, index_count=len(records))
    v1 = preamble(1, header) + b"".join(p.tobytes() for p in planes)
    return preamble(2, packed), body, records, v1, packed


def put(path, pre, body, records):
    path.write_bytes(pre + body + np.array(records, dtype="<u8").tobytes())
    return path


@pytest.mark.parametrize("dtype", DTYPES)
def test_expand_of_a_hand_assembled_file(tmp_path, dtype):
    pre, body, records, v1, packed = assemble(dtype)
    src = put(tmp_path / "packed.ckpt", pre, body, records)
    header = ck.read_header(src)
    assert header == packed and ck.is_packed(header)
    bands = ck.read_index(str(src), header)
    assert [w for w, _ in bands] == list(WINDOWS) and all(sorted(recs) == [0, 1, 2, 3] for _, recs in bands)
    plain = ck.expand(src, tmp_path / "plain.ckpt")
    assert (tmp_path / "plain.ckpt").read_bytes() == v1
    assert plain == {k: v for k, v in packed.items() if k not in ("codec", "index_offset", "index_count")}
    assert ck.read_header(tmp_path / "plain.ckpt") == plain and not ck.is_packed(plain)
    with pytest.raises(SolverException) as e:
        ck.expand(tmp_path / "plain.ckpt", tmp_path / "again.ckpt")      # not a packed file
    assert e.value.category == "io"


def io_error(tmp_path, src, says=""):
    with pytest.raises(SolverException) as e:
        ck.expand(src, tmp_path / "out.ckpt")
    assert e.value.category == "io" and str(src) in str(e.value) and says in str(e.value), e.value
    assert not (tmp_path / "out.ckpt").exists() and not (tmp_path / "out.ckpt.tmp").exists()


def test_a_damaged_index_is_an_io_error(tmp_path):
    pre, body, records, _, packed = assemble("float64")
    item = 8

    def changed(i, **fields):
        out = [list(r) for r in records]
        for k, v in fields.items():
            out[i][("plane", "codec", "col0", "row0", "wnx", "wny", "offset", "bytes").index(k)] = v
        return out
    raw = [i for i, r in enumerate(records) if r[1] == 0]
    i = raw[0]                                                           # a raw chunk of the first band: 60 x 17
    cases = {
        f"offsets {records[i - 1][6]} and {records[i - 1][6]} overlap": changed(i, offset=records[i - 1][6]),         # two chunks on the same bytes
        "plane v overlap at cell (59, 0)": changed(raw[2], col0=59),                   # the second tile's window, one column left
        "plane v leave a hole at cell (59, 0)": changed(i, wnx=59, bytes=59 * 17 * item),
        "leaves the chunk area": changed(i, offset=packed["index_offset"] - 8),        # a record past the end
        "leaves the domain": changed(i, row0=4),
        "codec 2": changed(i, codec=2),
        "plane 4": changed(i, plane=4),
        "do not share its window": changed(i, wny=16, bytes=60 * 16 * item) + [[2, 0, 0, 16, 60, 1, records[i][6] + 60 * 16 * item, 60 * item]],
        "an encoded chunk of 60 x 17": changed(0, bytes=8),
    }
    for says, recs in cases.items():
        header = dict(packed, index_count=len(recs))
        src = put(tmp_path / "bad.ckpt", preamble(2, header), body, recs)
        io_error(tmp_path, src, says)
    # the file's length is the index's end, no more and no less
    good = pre + body + np.array(records, dtype="<u8").tobytes()
    for name, data in (("long", good + bytes(8)), ("short", good[:-8])):
        src = tmp_path / "bad.ckpt"
        src.write_bytes(data)
        io_error(tmp_path, src, "truncated checkpoint")
    # a mask bit flipped inside an encoded chunk: its table no longer gives the length the index holds
    q, _, col0, row0, wnx, wny, off, nbytes = records[1]
    flipped = bytearray(good)
    flipped[off + pc.table_bytes(wny, wnx, item) + 2] ^= 0x40
    src = tmp_path / "bad.ckpt"
    src.write_bytes(bytes(flipped))
    io_error(tmp_path, src, "its mask table asks for")
    # header keys of a packed file that do not make sense
    for change in (dict(codec="zip"), dict(index_offset=packed["index_offset"] + 4), dict(index_count=0), dict(index_offset="12")):
        src = put(tmp_path / "bad.ckpt", preamble(2, dict(packed, **change)), body, records)
        io_error(tmp_path, src)


def test_the_option():
    assert ArmonParameters(test="Sod", N=(8, 8)).checkpoint_compress is False
    assert ArmonParameters(test="Sod", N=(8, 8), checkpoint_compress=True).checkpoint_compress is True
    with pytest.raises(SolverException) as e:
        ArmonParameters(test="Sod", N=(8, 8), checkpoint_compress="yes")
    assert e.value.category == "config"
    assert ck.VERSION == 1


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    """Argument errors are decided on the host before any launch: a NULL context is one of them."""
    import ctypes as C
    import armon_amd
    L = armon_amd.lib()
    assert L.armon_hip_plane_encode_bound(8, 1, 3) == 2 * 8 + 8 * 64 == pc.bound(1, 3, 8)
    assert L.armon_hip_plane_encode_bound(4, 33, 100) == pc.bound(33, 100, 4) == xr.shape_of(33, 100, 4)[3]
    for bad in ((2, 4, 4), (8, 0, 4), (8, 4, 0), (8, -1, 4)):
        assert L.armon_hip_plane_encode_bound(*bad) == 0
    for fn in (L.armon_hip_plane_encode, L.armon_hip_plane_encode_f32):
        assert fn(None, C.c_void_p(8), 1, 4, 4, C.c_void_p(8), 1 << 20, C.c_void_p(8)) == 1
    for fn in (L.armon_hip_plane_decode, L.armon_hip_plane_decode_f32):
        assert fn(None, C.c_void_p(8), 1 << 20, 4, 4, 0, 0, 4, 4, C.c_void_p(8), C.c_void_p(8)) == 1
