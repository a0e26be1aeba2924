"""The lossless plane codec "xorplane16" of packed checkpoints, restated in numpy (the device side is csrc/plane_codec.hip;
include/armon_hip.h and DESIGN §4.10 state the format). Host only: the reference the device is tested against, the check of
a chunk before it goes to the device, and what ``checkpoint.expand`` decodes with. No reference counterpart.

A chunk encodes one dense plane ``[R][C]`` of W = 64 or 32 bit elements, ``u`` = their bit patterns:

    t[r][c] = u[r][c] if r % 16 == 0 else u[r][c] ^ u[r-1][c]
    group g = r G + j, G = ceil(C / 64), n = R G;  lane l of group (r, j) = column 64 j + l
    base = t[r][64 j];  res[0] = 0;  res[l] = t[r][64 j + l] ^ t[r][64 j + l - 1] inside the plane, 0 past it
    mask = OR of res;  per set bit k of mask, ascending, one 64-bit word whose bit l is bit k of res[l]

Bytes, little-endian: ``base[n]`` (W/8 bytes each, zero-padded to a multiple of 8), ``mask[n]`` (the same), the words of group
0, 1, ... back to back.
"""
import numpy as np

ROW_BLOCK = 16
LANES = 64
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint64)
_LANE = np.arange(LANES, dtype=np.uint64)


def pad8(nbytes):
    return (int(nbytes) + 7) & ~7


def _uint(itemsize):
    if itemsize not in (4, 8):
        raise ValueError(f"the codec takes elements of 4 or 8 bytes, not {itemsize}")
    return np.dtype("<u8" if itemsize == 8 else "<u4")


def groups(rows, wnx):
    """→ (G, n): groups per row and groups of a ``rows`` x ``wnx`` plane."""
    G = (int(wnx) + LANES - 1) // LANES
    return G, int(rows) * G


def table_bytes(rows, wnx, itemsize):
    return pad8(groups(rows, wnx)[1] * itemsize)


def bound(rows, wnx, itemsize):
    """The largest chunk of this shape: every bit-plane of every group present."""
    return 2 * table_bytes(rows, wnx, itemsize) + 8 * 8 * itemsize * groups(rows, wnx)[1]


def popcount(a):
    """The number of set bits of the whole array → int."""
    return int(_POP8[np.ascontiguousarray(a).view(np.uint8)].sum())


def encode_reference(plane):
    """The chunk of the 2-D float64 / float32 (or uint64 / uint32) array ``plane`` → bytes."""
    plane = np.ascontiguousarray(plane)
    R, C = plane.shape
    if R < 1 or C < 1:
        raise ValueError(f"empty plane {plane.shape}")
    U = _uint(plane.dtype.itemsize)
    W = 8 * U.itemsize
    G, n = groups(R, C)
    u = plane.view(U)
    t = np.zeros((R, G * LANES), dtype=U)
    t[:, :C] = u
    below = np.arange(R) % ROW_BLOCK != 0
    t[below, :C] ^= u[np.flatnonzero(below) - 1]
    res = t.copy()
    res[:, 1:] ^= t[:, :-1]
    res[:, C:] = 0
    res = res.reshape(n, LANES)
    res[:, 0] = 0
    base = t.reshape(n, LANES)[:, 0]
    mask = np.bitwise_or.reduce(res, axis=1)
    words = np.zeros((n, W), dtype="<u8")
    for k in range(W):
        words[:, k] = np.bitwise_or.reduce(((res >> U.type(k)) & U.type(1)).astype(np.uint64) << _LANE, axis=1)
    present = ((mask[:, None] >> np.arange(W, dtype=U)) & U.type(1)).astype(bool)
    table = pad8(n * U.itemsize)
    fill = b"\0" * (table - n * U.itemsize)
    return base.tobytes() + fill + mask.tobytes() + fill + words[present].tobytes()


def _tables(data, rows, wnx, itemsize):
    U = _uint(itemsize)
    n = groups(rows, wnx)[1]
    table = pad8(n * itemsize)
    if len(data) < 2 * table:
        raise ValueError(f"a chunk of {len(data)} bytes cannot hold the tables of {rows} x {wnx} ({2 * table} bytes)")
    buf = np.frombuffer(data, dtype=np.uint8)
    return buf[:n * itemsize].view(U), buf[table:table + n * itemsize].view(U), buf[2 * table:]


def chunk_size(data_or_masks, rows=None, wnx=None, itemsize=None):
    """What a chunk holds, from its mask table: ``chunk_size(masks)`` with the uint64 / uint32 array of the n masks, or
    ``chunk_size(data, rows, wnx, itemsize)`` with (the start of) the chunk's bytes → int."""
    if rows is None:
        masks = np.asarray(data_or_masks)
        itemsize = masks.dtype.itemsize
        _uint(itemsize)
    else:
        masks = _tables(data_or_masks, rows, wnx, itemsize)[1]
    return 2 * pad8(masks.size * itemsize) + 8 * popcount(masks)


def check_chunk(data, rows, wnx, itemsize):
    """Raises ``ValueError`` unless ``data`` is exactly as long as its mask table says: the tables plus 8 bytes per set bit."""
    want = chunk_size(data, rows, wnx, itemsize)
    if want != len(data):
        raise ValueError(f"the mask table of the chunk asks for {want} bytes, the chunk has {len(data)}")


def decode_reference(data, rows, wnx, dtype):
    """The plane ``[rows][wnx]`` of ``dtype`` the chunk ``data`` encodes (checked with ``check_chunk`` first)."""
    dtype = np.dtype(dtype)
    U = _uint(dtype.itemsize)
    W = 8 * U.itemsize
    check_chunk(data, rows, wnx, dtype.itemsize)
    G, n = groups(rows, wnx)
    base, mask, rest = _tables(data, rows, wnx, dtype.itemsize)
    present = ((mask[:, None] >> np.arange(W, dtype=U)) & U.type(1)).astype(bool)
    words = np.zeros((n, W), dtype=np.uint64)
    words[present] = rest.view("<u8")
    res = np.zeros((n, LANES), dtype=U)
    for k in range(W):
        res |= ((words[:, k, None] >> _LANE) & np.uint64(1)).astype(U) << U.type(k)
    t = (np.bitwise_xor.accumulate(res, axis=1) ^ base[:, None]).reshape(rows, G * LANES)[:, :wnx]
    u = np.ascontiguousarray(t)
    for i in range(1, ROW_BLOCK):
        below = u[i::ROW_BLOCK]
        below ^= u[i - 1::ROW_BLOCK][:len(below)]
    return u.view(dtype)
