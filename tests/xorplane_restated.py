"""The "xorplane16" codec of packed checkpoints restated for the tests, element by element, from its specification (DESIGN
§4.10, include/armon_hip.h) — never from armon.jl_amd/plane_codec.py, which it is there to check. Slow on purpose: plain
Python integers, one group at a time.

    t[r][c] = u[r][c] if r % 16 == 0 else u[r][c] ^ u[r-1][c]
    group g = r G + j, G = ceil(C / 64), n = R G; lane l of group (r, j) is column 64 j + l
    base = t[r][64 j]; res[0] = 0; res[l] = t[r][64 j + l] ^ t[r][64 j + l - 1] for columns < C, 0 past C
    mask = OR of res; for every set bit k of mask, ascending, one 64-bit word whose bit l is bit k of res[l]
    bytes: base[n] (W/8 each, zero-padded to a multiple of 8), mask[n] (the same), the words of group 0, 1, ...
"""
import numpy as np


def pad8(n):
    return (n + 7) // 8 * 8


def bit_patterns(plane):
    plane = np.ascontiguousarray(plane)
    return plane.view(np.uint64 if plane.dtype.itemsize == 8 else np.uint32)


def shape_of(R, C, itemsize):
    """→ (G, n, bytes of one table, the bound)."""
    G = -(-C // 64)
    n = R * G
    return G, n, pad8(n * itemsize), 2 * pad8(n * itemsize) + 8 * 8 * itemsize * n


def encode(plane):
    """→ (the chunk's bytes, the masks as Python integers)."""
    u = bit_patterns(plane)
    R, C = u.shape
    size = u.dtype.itemsize
    W = 8 * size
    G, n, table, _ = shape_of(R, C, size)
    rows = [[int(v) for v in row] for row in u]
    bases, masks, words = [], [], []
    for r in range(R):
        t = rows[r] if r % 16 == 0 else [a ^ b for a, b in zip(rows[r], rows[r - 1])]
        for j in range(G):
            inside = min(64, C - 64 * j)                         # lanes past C have res = 0
            res = [0] * inside
            for lane in range(1, inside):
                res[lane] = t[64 * j + lane] ^ t[64 * j + lane - 1]
            mask = 0
            for v in res:
                mask |= v
            bases.append(t[64 * j])
            masks.append(mask)
            for k in range(W):
                if mask >> k & 1:
                    words.append(sum((res[lane] >> k & 1) << lane for lane in range(inside)))
    fill = b"\0" * (table - n * size)
    data = (b"".join(v.to_bytes(size, "little") for v in bases) + fill + b"".join(v.to_bytes(size, "little") for v in masks) + fill
            + b"".join(w.to_bytes(8, "little") for w in words))
    assert len(data) == 2 * table + 8 * sum(bin(m).count("1") for m in masks)
    return data, masks


def special_values(dtype, shape, seed):
    """A plane of drawn values salted with NaNs that carry payloads, both zeros, both infinities and subnormals."""
    dtype = np.dtype(dtype)
    U = np.uint64 if dtype.itemsize == 8 else np.uint32
    rng = np.random.default_rng(seed)
    plane = rng.standard_normal(shape).astype(dtype)
    bits = plane.view(U)
    expo = U(0x7ff0000000000000 if dtype.itemsize == 8 else 0x7f800000)
    sign = U(1 << (8 * dtype.itemsize - 1))
    frac = int(expo & (~expo + U(1))) - 1                        # the fraction bits
    flat = bits.reshape(-1)
    specials = [expo | U(1), expo | U(frac), sign | expo | U(0x1234 & frac) | U(1), U(0), sign, expo, sign | expo, U(1), U(frac),
                sign | U(7)]
    for i, s in zip(rng.choice(flat.size, size=min(flat.size, 2 * len(specials)), replace=False), specials * 2):
        flat[i] = s
    return plane


def random_bits(dtype, shape, seed):
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=int(np.prod(shape)) * dtype.itemsize, dtype=np.uint8)
    return raw.view(dtype).reshape(shape)


def encode_fast(plane):
    """The same chunk through numpy's bit packing (the GPU tests encode thousands of groups): residuals → bits
    ``[group][lane][k]`` → transposed to ``[group][k][lane]`` → packed into one word per (group, k); a bit-plane is present
    exactly when its word is not zero. tests/test_plane_codec_host.py holds it to ``encode`` → (bytes, masks array)."""
    u = bit_patterns(plane)
    R, C = u.shape
    size = u.dtype.itemsize
    W = 8 * size
    G, n, table, _ = shape_of(R, C, size)
    t = u.copy()
    for r in range(R):
        if r % 16:
            t[r] = u[r] ^ u[r - 1]
    wide = np.zeros((R, 64 * G), dtype=u.dtype)
    wide[:, :C] = t
    res = np.zeros_like(wide)
    res[:, 1:C] = wide[:, 1:C] ^ wide[:, :C - 1]
    res = res.reshape(n, 64)
    res[:, 0] = 0
    bits = np.unpackbits(res.astype(f"<u{size}").view(np.uint8).reshape(n, 64, size), axis=2, bitorder="little")     # [g][lane][k]
    words = np.packbits(bits.transpose(0, 2, 1), axis=2, bitorder="little").reshape(n, W, 8).copy().view("<u8").reshape(n, W)
    masks = np.packbits(words != 0, axis=1, bitorder="little").reshape(n, size).copy().view(f"<u{size}").reshape(n)
    fill = b"\0" * (table - n * size)
    base = wide.reshape(n, 64)[:, 0].astype(f"<u{size}")
    return base.tobytes() + fill + masks.tobytes() + fill + words[words != 0].tobytes(), masks
