"""Every user of the window walk (csrc/window.hpp) over ONE list of windows, each against its Python oracle, word for word.

The list takes every branch of the walk, for fp64 (V = 2 columns per lane, a span of 128) and fp32 (V = 4, a span of 256):

 * ``wnx`` in {1, V - 1, 64 V - 1, 64 V, 64 V + 1}: a lane with fewer than V columns left, an exactly full span, a second span with
   one live lane; each with ``wny`` in {1, 5};
 * each shape in four placements: an aligned block (16-B rows: the wide path), ``col0 = 1``, an odd ``row_length``, and vectors
   that start one element into their allocation (three ways of losing the alignment: the element path);
 * one tall window, ``wnx = 1`` and ``wny = 4 x 8 x (CUs of the device) + 3``: more items than the largest grid cap holds waves, so
   every wave of every walker takes more than one turn.

The walkers: history_sample, exact_norms, exact_fill, profile_bounds, profile (its own tiles, the shared lanes), state_compare,
state_pack, state_unpack, and coarsen and derive, which walk a whole block: they take the windows' shapes as blocks in the three
placements that have no ``col0``. history_sample is also held to the bad windows of tests/test_window_host.py here, where a
handle can be had.

No kernel is special to this file: it exists so that a change to window.hpp meets all its users at once."""
import ctypes as C
import re

import numpy as np
import pytest

from sweep_reference import draw_state
from test_window_host import BAD_WINDOWS, GOOD, POSITION_CASES, geometry_text

pytestmark = pytest.mark.gpu

DTYPES = ["float64", "float32"]
STATE = ("rho", "u", "v", "E")
PLACEMENTS = ("aligned", "col0", "odd_pitch", "offset")
G = 4                                   # ghost width: a multiple of V in both types
NX_GLOBAL, GX0, GY0 = 1000, 11, 5       # the block as a tile of a wider domain
GAMMA = 1.4
U64 = np.uint64


@pytest.fixture(scope="module")
def dev():
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.wait()
    d.close()


def shapes(dev, dtype):
    V = 16 // np.dtype(dtype).itemsize
    n_cu = int(re.search(r"(\d+) CUs", dev.name).group(1))              # armon_hip_device_name ends in the CU count
    small = [(wnx, wny, pl) for wnx in sorted({1, V - 1, 64 * V - 1, 64 * V, 64 * V + 1}) for wny in (1, 5) for pl in PLACEMENTS]
    return small + [(1, 4 * 8 * n_cu + 3, "aligned")]


class Block:
    """Four random vectors around a window ``wnx x wny`` in the given placement, on the host and on the device."""

    def __init__(self, dev, dtype, wnx, wny, placement, seed):
        self.dtype, self.wnx, self.wny, self.placement = np.dtype(dtype), wnx, wny, placement
        self.col0, self.row0 = (1 if placement == "col0" else 0), 1
        self.nx, self.ny = self.col0 + wnx, wny + 2
        self.pitch = (self.nx + 2 * G + 3) // 4 * 4 + (1 if placement == "odd_pitch" else 0)
        self.off = 1 if placement == "offset" else 0
        self.rows = self.ny + 2 * G
        n = self.off + self.rows * self.pitch
        f = draw_state(np.random.default_rng(seed), n, "perfect_gas")
        self.host = {k: f[k].astype(dtype) for k in STATE}
        self.buf = {k: dev.from_host(self.host[k]) for k in STATE}
        self.origin = (GX0 + self.col0, GY0 + self.row0)
        self.first = self.origin[1] * NX_GLOBAL + self.origin[0]

    def ptr(self, k):
        return C.c_void_p(self.buf[k].ptr + self.off * self.dtype.itemsize)

    def plane(self, flat):
        return flat[self.off:].reshape(self.rows, self.pitch)

    def window(self, k, flat=None):
        p = self.plane(self.host[k] if flat is None else flat)
        return p[G + self.row0:G + self.row0 + self.wny, G + self.col0:G + self.col0 + self.wnx]

    def real(self, k):
        return self.plane(self.host[k])[G:G + self.ny, G:G + self.nx]

    def geometry(self):
        return (self.pitch, G, self.nx, self.ny)

    def win(self):
        return (self.col0, self.row0, self.wnx, self.wny)

    def __repr__(self):
        return f"{self.dtype.name} window {self.wnx} x {self.wny}, {self.placement}"


@pytest.fixture(scope="module")
def blocks(dev):
    cache = {}

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = [Block(dev, dtype, wnx, wny, pl, 100 + i) for i, (wnx, wny, pl) in enumerate(shapes(dev, dtype))]
        return cache[dtype]

    yield get
    dev.wait()
    cache.clear()


def fn(dev, name, dtype):
    return getattr(dev._L, "armon_hip_" + name + ("_f32" if np.dtype(dtype) == np.float32 else ""))


def ok(dev, rc):
    assert rc == 0, dev._L.armon_hip_last_error()


def eos(b, fields=None):
    """p, c of the perfect gas in the data type, operation for operation as phys::perfect_gas."""
    rho, u, v, E = (b.window(k) for k in STATE) if fields is None else fields
    T = b.dtype.type
    e = E - T(0.5) * (u * u + v * v)
    p = (T(GAMMA) - T(1.)) * rho * e
    return p, np.sqrt((T(GAMMA) * p) / rho)


def words_differ(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} words differ, first at {tuple(bad[0])}" if len(bad) else ""


@pytest.mark.parametrize("dtype", DTYPES)
def test_history_sample(dev, blocks, dtype):
    from armon_amd import history as H
    from armon_amd._lib import HistorySpec
    bs = blocks(dtype)
    spec = HistorySpec()
    spec.eos, spec.gamma, spec.global_nx = 0, GAMMA, NX_GLOBAL
    scale = (-60,) * 6
    spec.scale_exp[:] = list(scale)
    h = C.c_void_p()
    ok(dev, dev._L.armon_hip_history_create(dev.ctx, len(bs), 0, C.byref(h)))
    try:
        sample = fn(dev, "history_sample", dtype)
        for slot, b in enumerate(bs):
            ok(dev, sample(dev.ctx, h, slot, C.byref(spec), *b.geometry(), *[b.ptr(k) for k in STATE], *b.win(), *b.origin))
        raw = np.zeros((len(bs), H.WORDS), dtype=U64)
        ok(dev, dev._L.armon_hip_history_read(dev.ctx, h, 0, len(bs), raw.ctypes.data_as(C.c_void_p), None))
        for slot, b in enumerate(bs):
            p, c = eos(b)
            want = H.reference_record(*[b.window(k) for k in STATE], p, c, origin=b.origin, global_nx=NX_GLOBAL, scale_exp=scale)
            assert not words_differ(raw[slot], want), b
            assert int(raw[slot][H.W_N]) == b.wnx * b.wny and int(raw[slot][H.W_BAD]) == 0, b
        # the bad windows of tests/test_window_host.py: the same answer in the same words, with a handle
        data = [bs[0].ptr(k) for k in STATE]
        for bad in BAD_WINDOWS:
            g = {**GOOD, **bad}
            assert sample(dev.ctx, h, 0, C.byref(spec), g["row_length"], g["nghost"], g["nx"], g["ny"], *data, g["col0"], g["row0"],
                          g["wnx"], g["wny"], g["gcol"], g["grow"]) == 1, bad
            text = dev._L.armon_hip_last_error().decode()
            assert text.startswith("invalid global position: ") if bad in POSITION_CASES else text == geometry_text(g), (bad, text)
    finally:
        ok(dev, dev._L.armon_hip_history_destroy(dev.ctx, h))


def exact_spec(b):
    from armon_amd import analytic as an
    sol = an.ExactSolution(an.RIEMANN, "x", (0.1, 0.0), GAMMA, time=0.17, riemann=an.riemann_exact((1.0, 0.0, 1.0), (0.125, 0.0, 0.1), GAMMA))
    # cells of 1 / NX_GLOBAL from the origin: the windows begin inside the fan, the wide ones reach past the contact
    return sol.spec((0.0, 0.0), (1.0 / NX_GLOBAL, 1.0 / NX_GLOBAL), NX_GLOBAL, samples=2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_norms(dev, blocks, dtype):
    from armon_amd import analytic as an
    out = dev.zeros(4 * an.WORDS, U64)
    for b in blocks(dtype):
        s = exact_spec(b)
        c_spec = an._c_spec(s, None)
        ok(dev, dev._L.armon_hip_exact_norms_reset(dev.ctx, C.c_void_p(out.ptr)))
        ok(dev, fn(dev, "exact_norms", dtype)(dev.ctx, *b.geometry(), *[b.ptr(k) for k in STATE], *b.win(), *b.origin, C.byref(c_spec),
                                              C.c_void_p(out.ptr)))
        dev.wait()
        want = an.reference_record(s, *[b.window(k) for k in STATE], origin=b.origin)
        assert not words_differ(out.to_host().reshape(4, an.WORDS), want), b
    out.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_fill(dev, blocks, dtype):
    from armon_amd import analytic as an
    for b in blocks(dtype):
        s = exact_spec(b)
        c_spec = an._c_spec(s, None)
        scratch = {k: dev.from_host(b.host[k]) for k in STATE}           # (the shared blocks stay as they are)
        ptrs = [C.c_void_p(scratch[k].ptr + b.off * b.dtype.itemsize) for k in STATE]
        ok(dev, fn(dev, "exact_fill", dtype)(dev.ctx, *b.geometry(), *ptrs, *b.win(), *b.origin, C.byref(c_spec)))
        dev.wait()
        gx = np.arange(b.wnx, dtype=np.int64)[None, :] + b.origin[0]
        gy = np.arange(b.wny, dtype=np.int64)[:, None] + b.origin[1]
        want, keep = an.stored_reference(s, gx, gy, b.dtype)
        assert keep.all()
        for k, w in zip(STATE, want):
            expect = b.host[k].copy()
            b.window(k, expect)[...] = w
            assert scratch[k].to_host().tobytes() == expect.tobytes(), (b, k)      # the window, and not one cell around it
            scratch[k].free()


def profile_spec(kind, nbins, scale=(0,) * 5):
    from armon_amd._lib import ProfileSpec
    s = ProfileSpec()
    s.kind, s.eos, s.nbins, s.width = kind, 0, nbins, 1
    s.cx, s.cy, s.dx, s.dy, s.inv_dr, s.gamma = 0.0, 0.0, 1.0, 1.0, 1.0, GAMMA
    s.scale_exp[:] = list(scale)
    return s


@pytest.mark.parametrize("dtype", DTYPES)
def test_profile_bounds_and_profile(dev, blocks, dtype):
    from armon_amd import profile as prof
    bounds = dev.zeros(5, U64)
    scale = (-60,) * 5
    for b in blocks(dtype):
        f = [b.window(k) for k in STATE]
        p, _ = eos(b)
        gx = np.arange(b.wnx, dtype=np.int64)[None, :] + b.origin[0]
        gy = np.arange(b.wny, dtype=np.int64)[:, None] + b.origin[1]
        args = [dev.ctx, *b.geometry(), *[b.ptr(k) for k in STATE], *b.win(), *b.origin]
        bounds.fill_bytes(0)
        ok(dev, fn(dev, "profile_bounds", dtype)(*args, C.byref(profile_spec(0, NX_GLOBAL)), C.c_void_p(bounds.ptr)))
        dev.wait()
        _, t = prof.cell_terms("x", *f, p, gx, gy)
        want = [int(np.array([np.abs(a).max()]).view(U64)[0]) for a in t]
        assert [int(v) for v in bounds.to_host()] == want, b
        # along y for the tall window (a bin per row), along x for the others
        kind, nbins = ("y", GY0 + b.row0 + b.wny) if b.wny > 5 else ("x", GX0 + b.col0 + b.wnx)
        bins = dev.empty(nbins * prof.WORDS, U64)
        ok(dev, dev._L.armon_hip_profile_reset(dev.ctx, nbins, C.c_void_p(bins.ptr)))
        ok(dev, fn(dev, "profile", dtype)(*args, C.byref(profile_spec(prof.KINDS[kind], nbins, scale)), C.c_void_p(bins.ptr)))
        dev.wait()
        want = prof.reference_record(kind, nbins, scale, *f, p, origin=b.origin)
        assert not words_differ(bins.to_host().reshape(nbins, prof.WORDS), want), b
        bins.free()
    bounds.free()


def vectors(b):
    return (C.c_void_p * 4)(*[b.ptr(k).value for k in STATE])


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_pack_and_unpack(dev, blocks, dtype):
    from armon_amd.checkpoint import digest_reference
    for b in blocks(dtype):
        n = b.wnx * b.wny
        dense, digest, back = dev.zeros(4 * n, dtype), dev.zeros(8, U64), dev.zeros(8, U64)
        ok(dev, fn(dev, "state_pack", dtype)(dev.ctx, *b.geometry(), 4, vectors(b), *b.win(), b.first, NX_GLOBAL, C.c_void_p(dense.ptr),
                                             C.c_void_p(digest.ptr)))
        blank = {k: dev.from_host(np.full(b.host[k].size, 7.5, dtype=dtype)) for k in STATE}
        table = (C.c_void_p * 4)(*[blank[k].ptr + b.off * b.dtype.itemsize for k in STATE])
        ok(dev, fn(dev, "state_unpack", dtype)(dev.ctx, *b.geometry(), 4, table, *b.win(), b.first, NX_GLOBAL, C.c_void_p(dense.ptr),
                                               C.c_void_p(back.ptr)))
        dev.wait()
        got = dense.to_host().reshape(4, b.wny, b.wnx)
        want = [digest_reference(b.window(k), q, NX_GLOBAL, b.origin) for q, k in enumerate(STATE)]
        for q, k in enumerate(STATE):
            assert got[q].tobytes() == np.ascontiguousarray(b.window(k)).tobytes(), (b, k)
            expect = np.full(b.host[k].size, 7.5, dtype=dtype)
            b.window(k, expect)[...] = b.window(k)
            assert blank[k].to_host().tobytes() == expect.tobytes(), (b, k)       # the window, and not one cell around it
        for d in (digest, back):
            assert [int(v) for v in d.to_host()[:4]] == want and not d.to_host()[4:].any(), b
        for a in [dense, digest, back] + list(blank.values()):
            a.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_compare(dev, blocks, dtype):
    from armon_amd.compare import cell_rule, diff_reference
    T = np.dtype(dtype).type
    rtol, atol = 4 * float(np.finfo(dtype).eps), 0.0
    diff = dev.zeros(64, U64)
    for i, b in enumerate(blocks(dtype)):
        rng = np.random.default_rng(500 + i)
        ref = np.stack([np.ascontiguousarray(b.window(k)) for k in STATE])
        for q in range(4):                                               # a last-place difference, a gross one and a NaN per variable
            for kind in range(3):
                j, c = int(rng.integers(b.wny)), int(rng.integers(b.wnx))
                ref[q, j, c] = (np.nextafter(ref[q, j, c], T(np.inf)), ref[q, j, c] * T(1.5), T(np.nan))[kind]
        ref_dev, row_out = dev.from_host(ref.ravel()), dev.zeros(4 * b.wny, np.uint32)
        ok(dev, dev._L.armon_hip_state_diff_reset(dev.ctx, 8, C.c_void_p(diff.ptr)))
        ok(dev, fn(dev, "state_compare", dtype)(dev.ctx, *b.geometry(), 4, vectors(b), *b.win(), b.first, NX_GLOBAL, C.c_void_p(ref_dev.ptr),
                                                rtol, atol, C.c_void_p(diff.ptr), C.c_void_p(row_out.ptr)))
        dev.wait()
        got, rows = diff.to_host().reshape(8, 8), row_out.to_host().reshape(4, b.wny)
        for q, k in enumerate(STATE):
            assert tuple(int(v) for v in got[q]) == diff_reference(b.window(k), ref[q], rtol, atol, NX_GLOBAL, b.origin), (b, k)
            assert rows[q].tolist() == cell_rule(b.window(k), ref[q], rtol, atol)[1].sum(axis=1).tolist(), (b, k)
        ref_dev.free()
        row_out.free()
    diff.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_coarsen_and_derive_walk_the_block(dev, blocks, dtype):
    """Factors (1, 1): a coarse cell is a cell, so the planes are the per-cell rule's (rho, (rho u) / rho, ... and
    derived.reference_planes) and only the walk over the block is under test."""
    from armon_amd import derived
    from armon_amd._lib import DeriveSpec
    spec = DeriveSpec()
    spec.nq, spec.eos, spec.neighbours, spec.gamma = 8, 0, 0, GAMMA
    spec.dx = spec.dy = 1.0 / NX_GLOBAL
    for q in range(8):
        spec.quantity[q], spec.reduce[q] = q, 0
    for b in blocks(dtype):
        if b.col0:
            continue                                                     # (a block has no col0)
        f = [np.ascontiguousarray(b.real(k)) for k in STATE]
        n = b.nx * b.ny
        out = dev.zeros(8 * n, dtype)
        ok(dev, fn(dev, "coarsen", dtype)(dev.ctx, *b.geometry(), 1, 1, *[b.ptr(k) for k in STATE], None, C.c_void_p(out.ptr)))
        dev.wait()
        got = out.to_host()[:4 * n].reshape(4, b.ny, b.nx)
        rho = f[0]
        for q, want in enumerate([rho] + [(rho * a) / rho for a in f[1:]]):
            assert got[q].tobytes() == want.tobytes(), (b, "coarsen", STATE[q])
        ok(dev, fn(dev, "derive", dtype)(dev.ctx, *b.geometry(), 1, 1, *[b.ptr(k) for k in STATE], C.byref(spec), C.c_void_p(out.ptr)))
        dev.wait()
        got = out.to_host().reshape(8, b.ny, b.nx)
        want = derived.reference_planes(*f, b.dtype.type(spec.dx), b.dtype.type(spec.dy), GAMMA)
        for q, name in enumerate(derived.QUANTITIES):
            assert got[q].tobytes() == want[name].tobytes(), (b, "derive", name)
        out.free()
