"""The window checks of the in-situ entry points (csrc/window.hpp), the host side (no GPU): every windowed entry point, fp64 and
fp32, refuses the same bad windows with the same words, and lets a good one through to its own checks. The context is a fake
one: every argument check comes before the first use of the context.

``history_sample`` needs a handle, which only a device gives: tests/test_gpu_window_walk.py holds it to the same list. The
coarsen and derive entry points take a whole block (no col0, row0, wnx, wny): the block's cases apply to them."""
import ctypes as C

import pytest

import armon_amd
from armon_amd._lib import DeriveSpec, ExactSpec, ProfileSpec

GOOD = dict(row_length=16, nghost=4, nx=8, ny=8, col0=0, row0=0, wnx=8, wny=8, gcol=0, grow=0)
BLOCK_CASES = (dict(nx=0), dict(ny=0), dict(nghost=-1), dict(row_length=15), dict(nx=1 << 31, row_length=(1 << 31) + 8))
WINDOW_CASES = (dict(col0=-1), dict(row0=-1), dict(wnx=0), dict(wny=0), dict(col0=1), dict(row0=1), dict(wnx=9), dict(wny=9),
                dict(col0=8))
POSITION_CASES = (dict(gcol=-1), dict(grow=-1))
BAD_WINDOWS = BLOCK_CASES + WINDOW_CASES + POSITION_CASES      # the 15 of test_profile_host.py, and col0 = nx


def geometry_text(g):
    """What armon_hip_last_error() says of a bad block or window: the first rule of window.hpp that the geometry breaks."""
    if not (g["nx"] >= 1 and g["ny"] >= 1 and g["nghost"] >= 0):
        return "invalid block: nx = %d, ny = %d, nghost = %d" % (g["nx"], g["ny"], g["nghost"])
    if not (g["nx"] < 1 << 31 and g["ny"] < 1 << 31):
        return "block too large: nx = %d, ny = %d" % (g["nx"], g["ny"])
    if g["row_length"] < g["nx"] + 2 * g["nghost"]:
        return "the real cells leave the block: row_length = %d < nx + 2 nghost = %d" % (g["row_length"], g["nx"] + 2 * g["nghost"])
    return "the window [%d, %d) x [%d, %d) leaves the real domain %d x %d" % (
        g["col0"], g["col0"] + g["wnx"], g["row0"], g["row0"] + g["wny"], g["nx"], g["ny"])


DATA = C.create_string_buffer(64)
FAKE_CTX = C.create_string_buffer(4096)
NO_VECTORS = (C.c_void_p * 8)()                     # state_pack's table of vectors, all NULL: read after the window checks only


def _pointers():
    return C.cast(FAKE_CTX, C.c_void_p), C.cast(DATA, C.c_void_p)


def call_state(fn, g, tail):
    """state_pack / state_unpack / state_compare: the position is (global_first, global_nx >= wnx)."""
    ctx, data = _pointers()
    first, gnx = (-1 if g["gcol"] < 0 else 0), (g["wnx"] - 1 if g["grow"] < 0 else 64)
    return fn(ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], 1, C.cast(NO_VECTORS, C.POINTER(C.c_void_p)), g["col0"], g["row0"],
              g["wnx"], g["wny"], first, gnx, data, *tail(data))


def call_cells(fn, g, spec, with_out):
    """profile / profile_bounds / exact_norms / exact_fill: the position is (global_col0, global_row0)."""
    ctx, data = _pointers()
    return fn(ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], data, data, data, data, g["col0"], g["row0"], g["wnx"], g["wny"],
              g["gcol"], g["grow"], C.byref(spec), *((data,) if with_out else ()))


def call_block(fn, g, tail):
    """coarsen / derive: the whole block, factors (2, 2)."""
    ctx, data = _pointers()
    return fn(ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], 2, 2, *tail(data))


def _spec(cls, **kw):
    s = cls()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


# name → (how it is called, the cases that apply, what a good window is refused for further down)
ENTRY_POINTS = {
    "state_pack": (lambda fn, g: call_state(fn, g, lambda d: (d,)), BAD_WINDOWS, "NULL array"),
    "state_unpack": (lambda fn, g: call_state(fn, g, lambda d: (d,)), BAD_WINDOWS, "NULL array"),
    "state_compare": (lambda fn, g: call_state(fn, g, lambda d: (0.0, 0.0, d, None)), BAD_WINDOWS, "NULL array"),
    "profile": (lambda fn, g: call_cells(fn, g, _spec(ProfileSpec, kind=3), True), BAD_WINDOWS, "unknown profile kind 3"),
    "profile_bounds": (lambda fn, g: call_cells(fn, g, _spec(ProfileSpec, kind=3), True), BAD_WINDOWS, "unknown profile kind 3"),
    "exact_norms": (lambda fn, g: call_cells(fn, g, _spec(ExactSpec, form=7), True), BAD_WINDOWS, "unknown form 7"),
    "exact_fill": (lambda fn, g: call_cells(fn, g, _spec(ExactSpec, form=7), False), BAD_WINDOWS, "unknown form 7"),
    "coarsen": (lambda fn, g: call_block(fn, g, lambda d: (None, d, d, d, d, d)), BLOCK_CASES, "NULL array"),
    "derive": (lambda fn, g: call_block(fn, g, lambda d: (d, d, d, d, C.byref(_spec(DeriveSpec, nq=0)), d)), BLOCK_CASES, "derive: nq = 0"),
}


@pytest.mark.parametrize("suffix", ["", "_f32"])
@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_every_entry_point_refuses_the_same_windows_in_the_same_words(name, suffix):
    L = armon_amd.lib()
    fn = getattr(L, "armon_hip_" + name + suffix)
    call, cases, further = ENTRY_POINTS[name]
    for bad in cases:
        g = {**GOOD, **bad}
        assert call(fn, g) == 1, (name + suffix, bad)                   # ARMON_ERR_INVALID_ARG
        text = L.armon_hip_last_error().decode()
        if bad in POSITION_CASES:
            assert text.startswith("invalid global position: "), (name + suffix, bad, text)
        else:
            assert text == geometry_text(g), (name + suffix, bad, text)
    # the good window passes every shared check: the call is refused for what comes after them (never for the fake context)
    assert call(fn, GOOD) == 1 and further in L.armon_hip_last_error().decode(), (name + suffix, L.armon_hip_last_error())

