"""Planes made of special values for one bounded scalar sweep (armon_hip_sweep_scalars_bounded) over the states
of tests/special_states.py (test infrastructure: a plain helper module, no tests). Built like tests/special_planes.py, whose
index grids, walls and poisoned cells it takes; ``ii`` is the real-cell index along the sweep axis, ``jj`` the one across it, and
every cell of the ghosted block is filled by the same formula.

 1 transverse   plane 1 of special_planes, the state's transverse velocity: the clamp engages on hundreds of its cells
 2 ramp         plane 2 of special_planes: minmod with Dp == Dm, and a knee where one difference is twice the other
 3 plateaus     (0, 0.7, 1)[((ii + 3 jj) // 3) % 3]: runs of three equal cells along the axis, offset line by line. The middle
                cell of a run has three equal neighbours and must not change; the other two stand beside a jump: minmod sees a
                zero difference on one side, a tie both ways, and a Dp of exactly +-0
 4 mixed zeros  plane 3 of special_planes
 5 subnormal    plane 4 of special_planes, or ``special_planes.poisoned``: launched alone, or in the slot of plane 4

Planes 2 to 4 are the same numbers in both precisions (0.7 rounded to fp32: the plateaus are exactly representable there).
``local_bounds`` and ``kept_cells`` state what the clamp promises of an input: its bounds cell by cell, and the cells it must
return unchanged."""
import functools

import numpy as np

import special_planes as SP
import special_states as SS
from bounded_restated import bounded_sweep
from scalars_restated import mirror_plus
from special_planes import WALLS, index_grids, poison_cells, poisoned      # noqa: F401 (what the tests take from here)

NAMES = ("transverse", "ramp", "plateaus", "mixed_zeros", "subnormal")
TRIPLES = SS.TRIPLES + [("Godunov", "minmod", "euler")]          # all four (scheme, projection) pairs
LEVELS = (0., float(np.float32(0.7)), 1.)


def reach(triple):
    """How many cells along the axis a value can reach in one sweep: the slope at the donor, the flux at its two faces, the
    clamp's bounds one cell either way — 2 cells under euler_2nd, 1 under euler."""
    return 2 if triple[2] == "euler_2nd" else 1


@functools.lru_cache(maxsize=None)
def bounded_special_planes(state, nx, ny, g, axis, dtype):
    """The four planes (flat, ghosted, read-only) in ``dtype`` for a bounded sweep along ``axis`` of special state ``state``."""
    dtype = np.dtype(dtype)
    ii, jj = index_grids(nx, ny, g, axis)
    old = SP.special_planes(state, nx, ny, g, axis, dtype.name)
    plateaus = np.choose(((ii + 3 * jj) // 3) % 3, LEVELS).ravel().astype(dtype)
    plateaus.setflags(write=False)
    return [old[0], old[1], plateaus, old[2]]


def fifth_plane(state, nx, ny, g, axis, dtype, poison=False):
    p = poisoned(state, nx, ny, g, axis, dtype) if poison else SP.special_planes(state, nx, ny, g, axis, np.dtype(dtype).name)[3]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def restated_bounded(state, nx, ny, g, axis, triple, dtype, ref_dtype=None, walls=False, poison=False):
    """One restated bounded sweep in ``ref_dtype`` of the five planes above in ``dtype`` (the fifth ``poisoned`` if asked) carried
    by the state in ``dtype``, both sides mirrored with the factors of tests/special_states.py, or with WALLS. Perfect gas, the
    step of ``special_states.step_of``. Returns ``(planes, planes before the clamp)``. Shared, never modified."""
    scheme, limiter, projection = triple
    rd = np.dtype(ref_dtype or dtype)
    f = {k: a.astype(rd) for k, a in SS.input_of(state, nx, ny, g, axis, dtype).items()}
    planes = bounded_special_planes(state, nx, ny, g, axis, dtype) + [fifth_plane(state, nx, ny, g, axis, dtype, poison)]
    dt, dx = SS.step_of((nx, ny)[axis], dtype)
    f_low, f_high = WALLS if walls else (SS.F_LOW, SS.F_HIGH)
    out, raw, _ = bounded_sweep(f, [p.astype(rd) for p in planes], nx, ny, g, axis, scheme, limiter, projection, "perfect_gas", dt, dx,
                                1, 1, f_low, f_high, rd)
    for a in out + raw:
        a.setflags(write=False)
    return out, raw


def neighbours(plane, nx, ny, g, axis, bc=(1, 1)):
    """``plane`` at i - 1, i and i + 1 along ``axis`` (flat, ghosted), mirrored with factor +1 on the sides with ``bc`` set, the
    ghosts as given on the others. What wraps around lands in the outermost ghosts only."""
    ax = 1 if axis == 0 else 0
    f = mirror_plus(plane, nx, ny, g, axis, bc[0], bc[1]).reshape(ny + 2 * g, nx + 2 * g)
    return np.roll(f, 1, axis=ax).ravel(), f.ravel(), np.roll(f, -1, axis=ax).ravel()


def local_bounds(plane, nx, ny, g, axis, bc=(1, 1)):
    """(lo, hi): the smallest and the largest of the input at i - 1, i, i + 1, cell by cell — the clamp's bounds."""
    fm, f, fp = neighbours(plane, nx, ny, g, axis, bc)
    return np.minimum(np.minimum(fm, f), fp), np.maximum(np.maximum(fm, f), fp)


def assert_in_local_range(out, plane, inside, nx, ny, g, axis, bc=(1, 1), what=""):
    """Every cell of ``out`` under the mask ``inside`` lies within ``local_bounds`` of its own cell of the input ``plane``."""
    lo, hi = local_bounds(plane, nx, ny, g, axis, bc)
    bad = np.flatnonzero(inside & ~((out >= lo) & (out <= hi)))
    assert bad.size == 0, (f"{what}{bad.size} cells outside the range of their three neighbours, first at flat index {bad[0]} "
                           f"(pitch {nx + 2 * g}): {out[bad[0]]!r} not in [{lo[bad[0]]!r}, {hi[bad[0]]!r}]")


def kept_cells(plane, nx, ny, g, axis, bc=(1, 1)):
    """Mask of the real cells whose (mirrored) neighbours i - 1, i, i + 1 are equal: the clamp returns them unchanged."""
    from sweep_reference import real_mask
    fm, f, fp = neighbours(plane, nx, ny, g, axis, bc)
    return real_mask(nx, ny, g, axis) & (fm == f) & (fp == f)


def near_poison(nx, ny, g, axis, r):
    """Mask of the real cells on the line of a poisoned cell and within ``r`` cells of it along the axis."""
    pitch = nx + 2 * g
    m = np.zeros((ny + 2 * g, pitch), dtype=bool)
    for c in poison_cells(nx, ny, g, axis):
        y, x = divmod(c, pitch)
        if axis == 0:
            m[y, max(x - r, g):min(x + r, g + nx - 1) + 1] = True
        else:
            m[max(y - r, g):min(y + r, g + ny - 1) + 1, x] = True
    return m.ravel()
