"""Planes made of special values for one scalar sweep over the states of tests/special_states.py (test infrastructure: a plain
helper module, no fixtures). ``ii`` is the real-cell index along the sweep axis, ``jj`` the one across it, as there; every cell
of the ghosted block is filled by the same formula.

 1 transverse   the state's own transverse velocity: the plane must come out as the sweep's transverse velocity
 2 ramp         phi = ii / 128 below the middle of the axis, continued with slope 1 / 64 above: where rho is uniform the slope
                ratios of rho phi are exactly 1, 1/2 and 2, the knees of the remap's limiter, on the planes' own slopes
 3 mixed zeros  -0 where (ii + jj) is even, else +0
 4 subnormal    random integer multiples, within +-2000, of the smallest subnormal of the precision

Planes 1 to 3 are exactly representable in fp32 (plane 1 of state 6, the subnormal velocities, only in its own precision, as
the state itself), so both precisions and both restatements get the same numbers; plane 4 is drawn per precision.
``poisoned`` is plane 4 with one NaN and one +inf in real cells away from the edges."""
import functools

import numpy as np

import special_states as SS
from scalars_restated import restated_sweep

NAMES = ("transverse", "ramp", "mixed_zeros", "subnormal")
WALLS = ((-1., 1.), (1., 1.))                 # mirrors whose transverse factor is +1, the one a plane is mirrored with


def index_grids(nx, ny, g, axis):
    y, x = np.meshgrid(np.arange(-g, ny + g), np.arange(-g, nx + g), indexing="ij")
    return (x, y) if axis == 0 else (y, x)


def ramp_line(ii, n):
    mid = n // 2
    return np.where(ii < mid, ii / 128., mid / 128. + (ii - mid) / 64.)


@functools.lru_cache(maxsize=None)
def special_planes(state, nx, ny, g, axis, dtype):
    """The four planes (flat, ghosted, read-only) in ``dtype`` for a sweep along ``axis`` of special state ``state``."""
    dtype = np.dtype(dtype)
    ii, jj = index_grids(nx, ny, g, axis)
    f = SS.input_of(state, nx, ny, g, axis, dtype.name)
    rng = np.random.default_rng([SS.SEED, nx, ny, g, axis, 4])
    tiny = float(np.finfo(dtype).smallest_subnormal)
    planes = [f[SS.along_across(axis)[1]].copy(),
              ramp_line(ii, (nx, ny)[axis]).ravel().astype(dtype),
              np.where((ii + jj) % 2 == 0, -0., 0.).ravel().astype(dtype),
              (rng.integers(-2000, 2001, ii.shape) * tiny).ravel().astype(dtype)]
    for p in planes:
        p.setflags(write=False)
    return planes


def poison_cells(nx, ny, g, axis):
    """Flat indices of the (NaN, +inf) cells of ``poisoned``, on two lines in the middle: the NaN a third along the axis, the +inf
    in the first cell above the middle — in state 4 the donor of the interface whose velocity is exactly 0, where the flux is
    0 x inf if and only if the upwind choice at ``disp == 0`` takes that cell."""
    n, m = ((nx, ny), (ny, nx))[axis]
    cells = []
    for i, j in ((n // 3, m // 2), (n // 2, m // 2 - 1)):
        x, y = (i, j) if axis == 0 else (j, i)
        cells.append((y + g) * (nx + 2 * g) + x + g)
    return cells


def poisoned(state, nx, ny, g, axis, dtype):
    p = special_planes(state, nx, ny, g, axis, dtype)[3].copy()
    a, b = poison_cells(nx, ny, g, axis)
    p[a], p[b] = np.nan, np.inf
    return p


@functools.lru_cache(maxsize=None)
def restated_planes(state, nx, ny, g, axis, triple, dtype, ref_dtype=None, walls=False, poison=False):
    """One restated sweep in ``ref_dtype`` of the planes of ``special_planes`` (plane 4 ``poisoned`` if asked) in ``dtype`` carried
    by the state in ``dtype``, both sides mirrored with the factors of tests/special_states.py, or with WALLS. Perfect gas, the
    step of ``special_states.step_of``. Shared, never modified."""
    scheme, limiter, projection = triple
    rd = np.dtype(ref_dtype or dtype)
    f = {k: a.astype(rd) for k, a in SS.input_of(state, nx, ny, g, axis, dtype).items()}
    planes = list(special_planes(state, nx, ny, g, axis, dtype))
    if poison:
        planes[3] = poisoned(state, nx, ny, g, axis, dtype)
    dt, dx = SS.step_of((nx, ny)[axis], dtype)
    f_low, f_high = WALLS if walls else (SS.F_LOW, SS.F_HIGH)
    out, _ = restated_sweep(f, [p.astype(rd) for p in planes], nx, ny, g, axis, scheme, limiter, projection, "perfect_gas", dt, dx, 1, 1,
                            f_low, f_high, rd)
    for a in out:
        a.setflags(write=False)
    return out

