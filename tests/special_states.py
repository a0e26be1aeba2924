"""States made of special values for one sweep of the real kernels (test infrastructure: a plain helper module, no fixtures).

The physical test cases are piecewise constant with velocities +0 at rest, and continuous random states never produce a tie:
no slope ratio of exactly 0, 1/2, 1 or 2, no interface velocity of exactly 0, never a -0. These six states do. ``ii`` is the
real-cell index along the sweep axis, ``jj`` the one across it (negative in the low ghost cells: every cell of the ghosted block
is filled by the same formula); every value is exactly representable in fp32, so both precisions and both oracles get the same
numbers.

 1 rest           rho = 1, u = v = +0, E = 2.5
 2 mixed zeros    rho = 0.125, E = 2.5; along the axis -0 where (ii + jj) is even, else +0; across it -0 where
                  (ii + 2 jj) % 3 != 0, else +0
 3 step           Sod's two states split at the middle of the axis; +0 along the axis, -0 across it
 4 collision      rho = 1, E = 2.5; +0.5 below the middle of the axis, -0.5 above: the interface velocity in the middle is exactly 0
                  (the upwind choice at disp == 0); across the axis +-0.25 by the parity of jj
 5 ramps          rho = 1 + ii / 64, E = 3 + ii / 32; along the axis slope 1 / 128 below the middle and 1 / 64 above (slope ratios
                  of exactly 1, 1/2 and 2: the knees of minmod and superbee); across it (jj % 64) / 32 - 0.25
 6 subnormal      rho = 1 + (ii % 3) / 4, E = 2.5 + (jj % 2) / 2; both velocities random integer multiples, within +-2000, of the
                  smallest subnormal of the precision

(State 5 wraps the transverse ramp at 64 cells: unwrapped, a block 530 cells wide reaches a transverse velocity of 16 with a
total energy of 4, a negative internal energy and no sound speed. Up to 64 cells across it is jj / 32 - 0.25.)
"""
import functools
import os

import numpy as np

from sweep_reference import STATE, reference_sweep

SEED = int(os.environ.get("ARMON_RANDOM_SEED", "20261019"))
STATES = {1: "rest", 2: "mixed_zeros", 3: "step", 4: "collision", 5: "ramps", 6: "subnormal"}
TRIPLES = [("GAD", "minmod", "euler_2nd"), ("GAD", "superbee", "euler"), ("Godunov", "minmod", "euler_2nd")]
# each launch form needs a second, partial unit: smaller, and a tie never falls in the last strip or run
SHAPES = {0: [(123, 5), (250, 9)], 1: [(70, 101), (530, 37)]}
GHOSTS = (4, 5)
DTYPES = ("float64", "float32")
F_LOW, F_HIGH = (-1., 1.), (1., -1.)        # as tests/sweep_harness.py: (along the axis, across it) of either mirror


def special_state(state, nx, ny, g, axis, dtype, seed=SEED):
    """{rho, u, v, E}: flat arrays over the ghosted block in ``dtype`` for a sweep along ``axis`` (0 = x, 1 = y)."""
    dtype = np.dtype(dtype)
    y, x = np.meshgrid(np.arange(-g, ny + g), np.arange(-g, nx + g), indexing="ij")
    ii, jj = (x, y) if axis == 0 else (y, x)
    n = (nx, ny)[axis]
    mid = n // 2
    below = ii < mid
    one = np.ones(ii.shape)
    if state == 1:
        rho, ua, ut, E = one, 0. * one, 0. * one, 2.5 * one
    elif state == 2:
        rho, E = 0.125 * one, 2.5 * one
        ua = np.where((ii + jj) % 2 == 0, -0., 0.)
        ut = np.where((ii + 2 * jj) % 3 != 0, -0., 0.)
    elif state == 3:
        rho, E = np.where(below, 1., 0.125), np.where(below, 2.5, 2.)
        ua, ut = 0. * one, -0. * one
    elif state == 4:
        rho, E = one, 2.5 * one
        ua = np.where(below, 0.5, -0.5)
        ut = np.where(jj % 2 == 0, 0.25, -0.25)
    elif state == 5:
        rho, E = 1. + ii / 64., 3. + ii / 32.
        ua = np.where(below, ii / 128., mid / 128. + (ii - mid) / 64.)
        ut = (jj % 64) / 32. - 0.25
    elif state == 6:
        rng = np.random.default_rng([seed, nx, ny, g, axis])
        tiny = float(np.finfo(dtype).smallest_subnormal)
        rho, E = 1. + (ii % 3) / 4., 2.5 + (jj % 2) / 2.
        ua = rng.integers(-2000, 2001, ii.shape) * tiny
        ut = rng.integers(-2000, 2001, ii.shape) * tiny
    else:
        raise ValueError(state)
    u, v = (ua, ut) if axis == 0 else (ut, ua)
    f = dict(rho=rho, u=u, v=v, E=E)
    out = {}
    for k in STATE:
        a = np.ascontiguousarray(f[k], dtype=np.float64).ravel()
        out[k] = a.astype(dtype)
        assert np.array_equal(out[k].astype(np.float32).astype(np.float64), a) or state == 6, k    # exactly representable in fp32
        assert np.array_equal(np.signbit(out[k]), np.signbit(a)), k
    return out


def along_across(axis):
    """Names of the velocity along the sweep axis and of the one across it."""
    return ("u", "v") if axis == 0 else ("v", "u")


def step_of(n_axis, dtype):
    """(dt, dx, dy-independent): the cell size along the axis in the working precision and dt = 0.2 dx / 3 rounded to fp32, the
    same number in either precision."""
    T = np.dtype(dtype).type
    dx = float(T(1.) / T(n_axis))
    return float(np.float32(0.2 * dx / 3.)), dx


@functools.lru_cache(maxsize=None)
def input_of(state, nx, ny, g, axis, dtype):
    f = special_state(state, nx, ny, g, axis, dtype)
    for a in f.values():
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def special_reference(state, nx, ny, g, axis, triple, dtype, ref_dtype=None):
    """(input in ``dtype``, one sweep of the oracle in ``ref_dtype`` on that very input with both sides mirrored, dt). The CFL
    reduction takes the cell sizes of the unit square in ``dtype``, as ArmonParameters.cell_size gives them. Computed once per
    case, shared, never modified."""
    scheme, limiter, projection = triple
    f = input_of(state, nx, ny, g, axis, dtype)
    T = np.dtype(dtype).type
    cs = [float(T(1.) / T(nx)), float(T(1.) / T(ny))]
    dt, dx = step_of((nx, ny)[axis], dtype)
    assert dx == cs[axis]
    rd = np.dtype(ref_dtype or dtype)
    fin = {k: f[k].astype(rd) for k in STATE}
    ref = reference_sweep(fin, nx, ny, g, axis, scheme, limiter, projection, "perfect_gas", dt, dx, 1, 1, F_LOW, F_HIGH, rd,
                          cfl_dx=cs[0], cfl_dy=cs[1])
    for k in STATE + ("p", "c"):
        getattr(ref, k).setflags(write=False)
    return f, ref, dt
