"""What tests/test_gpu_scalars_special.py rests on, without a device: the planes of tests/special_planes.py are what they claim,
and the restatement (tests/scalars_restated.py) is finite on every one of them, so that nothing there passes on a reference
that lost the property."""
import numpy as np
import pytest

import special_planes as SP
import special_states as SS
from sweep_reference import real_mask

CASES = [(axis, nx, ny, g) for axis in (0, 1) for (nx, ny) in SS.SHAPES[axis] for g in SS.GHOSTS]
IDS = [f"{'XY'[a]}-{nx}x{ny}-g{g}" for a, nx, ny, g in CASES]


@pytest.mark.parametrize("axis,nx,ny,g", CASES, ids=IDS)
def test_the_planes_are_exactly_representable_and_the_same_in_both_precisions(axis, nx, ny, g):
    ii, jj = SP.index_grids(nx, ny, g, axis)
    for state in SS.STATES:
        p64 = SP.special_planes(state, nx, ny, g, axis, "float64")
        p32 = SP.special_planes(state, nx, ny, g, axis, "float32")
        for k in range(3):
            if (state, k) == (6, 0):                       # the subnormal velocities of state 6: drawn per precision, as the state
                continue
            assert np.array_equal(p32[k].astype(np.float64), p64[k]), (state, SP.NAMES[k])
            assert np.array_equal(np.signbit(p32[k]), np.signbit(p64[k])), (state, SP.NAMES[k])
        for dtype, p in (("float64", p64), ("float32", p32)):
            t = SS.input_of(state, nx, ny, g, axis, dtype)[SS.along_across(axis)[1]]
            assert p[0].tobytes() == t.tobytes()
            assert np.array_equal(p[1].astype(np.float64), SP.ramp_line(ii, (nx, ny)[axis]).ravel())
            assert (p[2] == 0).all() and np.array_equal(np.signbit(p[2]), ((ii + jj) % 2 == 0).ravel())
            assert np.signbit(p[2]).any() and not np.signbit(p[2]).all()
            tiny = float(np.finfo(np.dtype(dtype)).smallest_subnormal)
            count = p[3].astype(np.float64) / tiny            # exact: a division by a power of two
            assert np.array_equal(count, np.rint(count)) and np.abs(count).max() <= 2000 and (count != 0).any()
            assert np.abs(p[3]).max() < float(np.finfo(np.dtype(dtype)).tiny)
            assert p[3].dtype == np.dtype(dtype) and all(not a.flags.writeable for a in p)


@pytest.mark.parametrize("n", sorted({(nx, ny)[axis] for axis in (0, 1) for nx, ny in SS.SHAPES[axis]}))
def test_the_ramps_slope_ratios_are_exactly_one_a_half_and_two(n):
    """Differences of neighbouring cells along the axis, ghosts included (the widest ghost layer of the tests): the ratio of a
    difference to the one before it is 1 everywhere, 2 at the knee; the other way round 1/2. Computed in fp32."""
    g = max(SS.GHOSTS)
    line = SP.ramp_line(np.arange(-g, n + g), n).astype(np.float32)
    d = np.diff(line)
    assert (d > 0).all()
    up, down = d[1:] / d[:-1], d[:-1] / d[1:]
    assert set(up.tolist()) == {1., 2.} and set(down.tolist()) == {1., 0.5}
    knee = np.flatnonzero(up == 2.)
    assert knee.tolist() == [n // 2 + g - 1] and 2 * g < knee[0] < n - 2 * g      # one knee, away from the mirrors
    assert np.array_equal(np.cumsum(np.concatenate([[line[0]], d]), dtype=np.float32), line)     # nothing was rounded


@pytest.mark.parametrize("dtype", SS.DTYPES)
@pytest.mark.parametrize("axis,nx,ny,g", CASES, ids=IDS)
def test_the_restatement_is_finite_on_the_special_planes(axis, nx, ny, g, dtype):
    """Every (state, shape, triple, precision) of the GPU test, with the mirrors of the exact launches and with the walls of the
    tuned ones; the plane of zeros stays zeros."""
    inside = real_mask(nx, ny, g, axis)
    for state in SS.STATES:
        for triple in SS.TRIPLES:
            for walls in (False, True):
                out = SP.restated_planes(state, nx, ny, g, axis, triple, dtype, walls=walls)
                assert len(out) == 4
                for k, a in enumerate(out):
                    assert np.isfinite(a[inside]).all(), (SS.STATES[state], triple, SP.NAMES[k], walls)
                assert (out[2][inside] == 0).all(), (SS.STATES[state], triple)
            if state in (4, 5):                             # the non-finite plane of the isolation test spreads, and not everywhere
                bad = ~np.isfinite(SP.restated_planes(state, nx, ny, g, axis, triple, dtype, walls=True, poison=True)[3]) & inside
                assert 2 <= bad.sum() < inside.sum() // 2, (SS.STATES[state], triple, int(bad.sum()))
