"""What tests/test_gpu_bounded_special.py rests on, without a device: on the restatement alone (tests/bounded_restated.py), over
the full case list of the GPU test — both precisions, both axes, the shapes and ghost widths of tests/special_states.py, the six
states, the four triples of tests/bounded_planes.py, the mirrors of the exact launches and the walls of the tuned ones — the
planes of tests/bounded_planes.py are what the GPU test assumes:

 finite      every restated output, without poison
 kept        every real cell of the plateau plane whose mirrored neighbours i - 1, i, i + 1 are equal comes out with the
             input's bits, and there is more than one such cell per case
 clamped     for every (precision, axis, shape, triple), summed over the six states and both ghost widths, the plateau plane
             has real cells clamped up (raw < out) and real cells clamped down (raw > out)
 zeros       in at least one state per (precision, axis) the restated plane of mixed zeros differs from its input in sign bits
 local       every restated output of every plane lies within the smallest and largest of the mirrored input at i - 1, i, i + 1
 poison      with ``poisoned`` in the fifth slot the non-finite real cells lie on the two poisoned lines within R cells along the
             axis of a poisoned cell, and every other real cell of that plane has the bits of the clean sweep

The reach R of a non-finite value is what the stencil says — the slope at the donor, the flux at its two faces, the clamp's
bounds one cell either way: 2 cells under euler_2nd, 1 under euler (``bounded_planes.reach``) — and the restatement shows no
wider one on any case. Prints the counts it finds (pytest -s)."""
import numpy as np
import pytest

import bounded_planes as BP
import special_states as SS
from sweep_harness import bits
from sweep_reference import real_mask

CASES = [(dtype, axis, nx, ny) for dtype in SS.DTYPES for axis in (0, 1) for (nx, ny) in SS.SHAPES[axis]]
IDS = [f"{d}-{'XY'[a]}-{nx}x{ny}" for d, a, nx, ny in CASES]


def test_the_plateaus_are_runs_of_three_equal_cells_in_both_precisions():
    for axis in (0, 1):
        for nx, ny in SS.SHAPES[axis]:
            for g in SS.GHOSTS:
                p64 = BP.bounded_special_planes(1, nx, ny, g, axis, "float64")[2]
                p32 = BP.bounded_special_planes(1, nx, ny, g, axis, "float32")[2]
                assert np.array_equal(p32.astype(np.float64), p64) and set(p64.tolist()) == set(BP.LEVELS)
                fm, f, fp = BP.neighbours(p64, nx, ny, g, axis)
                inside = real_mask(nx, ny, g, axis)
                ii, _ = BP.index_grids(nx, ny, g, axis)
                n = (nx, ny)[axis]
                middle = (ii.ravel() % 3 == 1) & inside
                edge = inside & ((ii.ravel() == 0) | (ii.ravel() == n - 1))          # a mirror lengthens a run that ends at it
                kept = BP.kept_cells(p64, nx, ny, g, axis)
                assert np.array_equal(kept & ~edge, middle & ~edge) and (kept | ~middle).all()
                beside = inside & ~kept                                                # one difference is zero, the other a jump
                assert (((fm == f) ^ (fp == f)) | ~beside).all() and beside.sum() >= kept.sum()


@pytest.mark.parametrize("dtype,axis,nx,ny", CASES, ids=IDS)
def test_the_restatement_on_the_bounded_special_planes(oracle, dtype, axis, nx, ny):
    """finite, kept, clamped, zeros (collected per precision and axis below) and local of the module's list."""
    for walls in (False, True):
        for triple in BP.TRIPLES:
            up = down = 0
            engaged = [0] * 5
            for g in SS.GHOSTS:
                inside = real_mask(nx, ny, g, axis)
                for state in SS.STATES:
                    what = (SS.STATES[state], g, triple, walls)
                    planes = BP.bounded_special_planes(state, nx, ny, g, axis, dtype) + [BP.fifth_plane(state, nx, ny, g, axis, dtype)]
                    out, raw = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype, walls=walls)
                    assert len(out) == len(raw) == 5
                    for k in range(5):
                        assert np.isfinite(out[k][inside]).all() and np.isfinite(raw[k][inside]).all(), (what, BP.NAMES[k])
                        BP.assert_in_local_range(out[k], planes[k], inside, nx, ny, g, axis, what=f"{what} {BP.NAMES[k]}: ")
                        engaged[k] += int((bits(raw[k]) != bits(out[k]))[inside].sum())
                    kept = BP.kept_cells(planes[2], nx, ny, g, axis)
                    assert kept.sum() > 1 and np.array_equal(bits(out[2])[kept], bits(planes[2])[kept]), what
                    up += int((raw[2] < out[2])[inside].sum())
                    down += int((raw[2] > out[2])[inside].sum())
                    assert (out[3][inside] == 0).all(), what
            print(f"\n{dtype} {'XY'[axis]} {nx}x{ny} {'-'.join(triple)} {'walls' if walls else 'mirrors'}: plateaus clamped up on {up} "
                  f"cells, down on {down}; the clamp engages on " + ", ".join(f"{n} {c}" for n, c in zip(BP.NAMES, engaged)))
            assert up >= 1 and down >= 1, (triple, walls, up, down)


@pytest.mark.parametrize("dtype", SS.DTYPES)
@pytest.mark.parametrize("axis", (0, 1))
def test_the_signs_of_the_mixed_zeros_change(oracle, axis, dtype):
    """The integer comparison of the GPU test means something: the restated plane of zeros is not its input."""
    changed = set()
    nx, ny = SS.SHAPES[axis][0]
    g = SS.GHOSTS[0]
    inside = real_mask(nx, ny, g, axis)
    for state in SS.STATES:
        plane = BP.bounded_special_planes(state, nx, ny, g, axis, dtype)[3]
        for triple in BP.TRIPLES:
            out, _ = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype)
            if (np.signbit(out[3]) != np.signbit(plane))[inside].any():
                changed.add(SS.STATES[state])
    print(f"\n{dtype} {'XY'[axis]}: the signs of the mixed zeros change under {sorted(changed)}")
    assert changed


@pytest.mark.parametrize("dtype,axis,nx,ny", CASES, ids=IDS)
def test_a_poisoned_plane_spoils_its_neighbourhood_only(oracle, dtype, axis, nx, ny):
    """poison of the module's list, under the walls of the isolation test, states 4 and 5."""
    for g in SS.GHOSTS:
        inside = real_mask(nx, ny, g, axis)
        for state in (4, 5):
            for triple in BP.TRIPLES:
                clean, _ = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype, walls=True)
                dirty, _ = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype, walls=True, poison=True)
                for k in range(4):
                    assert np.array_equal(bits(clean[k])[inside], bits(dirty[k])[inside])
                near = BP.near_poison(nx, ny, g, axis, BP.reach(triple))
                assert (near & inside).sum() == 2 * (2 * BP.reach(triple) + 1)           # away from the edges
                spoilt = ~np.isfinite(dirty[4]) & inside
                what = (SS.STATES[state], g, triple, int(spoilt.sum()))
                assert 2 <= spoilt.sum() and (near | ~spoilt).all(), what
                assert np.array_equal(bits(dirty[4])[inside & ~near], bits(clean[4])[inside & ~near]), what
