"""armon_hip_sweep_scalars_bounded on states and planes made of special values: the six states of
tests/special_states.py carrying the planes of tests/bounded_planes.py — the state's transverse velocity, a ramp with a knee,
plateaus of three equal cells, mixed signed zeros, and subnormals in a launch of their own. The bounded rule is a plain minmod,
an upwind choice at ``dt us > 0`` and a clamp to the smallest and largest of three neighbours taken by comparisons: all ties,
signs of zero and NaN order. This pins, for phi under that rule, what tests/test_gpu_scalars_special.py pins under the remap:
minmod at Dp == 0 (where the sign factor is Dp itself, +-0), at Dp == Dm and at the knee, the upwind choice at an interface
velocity of exactly 0, mass fluxes of 0 and of subnormal size, +-0 and subnormal values through the clamp, the clamp's own
neighbours (cell by cell, not the plane's global range), and a non-finite value in one plane of a multi-plane launch.
tests/test_bounded_special_host.py shows on the restatement alone that these inputs are what is assumed of them here.

Shapes, ghost widths and precisions are those of tests/special_states.py, the triples those of tests/bounded_planes.py: all four
(scheme, projection) pairs, on which the ring slots of ScalarMarch::step_bounded depend; perfect gas; both sides mirrored. The
exact launches mirror with the factor pairs of the harness, the tuned ones and the isolation test with walls. Prints what it
measures (pytest -s)."""
import numpy as np
import pytest

import bounded_planes as BP
import special_states as SS
from scalars_harness import Planes, assert_untouched, bounded_launch, descriptor, exact_launch_is_the_restatement
from sweep_harness import MARKER, bits, block_cache
from sweep_reference import real_mask

pytestmark = pytest.mark.gpu

WALLS = dict(f_low=BP.WALLS[0], f_high=BP.WALLS[1])
CASES = [(dtype, axis, nx, ny, g, state) for dtype in SS.DTYPES for axis in (0, 1) for (nx, ny) in SS.SHAPES[axis] for g in SS.GHOSTS
         for state in SS.STATES]
IDS = [f"{d}-{'XY'[a]}-{nx}x{ny}-g{g}-{SS.STATES[s]}" for d, a, nx, ny, g, s in CASES]
ISOLATION = [(c, i) for c, i in zip(CASES, IDS) if c[5] in (4, 5)]


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


def options(axis, triple):
    return (axis, triple[0], triple[1], triple[2], "perfect_gas")


def walled_launch(blk, planes, opts, exact, dt):
    """One launch under WALLS of ``planes`` on the state the block holds. Returns phi_out."""
    P = Planes(blk, len(planes))
    try:
        blk.mark_outputs()
        P.upload(planes)
        bounded_launch(blk, descriptor(blk, *opts, exact, dt, **WALLS), P.inp, P.out)
        return P.fetch()[1]
    finally:
        P.free()


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_exact_bounded_sweep_of_special_planes_is_the_restatement(blocks, dtype, axis, nx, ny, g, state):
    """The ns = 4 launch, and the subnormal plane alone: the restatement's bits as integers on the real cells — a zero of the
    other sign is a difference —, the marker elsewhere; phi_in, the state and the descriptor's outputs untouched."""
    blk = blocks(nx, ny, g, dtype)
    f = SS.input_of(state, nx, ny, g, axis, dtype)
    planes = BP.bounded_special_planes(state, nx, ny, g, axis, dtype)
    tiny = BP.fifth_plane(state, nx, ny, g, axis, dtype)
    dt, _dx = SS.step_of((nx, ny)[axis], dtype)
    for triple in BP.TRIPLES:
        want, _ = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype)
        what = f"{SS.STATES[state]} {'-'.join(triple)}: "
        for some, theirs in ((planes, want[:4]), ([tiny], want[4:])):
            exact_launch_is_the_restatement(blk, f, some, theirs, *options(axis, triple), dt, each_alone=False,
                                            what=what + ("subnormal plane: " if len(some) == 1 else ""), launch=bounded_launch)


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_tuned_bounded_sweep_of_special_planes(blocks, dtype, axis, nx, ny, g, state):
    """Tuned arithmetic under walls, exactly the real cells written. Every real cell of every plane lies within the smallest and
    largest of the mirrored input at i - 1, i, i + 1 (no tolerance); every cell of the plateau plane whose three neighbours are
    equal has the input's bits; the plane of mixed zeros comes out as zeros of either sign (how many signs agree with the
    restatement is printed, not asserted); every plane is finite; the ramp stays within 4 max(kappa, 1) eps of the field maximum
    from the fp64 restatement of the input the kernel got, kappa = max|restated32 - restated64| / (eps32 max|restated64|) on
    the fp32 form of these very inputs (the yardstick and bound of tests/test_gpu_scalars_special.py, with bounded_sweep)."""
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    mark = MARKER[blk.dtype.name]
    f = SS.input_of(state, nx, ny, g, axis, dtype)
    planes = BP.bounded_special_planes(state, nx, ny, g, axis, dtype)
    kept = BP.kept_cells(planes[2], nx, ny, g, axis)
    assert kept.sum() > 1
    dt, _dx = SS.step_of((nx, ny)[axis], dtype)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    eps32 = float(np.finfo(np.float32).eps)
    for triple in BP.TRIPLES:
        what = f"tuned {dtype} {'XY'[axis]} {nx}x{ny} g{g} {SS.STATES[state]} {'-'.join(triple)}"
        blk.upload(f)
        got = walled_launch(blk, planes, options(axis, triple), False, dt)
        assert_untouched(blk, f, what)
        for k in range(4):
            assert ((bits(got[k]) == mark) == ~inside).all(), f"{what}: phi_out[{k}]: not exactly the real cells were written"
            assert np.isfinite(got[k][inside]).all(), f"{what}: plane {BP.NAMES[k]} is not finite"
            BP.assert_in_local_range(got[k], planes[k], inside, nx, ny, g, axis, what=f"{what}: plane {BP.NAMES[k]}: ")
        moved = np.flatnonzero((bits(got[2]) != bits(planes[2])) & kept)
        assert moved.size == 0, (f"{what}: {moved.size} cells of a plateau changed between equal neighbours, first at flat index "
                                 f"{moved[0]}: {got[2][moved[0]]!r} from {planes[2][moved[0]]!r}")
        same, _ = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype, walls=True)
        assert (got[3][inside] == 0).all(), f"{what}: the plane of zeros holds {got[3][inside][got[3][inside] != 0][:1]!r}"
        agree = int((np.signbit(got[3][inside]) == np.signbit(same[3][inside])).sum())
        r32 = BP.restated_bounded(state, nx, ny, g, axis, triple, "float32", "float32", walls=True)[0][1][inside]
        r64 = BP.restated_bounded(state, nx, ny, g, axis, triple, "float32", "float64", walls=True)[0][1][inside]
        kappa = float(np.abs(r32.astype(np.float64) - r64).max() / (eps32 * np.abs(r64).max()))
        want = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype, "float64", walls=True)[0][1][inside]
        r = float(np.abs(got[1][inside].astype(np.float64) - want).max() / (eps * np.abs(want).max()))
        print(f"\n{what}: ramp {r:.2f} eps of the field maximum (kappa {kappa:.2f}, bound {4 * max(kappa, 1.):.2f}); zeros: {agree} of "
              f"{int(inside.sum())} signs as the restatement's")
        assert r <= 4 * max(kappa, 1.), f"{what}: the ramp is {r:.2f} eps of the field maximum from the fp64 restatement, kappa {kappa:.2f}"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", [c for c, _ in ISOLATION], ids=[i for _, i in ISOLATION])
def test_a_non_finite_plane_stays_in_its_plane_and_its_neighbourhood(blocks, dtype, axis, nx, ny, g, state, exact):
    """The transverse, ramp and plateau planes with the subnormal plane in slot 4, then with one NaN and one +inf in real cells
    of it: planes 1 to 3 are bit for bit those of the launch without them; plane 4 keeps a non-finite value; every real cell of
    plane 4 on another line, or farther than R cells along the axis from a poisoned cell (bounded_planes.reach: 2 under
    euler_2nd, 1 under euler), has the bits of the clean launch. In exact arithmetic the set of non-finite cells is the
    restatement's (the sets, not the payloads; phys::mn / phys::mx are asymmetric in a NaN argument, and
    bounded_restated._mn / _mx restate that)."""
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    f = SS.input_of(state, nx, ny, g, axis, dtype)
    first = BP.bounded_special_planes(state, nx, ny, g, axis, dtype)[:3]
    clean = first + [BP.fifth_plane(state, nx, ny, g, axis, dtype)]
    dirty = first + [BP.fifth_plane(state, nx, ny, g, axis, dtype, poison=True)]
    assert all(inside[c] for c in BP.poison_cells(nx, ny, g, axis)) and not np.isfinite(dirty[3]).all()
    dt, _dx = SS.step_of((nx, ny)[axis], dtype)
    for triple in BP.TRIPLES:
        what = f"{'exact' if exact else 'tuned'} {SS.STATES[state]} {'-'.join(triple)}: "
        blk.upload(f)
        outs = [walled_launch(blk, planes, options(axis, triple), exact, dt) for planes in (clean, dirty)]
        for k in range(3):
            assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), f"{what}plane {k + 1} changed with a non-finite plane 4"
        spoilt = ~np.isfinite(outs[1][3]) & inside
        assert spoilt.any(), what + "the non-finite values vanished"
        far = inside & ~BP.near_poison(nx, ny, g, axis, BP.reach(triple))
        wrong = np.flatnonzero((bits(outs[1][3]) != bits(outs[0][3])) & far)
        assert wrong.size == 0, (f"{what}{wrong.size} cells of plane 4 beyond the reach of a poisoned cell changed, first at flat index "
                                 f"{wrong[0]} (pitch {nx + 2 * g}): {outs[1][3][wrong[0]]!r} from {outs[0][3][wrong[0]]!r}")
        if exact:
            want = BP.restated_bounded(state, nx, ny, g, axis, triple, dtype, walls=True, poison=True)[0][4]
            wrong = np.flatnonzero(spoilt != (~np.isfinite(want) & inside))
            assert wrong.size == 0, (f"{what}{wrong.size} cells of plane 4 are finite on one side only, first at flat index {wrong[0]}: "
                                     f"{outs[1][3][wrong[0]]!r} against the restatement's {want[wrong[0]]!r}")
