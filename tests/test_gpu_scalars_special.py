"""armon_hip_sweep_scalars on states and planes made of special values: the six states of tests/special_states.py (rest, mixed
zeros, a step, an interface velocity of exactly 0, slope ratios of exactly 1, 1/2 and 2, subnormal velocities) carrying the four
planes of tests/special_planes.py (the state's transverse velocity, a ramp with knees, mixed signed zeros, subnormals) in one
launch of ns = 4. tests/test_gpu_special_states.py pins ties and special values for rho, u, v and E; this does for phi: the
upwind choice at ``disp == 0``, the limiter knees of the second-order remap on the planes' own slopes, +-0 and subnormal plane
values, and a non-finite value in one plane of a multi-plane launch. tests/test_scalars_special_host.py shows that the
restatement is finite on all of it and that the planes are what they claim.

Shapes, ghost widths, scheme triples and precisions are those of tests/special_states.py; perfect gas; both sides mirrored.
The exact launches mirror with the factor pairs of the harness; the tuned ones with walls whose transverse factor is +1, under
which plane 1 must be the state sweep's transverse velocity. Prints what it measures (pytest -s)."""
import numpy as np
import pytest

import special_planes as SP
import special_states as SS
from scalars_harness import Planes, assert_untouched, descriptor, exact_launch_is_the_restatement, launch, plane_kappa
from sweep_harness import MARKER, bits, block_cache
from sweep_reference import real_mask

pytestmark = pytest.mark.gpu

WALLS = dict(f_low=SP.WALLS[0], f_high=SP.WALLS[1])
CASES = [(dtype, axis, nx, ny, g, state) for dtype in SS.DTYPES for axis in (0, 1) for (nx, ny) in SS.SHAPES[axis] for g in SS.GHOSTS
         for state in SS.STATES]
IDS = [f"{d}-{'XY'[a]}-{nx}x{ny}-g{g}-{SS.STATES[s]}" for d, a, nx, ny, g, s in CASES]
ISOLATION = [(c, i) for c, i in zip(CASES, IDS) if c[5] in (4, 5)]


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


def options(axis, triple):
    return (axis, triple[0], triple[1], triple[2], "perfect_gas")


def tuned_launch(blk, f, planes, opts, dt):
    """One tuned launch under WALLS of ``planes`` on the uploaded state ``f``: exactly the real cells written, the state and the
    descriptor's outputs untouched. Returns phi_out."""
    inside = real_mask(blk.nx, blk.ny, blk.g, opts[0])
    mark = MARKER[blk.dtype.name]
    P = Planes(blk, len(planes))
    try:
        blk.mark_outputs()
        P.upload(planes)
        launch(blk, descriptor(blk, *opts, False, dt, **WALLS), P.inp, P.out)
        _, got = P.fetch()
    finally:
        P.free()
    assert_untouched(blk, f, "tuned scalar sweep")
    for k in range(len(planes)):
        assert ((bits(got[k]) == mark) == ~inside).all(), f"phi_out[{k}]: not exactly the real cells were written"
    return got


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_exact_scalar_sweep_of_special_planes_is_the_restatement(blocks, dtype, axis, nx, ny, g, state):
    """Every plane of the ns = 4 launch: the restatement's bits as integers on the real cells — a zero of the other sign is a
    difference —, the marker elsewhere; phi_in, the state and the descriptor's outputs untouched."""
    blk = blocks(nx, ny, g, dtype)
    f = SS.input_of(state, nx, ny, g, axis, dtype)
    planes = SP.special_planes(state, nx, ny, g, axis, dtype)
    dt, _dx = SS.step_of((nx, ny)[axis], dtype)
    for triple in SS.TRIPLES:
        want = SP.restated_planes(state, nx, ny, g, axis, triple, dtype)
        exact_launch_is_the_restatement(blk, f, planes, want, *options(axis, triple), dt, each_alone=False,
                                        what=f"{SS.STATES[state]} {'-'.join(triple)}: ")


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_tuned_scalar_sweep_of_special_planes(blocks, dtype, axis, nx, ny, g, state):
    """Tuned arithmetic. Plane 1 is the transverse velocity armon_hip_sweep writes for the same descriptor, bit for bit. Plane 3
    comes out as zeros of either sign (how many signs agree with the restatement is printed, not asserted). Plane 2 stays
    within 4 kappa eps of the field maximum from the fp64 restatement of the input the kernel got, kappa =
    max|restated32 - restated64| / (eps32 max|restated64|) on the fp32 form of these very inputs (plane_kappa); where that
    yardstick is degenerate (below 0.5: the two restatements agree to half a unit or exactly, as on a fluid at rest, and say
    nothing about the rounding of the operation) it is reported, and the state is held by the exact comparison of the test
    above; the tuned ramp then only has to stay within 4 max(kappa, 1) = 4 eps of the field maximum, the floor
    tests/test_gpu_special_states.py gives a degenerate state. Every plane is finite."""
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    f = SS.input_of(state, nx, ny, g, axis, dtype)
    planes = SP.special_planes(state, nx, ny, g, axis, dtype)
    dt, _dx = SS.step_of((nx, ny)[axis], dtype)
    t_name = SS.along_across(axis)[1]
    eps = float(np.finfo(np.dtype(dtype)).eps)
    for triple in SS.TRIPLES:
        opts = options(axis, triple)
        what = f"tuned {dtype} {'XY'[axis]} {nx}x{ny} g{g} {SS.STATES[state]} {'-'.join(triple)}"
        blk.upload(f)
        got = tuned_launch(blk, f, planes, opts, dt)
        blk.mark_outputs()
        blk.sweep(*opts, False, dt, **WALLS)               # the state sweep of the same descriptor
        state_out = blk.fetch()
        assert np.array_equal(bits(got[0])[inside], bits(state_out[t_name])[inside]), f"{what}: the plane of ut is not the sweep's ut"
        for k in range(4):
            assert np.isfinite(got[k][inside]).all(), f"{what}: plane {k + 1} is not finite"
        # plane 3: zeros
        same = SP.restated_planes(state, nx, ny, g, axis, triple, dtype, walls=True)
        assert (got[2][inside] == 0).all(), f"{what}: the plane of zeros holds {got[2][inside][got[2][inside] != 0][:1]!r}"
        agree = int((np.signbit(got[2][inside]) == np.signbit(same[2][inside])).sum())
        # plane 2: the ramp
        f32 = SS.input_of(state, nx, ny, g, axis, "float32")
        p32 = SP.special_planes(state, nx, ny, g, axis, "float32")
        dt32, dx32 = SS.step_of((nx, ny)[axis], "float32")
        kappa = plane_kappa(f32, [p32[1]], nx, ny, g, *opts, dt32, dx32, **WALLS)[0][0]
        want = SP.restated_planes(state, nx, ny, g, axis, triple, dtype, "float64", walls=True)[1][inside]
        r = float(np.abs(got[1][inside].astype(np.float64) - want).max() / (eps * np.abs(want).max()))
        zeros = f"zeros: {agree} of {int(inside.sum())} signs as the restatement's"
        if kappa < 0.5:
            print(f"\n{what}: degenerate yardstick (kappa {kappa:.3f}): the ramp is held by the exact comparison; tuned {r:.2f} eps "
                  f"of the field maximum (bound 4); {zeros}")
            assert r <= 4, f"{what}: the ramp is {r:.2f} eps of the field maximum from the fp64 restatement, bound 4"
            continue
        print(f"\n{what}: ramp {r:.2f} eps of the field maximum (kappa {kappa:.2f}: {r / kappa:.2f} of it, bound 4 kappa); {zeros}")
        assert r <= 4 * kappa, f"{what}: the ramp is {r:.2f} eps of the field maximum from the fp64 restatement, kappa {kappa:.2f}"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", [c for c, _ in ISOLATION], ids=[i for _, i in ISOLATION])
def test_a_non_finite_plane_stays_in_its_plane(blocks, dtype, axis, nx, ny, g, state, exact):
    """Plane 4 with one NaN and one +inf in real cells: planes 1 to 3 of that launch are bit for bit those of the launch
    without them. In exact arithmetic the set of non-finite cells of plane 4 is the restatement's (the sets, not the payloads)."""
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    f = SS.input_of(state, nx, ny, g, axis, dtype)
    clean = SP.special_planes(state, nx, ny, g, axis, dtype)
    dirty = list(clean[:3]) + [SP.poisoned(state, nx, ny, g, axis, dtype)]
    assert all(inside[c] for c in SP.poison_cells(nx, ny, g, axis)) and not np.isfinite(dirty[3]).all()
    dt, _dx = SS.step_of((nx, ny)[axis], dtype)
    for triple in SS.TRIPLES:
        opts = options(axis, triple)
        what = f"{'exact' if exact else 'tuned'} {SS.STATES[state]} {'-'.join(triple)}: "
        blk.upload(f)
        outs = []
        for planes in (clean, dirty):
            P = Planes(blk, 4)
            try:
                blk.mark_outputs()
                P.upload(planes)
                launch(blk, descriptor(blk, *opts, exact, dt, **WALLS), P.inp, P.out)
                outs.append(P.fetch()[1])
            finally:
                P.free()
        for k in range(3):
            assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), f"{what}plane {k + 1} changed with a non-finite plane 4"
        spoilt = ~np.isfinite(outs[1][3]) & inside
        assert spoilt.any(), what + "the non-finite values vanished"
        if exact:
            want = SP.restated_planes(state, nx, ny, g, axis, triple, dtype, walls=True, poison=True)[3]
            wrong = np.flatnonzero(spoilt != (~np.isfinite(want) & inside))
            assert wrong.size == 0, (f"{what}{wrong.size} cells of plane 4 are finite on one side only, first at flat index {wrong[0]}: "
                                     f"{outs[1][3][wrong[0]]!r} against the restatement's {want[wrong[0]]!r}")
