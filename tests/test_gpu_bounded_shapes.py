"""armon_hip_sweep_scalars_bounded in exact arithmetic on the shapes at which the launch geometry of the scalar
sweep changes, against its restatement (tests/bounded_restated.py), bit for bit, both precisions. The bounded and the remap
launch share their text (csrc/scalar_sweep.hpp), but the bounded rule's clamp reads phi of the cells i - 1 and i + 1 of every
cell it emits — at the strip and run thresholds and at ``bc = 0`` sides, where the remap rule does not.

The shapes are the fixed list of tests/test_gpu_scalars_shapes.py (X_FIXED x X_ROWS, Y_ROWS, Y_LANES x Y_GHOSTS: its docstring
says what each reaches), without its random draw. Scheme and limiter, projection, EOS, bc pair and ns are dealt from the decks
of tests/test_gpu_scalars.py, the (scheme and limiter, projection) pairs, the bc pairs and ns from one deck per axis, so that,
per precision and whatever the seed (ARMON_RANDOM_SEED): every value of every option occurs; all four (scheme, projection) pairs
— on which the ring slots of ScalarMarch::step_bounded depend — and every bc pair occur on each axis; ns = 2 and ns = 3, the
template instances no other exact test of the bounded rule launches, each meet both axes. ``draw_cases`` asserts it.

The checks are those of tests/test_gpu_bounded.py::test_exact_bounded_sweep_is_the_restatement: the restatement's bits on the
real cells, the marker elsewhere, inputs and state untouched, plane k of the ns-launch equal to its own ns = 1 launch; and cell
by cell the range of the input at i - 1, i, i + 1, the ghosts as given at ``bc = 0`` sides."""
import itertools
import os
import random

import pytest

import bounded_planes as BP
from bounded_restated import bounded_sweep
from scalars_harness import bounded_launch, case_numbers, exact_launch_is_the_restatement, lag_of, rand_planes
from sweep_harness import F_HIGH, F_LOW, block_cache
from sweep_reference import rand_state, real_mask
from test_gpu_scalars import BCS, DTYPES, EOSES, PROJECTIONS, SCHEMES
from test_gpu_scalars_shapes import LAG, NSS, X_FIXED, X_ROWS, Y_GHOSTS, Y_LANES, Y_ROWS

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("ARMON_RANDOM_SEED", "20261021"))
RULES = list(itertools.product(SCHEMES, PROJECTIONS))        # ((scheme, limiter), projection)


def draw_cases(seed):
    rng = random.Random(seed + 417)
    decks = {}

    def deal(name, values):
        if not decks.get(name):
            decks[name] = list(values)
            rng.shuffle(decks[name])
        return decks[name].pop()

    cases = []
    for dtype in DTYPES:
        def case(axis, nx, ny, g):
            (scheme, limiter), projection = deal(dtype + f"rule{axis}", RULES)
            lag = lag_of(scheme, projection)
            nx, ny, g = (lag if v == LAG else v for v in (nx, ny, g))
            cases.append(dict(dtype=dtype, axis=axis, nx=nx, ny=ny, g=g, scheme=scheme, limiter=limiter, projection=projection,
                              eos=deal(dtype + "eos", EOSES), bc=deal(dtype + f"bc{axis}", BCS), ns=deal(dtype + f"ns{axis}", NSS),
                              seed=rng.randint(0, 10 ** 6), lag=lag))

        for nx, g in X_FIXED:
            case(0, nx, deal(dtype + "rows", X_ROWS), g)
        for ny in Y_ROWS:
            case(1, 70, ny, deal(dtype + "g", (4, 5)))
        for g in Y_GHOSTS:
            for lanes in Y_LANES:
                case(1, lanes - g % 16, 37, g)

    for dtype in DTYPES:
        mine = [c for c in cases if c["dtype"] == dtype]
        assert {(c["scheme"], c["limiter"]) for c in mine} == set(SCHEMES)
        for key, values in (("projection", PROJECTIONS), ("eos", EOSES), ("bc", BCS), ("ns", NSS)):
            assert {c[key] for c in mine} == set(values), (dtype, key)
        for axis in (0, 1):
            there = [c for c in mine if c["axis"] == axis]
            assert {(c["scheme"], c["projection"]) for c in there} == set(itertools.product(("GAD", "Godunov"), PROJECTIONS)), (dtype, axis)
            assert {c["bc"] for c in there} == set(BCS), (dtype, axis)
            assert {2, 3} <= {c["ns"] for c in there}, (dtype, axis)
        shapes = {(c["axis"], c["nx"], c["g"]) for c in mine} | {(c["axis"], c["ny"]) for c in mine}
        assert {(0, nx, g) for nx, g in X_FIXED} <= shapes and {(1, ny) for ny in Y_ROWS} <= shapes
        assert {(1, lanes - g % 16, g) for g in Y_GHOSTS for lanes in Y_LANES} <= shapes
        rows = {c["ny"] for c in mine if c["axis"] == 0}
        assert {5, 9} <= rows and any(c["ny"] == c["lag"] for c in mine if c["axis"] == 0), (dtype, rows)
        assert all(c["g"] >= max(c["lag"], 4) and c["nx"] >= c["lag"] and c["ny"] >= c["lag"] for c in mine)
    return cases


def case_id(c):
    return (f"{c['dtype']}-{'XY'[c['axis']]}-{c['nx']}x{c['ny']}-g{c['g']}-{c['scheme']}-{c['limiter']}-{c['projection']}-{c['eos']}-"
            f"bc{c['bc'][0]}{c['bc'][1]}-ns{c['ns']}")


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


@pytest.mark.parametrize("case", draw_cases(SEED), ids=case_id)
def test_exact_bounded_sweep_of_a_threshold_shape_is_the_restatement(blocks, case):
    c = case
    nx, ny, g, axis = c["nx"], c["ny"], c["g"], c["axis"]
    opts = (axis, c["scheme"], c["limiter"], c["projection"], c["eos"])
    f = rand_state(nx, ny, g, c["eos"], c["dtype"], c["seed"])
    planes = rand_planes(nx, ny, g, c["ns"], c["dtype"], c["seed"] + 1)
    dt, dx = case_numbers(nx, ny, axis, c["eos"], c["dtype"])
    want, _, _ = bounded_sweep(f, planes, nx, ny, g, *opts, dt, dx, c["bc"][0], c["bc"][1], F_LOW, F_HIGH, c["dtype"])
    got = exact_launch_is_the_restatement(blocks(nx, ny, g, c["dtype"]), f, planes, want, *opts, dt, bc=c["bc"], launch=bounded_launch)
    inside = real_mask(nx, ny, g, axis)
    for k in range(c["ns"]):
        BP.assert_in_local_range(got[k], planes[k], inside, nx, ny, g, axis, c["bc"], what=f"plane {k}: ")
