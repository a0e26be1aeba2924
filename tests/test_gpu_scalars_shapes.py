"""armon_hip_sweep_scalars in exact arithmetic on the shapes at which its launch geometry changes (csrc/scalar_sweep.hpp),
against the restatement (tests/scalars_restated.py), bit for bit, both precisions. The checks are those of
test_exact_scalar_sweep_is_the_restatement (tests/test_gpu_scalars.py): phi_out is the restatement on the real cells and the
marker elsewhere; phi_in, the state, p, c and dt are untouched; plane k of an ns-launch is the ns = 1 launch on it.

A fixed list, present whatever the seed, and what each shape reaches:

X sweep, k_scalar_x: a wave produces the 120 cells [w0, w0 + 120) of a row, w0 = x_first + 120 blockIdx.x with
x_first = -(nghost % 8); lane l holds the cells j0 = w0 - 4 + 2 l and j0 + 1. grid.x = ceil((nx - x_first) / 120), so the last
strip always begins below nx: the ``w0 >= a.o_hi`` half of the early return is never true in a launch of scalar_launch, and
nx = 116 with nghost 4 is instead the block whose only strip ends exactly at nx (``hi = w0 + STRIDE``).

 nghost 4  nx 116       one strip, ``hi = w0 + STRIDE == o_hi``
 (-4)      nx 117       a second strip that produces one cell; odd pitch, no ``vec``
           nx 118       a last strip of two cells: one ``vec`` pair stored after a clamped load (even pitch)
           nx 120, 121  a last strip of 4 and 5 cells, even and odd pitch
           nx 236       two strips, the second ends exactly at nx; 237: a third strip of one cell
           nx 244       the smallest block with a strip loaded by the uniform ``vec`` branch (``cb + WIDTH <= nx``: 112 + 128 <= 244)
 nghost 5  nx 114       even pitch with odd strip origins: the lane pair (-1, 0) straddles ``lo`` and the pair (113, 114)
 (-5)                   straddles ``hi``: both take the scalar stores of the ``else`` branch inside a ``vec`` launch
           nx 115       one strip that ends exactly at nx, odd pitch
           nx 116       a second strip of one cell whose pair (115, 116) straddles ``hi``
           nx 250       three strips; the middle one takes the uniform ``vec`` loads at an odd j0 (the case (250, 9) of
                        tests/test_gpu_scalars.py meets nghost 5 only if the shuffle says so)
 nghost 8  nx 120       ``x_first = 0``: one strip, exactly; 121: a second strip of one cell; 128: one wave's whole load width,
 (0)                    a second strip of 8 cells, the first strip's ``cb = -4 < 0`` keeps it off the uniform branch
 nghost 9  nx 119       ``x_first = -1``: one strip, exactly, odd pitch; 120: a second strip of one cell, even pitch, the pair
 (-1)                   (-1, 0) straddles ``lo``
 ny        LAG, 5, 9    the smallest block; two workgroups of kSXRows = 4 rows, the second with one row; three with one row

Y sweep, k_scalar_y: 256 columns per workgroup, lane = column + xshift with xshift = nghost % 16; runs of ``seg`` rows,
seg = 32 for a block this small on any device of at least 8 CUs (scalar_y_seg), or ny if ny < 32.

 nx 70     ny 31        ``seg = ny < 32``: one run, other than LAG
           ny 32, 64    runs that end exactly at ny
           ny 33, 65    a last run of one row: T = 2 LAG + 1 steps, ``plain_end <= 1``, no unchecked stretch (``M = P``), the
                        mirror rows inside the run; its checked store guard ``o >= o0 && o < o1`` passes one step only
           ny 63, 97    a last run of 31 rows and one of one row after three full ones
 ny 37     nx + xshift  at nghost 4, 5 (xshift 4, 5) and 16 (``xshift = 0``):
           63           one wave with an idle tail lane that shadows column nx - 1; three waves return ("no column at all")
           64           one full wave; 65: a second wave with one column and 63 idle lanes
           255, 256     four waves, an idle tail lane / none; 257: a second workgroup with one column, three of its waves return
           320          a second workgroup of one full wave; 321: its second wave has one column

Schemes, projections, EOS and bc pairs are dealt from the decks of tests/test_gpu_scalars.py, ns from {1, 2, 3, 4}: the draw
asserts, per precision, that every value of every option occurs and that ns = 2 and ns = 3 each meet both axes (the template
instances of two and three planes are launched by no other exact test). On top a seeded random draw (ARMON_RANDOM_SEED,
ARMON_RANDOM_CASES per precision): nx in [LAG, 700], ny in [LAG, 400], nghost in {LAG, 4, ..., 9, 16, 17}."""
import os
import random

import pytest

from scalars_harness import case_numbers, exact_launch_is_the_restatement, lag_of, rand_planes
from scalars_restated import restated_sweep
from sweep_harness import F_HIGH, F_LOW, block_cache
from sweep_reference import rand_state
from test_gpu_scalars import BCS, DTYPES, EOSES, PROJECTIONS, SCHEMES

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("ARMON_RANDOM_SEED", "20261021"))
COUNT = int(os.environ.get("ARMON_RANDOM_CASES", "24"))
NSS = (1, 2, 3, 4)
LAG = "LAG"
X_FIXED = ([(nx, 4) for nx in (116, 117, 118, 120, 121, 236, 237, 244)] + [(nx, 5) for nx in (114, 115, 116, 250)] +
           [(nx, 8) for nx in (120, 121, 128)] + [(nx, 9) for nx in (119, 120)])
X_ROWS = (LAG, 5, 9)
Y_ROWS = (31, 32, 33, 63, 64, 65, 97)               # with nx = 70
Y_LANES = (63, 64, 65, 255, 256, 257, 320, 321)     # nx + nghost % 16, with ny = 37
Y_GHOSTS = (4, 5, 16)
RANDOM_GHOSTS = (LAG, 4, 5, 6, 7, 8, 9, 16, 17)


def draw_cases(seed, count):
    rng = random.Random(seed)
    decks = {}

    def deal(name, values):
        if not decks.get(name):
            decks[name] = list(values)
            rng.shuffle(decks[name])
        return decks[name].pop()

    cases = []
    for dtype in DTYPES:
        def case(axis, nx, ny, g, fixed=True):
            scheme, limiter = deal(dtype + "scheme", SCHEMES)
            projection = deal(dtype + "proj", PROJECTIONS)
            lag = lag_of(scheme, projection)
            nx, ny, g = (lag if v == LAG else v for v in (nx, ny, g))
            cases.append(dict(dtype=dtype, axis=axis, nx=nx, ny=ny, g=g, scheme=scheme, limiter=limiter, projection=projection,
                              eos=deal(dtype + "eos", EOSES), bc=deal(dtype + "bc", BCS), ns=deal(dtype + f"ns{axis}", NSS),
                              seed=rng.randint(0, 10 ** 6), fixed=fixed, lag=lag))

        for nx, g in X_FIXED:
            case(0, nx, deal(dtype + "rows", X_ROWS), g)
        for ny in Y_ROWS:
            case(1, 70, ny, deal(dtype + "g", (4, 5)))
        for g in Y_GHOSTS:
            for lanes in Y_LANES:
                case(1, lanes - g % 16, 37, g)
        for _ in range(count):
            case(rng.randint(0, 1), rng.randint(0, 700), rng.randint(0, 400), rng.choice(RANDOM_GHOSTS), fixed=False)
            c = cases[-1]                                    # nx in [LAG, 700], ny in [LAG, 400]
            c["nx"], c["ny"] = max(c["nx"], c["lag"]), max(c["ny"], c["lag"])

    for dtype in DTYPES:                                     # what the issue asks of the draw, whatever the seed
        mine = [c for c in cases if c["dtype"] == dtype and c["fixed"]]
        assert {(c["scheme"], c["limiter"]) for c in mine} == set(SCHEMES)
        for key, values in (("projection", PROJECTIONS), ("eos", EOSES), ("bc", BCS), ("ns", NSS)):
            assert {c[key] for c in mine} == set(values), (dtype, key)
        for ns in (2, 3):
            assert {c["axis"] for c in mine if c["ns"] == ns} == {0, 1}, (dtype, ns)
        shapes = {(c["axis"], c["nx"], c["g"]) for c in mine} | {(c["axis"], c["ny"]) for c in mine}
        assert {(0, nx, g) for nx, g in X_FIXED} <= shapes and {(1, ny) for ny in Y_ROWS} <= shapes
        assert {(1, lanes - g % 16, g) for g in Y_GHOSTS for lanes in Y_LANES} <= shapes
        rows = {c["ny"] for c in mine if c["axis"] == 0}
        assert {5, 9} <= rows and any(c["ny"] == c["lag"] for c in mine if c["axis"] == 0), (dtype, rows)
        assert all(c["g"] >= c["lag"] and c["nx"] >= c["lag"] and c["ny"] >= c["lag"] for c in cases)
    return cases


def case_id(c):
    return (f"{c['dtype']}-{'XY'[c['axis']]}-{c['nx']}x{c['ny']}-g{c['g']}-{c['scheme']}-{c['limiter']}-{c['projection']}-{c['eos']}-"
            f"bc{c['bc'][0]}{c['bc'][1]}-ns{c['ns']}" + ("" if c["fixed"] else "-drawn"))


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


@pytest.mark.parametrize("case", draw_cases(SEED, COUNT), ids=case_id)
def test_exact_scalar_sweep_of_a_threshold_shape_is_the_restatement(blocks, case):
    c = case
    nx, ny, g, axis = c["nx"], c["ny"], c["g"], c["axis"]
    opts = (axis, c["scheme"], c["limiter"], c["projection"], c["eos"])
    f = rand_state(nx, ny, g, c["eos"], c["dtype"], c["seed"])
    planes = rand_planes(nx, ny, g, c["ns"], c["dtype"], c["seed"] + 1)
    dt, dx = case_numbers(nx, ny, axis, c["eos"], c["dtype"])
    want, _ = restated_sweep(f, planes, nx, ny, g, *opts, dt, dx, c["bc"][0], c["bc"][1], F_LOW, F_HIGH, c["dtype"])
    narrow = dict(scheme=c["scheme"], projection=c["projection"]) if g < 4 else {}     # the default scheme asks for 4 ghost cells
    exact_launch_is_the_restatement(blocks(nx, ny, g, c["dtype"], **narrow), f, planes, want, *opts, dt, bc=c["bc"])
