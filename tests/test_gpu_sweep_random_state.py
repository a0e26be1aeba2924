"""armon_hip_sweep on random states against a single sweep of the CPU oracle (tests/sweep_reference.py).

The physical test cases leave the walls quiescent, their states piecewise constant and the mirror factors at the three pairs
the cases have; here every cell of the ghosted block differs from its neighbours, both velocities take both signs, the two
sides of the sweep axis are switched between mirror and halo independently with factor pairs that differ in both components
and between the sides, and every output array starts as a marker (a NaN with a payload, compared as integers), so that what
a sweep writes — and what it must leave alone — is checked cell by cell:

 * rho, u, v, E, p_out, c_out: the real cells with out_lo <= i < out_hi along the sweep axis, nothing else;
 * dt_cfl_out: one element.

Shapes: the smallest at which each launch form has more than one unit in both directions and a partial last one. X sweep: 120
result cells per wave strip, 4 rows (fp64) or 4 strips (fp32) per workgroup, row-by-row strip origins when the pitch is not a
multiple of a 64-B sector, the narrow form for pieces of at most 8 cells. Y march: 256 lanes (512 with the store exchange)
times 1 or 2 columns per lane, runs of 32 rows at these sizes. Ghost widths 4, 5, 6: even / odd pitch and ghost width, which
the fp32 rule for two columns per lane reads.

Mirror factors are +1 / -1 only: the fused sweep refuses anything else (include/armon_hip.h, armon_sweep_desc), which
test_mirror_factors_other_than_unit_magnitude_are_refused pins.

Tuned arithmetic: test_tuned_forms_agree_and_stay_within_the_rounding_of_the_operation prints what it measures (run with -s).
"""
import functools
import os
import random

import numpy as np
import pytest

from sweep_harness import (F_HIGH, F_LOW, MARKER, OUT_NAMES, TUNED_DEFAULTS, TUNED_FORMS, Block, bits, block_cache, check_outputs,
                           run_tuned_forms)
from sweep_reference import STATE, rand_dt, rand_state, real_mask, reference_sweep

pytestmark = pytest.mark.gpu

SEED = int(os.environ.get("ARMON_RANDOM_SEED", "20261017"))
N_CASES = int(os.environ.get("ARMON_RANDOM_CASES", "36"))

X_SHAPES = [(250, 9), (1004, 6), (123, 5)]
Y_SHAPES = [(1100, 70), (530, 37), (70, 101)]
SHAPES = {0: X_SHAPES, 1: Y_SHAPES}
GHOSTS = (4, 5, 6)
DTYPES = ("float64", "float32")
SCHEMES = [("GAD", "minmod"), ("GAD", "superbee"), ("GAD", "no_limiter"), ("Godunov", "minmod")]
PROJECTIONS = ["euler", "euler_2nd"]
EOSES = ["perfect_gas", "bizarrium"]
EMITS = [(0, 0), (1, 0), (0, 1), (1, 1)]                  # (p_out, c_out)


def lag_of(scheme, projection):
    return 2 + (scheme == "GAD") + (projection == "euler_2nd")


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


# ---- the reference, computed once per case and shared ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def state_of(nx, ny, g, eos, dtype, seed):
    f = rand_state(nx, ny, g, eos, dtype, seed)
    for a in f.values():
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(nx, ny, g, axis, scheme, limiter, projection, eos, dtype, seed, bc=(1, 1), ref_dtype=None, plant=None):
    """(input state in ``dtype``, sweep of the oracle in ``ref_dtype`` on that very input, dt). The CFL reduction takes the
    cell sizes of the unit square, 1 / nx and 1 / ny; with ``plant`` (see plant_cell) the size along the axis for both."""
    f = state_of(nx, ny, g, eos, dtype, seed)
    if plant is not None:
        f = plant_cell(f, nx, ny, g, axis, eos, plant)
    T = np.dtype(dtype).type
    cs = [float(T(1.) / T(nx)), float(T(1.) / T(ny))]            # ArmonParameters.cell_size of the unit square
    dt = float(np.float32(rand_dt(eos, cs[axis])))                # the same number in either precision
    rd = np.dtype(ref_dtype or dtype)
    fin = {k: f[k].astype(rd) for k in STATE}
    cfl = cs if plant is None else [cs[axis]] * 2
    ref = reference_sweep(fin, nx, ny, g, axis, scheme, limiter, projection, eos, dt, cs[axis], bc[0], bc[1], F_LOW, F_HIGH, rd,
                          cfl_dx=cfl[0], cfl_dy=cfl[1])
    for k in OUT_NAMES:
        assert np.isfinite(getattr(ref, k).reshape(ny + 2 * g, -1)[g:g + ny, g:g + nx]).all(), k     # a usable reference
    return f, ref, dt


# ---- the yardstick of the tuned arithmetic ---------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def kappa_of(nx, ny, g, axis, scheme, limiter, projection, eos, seed, bc=(1, 1)):
    """Per field, max|oracle32 - oracle64| / (eps32 max|oracle64|) over the real cells: how many fp32 roundings of the field
    maximum the operation itself costs when every step is rounded once. Both oracles take the SAME numbers — the state, the
    cell size and the step rounded to fp32 — so no rounding of the input is counted; an fp64 case shares the value of its fp32
    twin. From the two oracles alone: nothing the kernels compute enters."""
    opts = (axis, scheme, limiter, projection, eos)
    _f, o64, _dt = reference(nx, ny, g, *opts, "float32", seed, bc=bc, ref_dtype="float64")
    _f, o32, _dt = reference(nx, ny, g, *opts, "float32", seed, bc=bc, ref_dtype="float32")
    inside = real_mask(nx, ny, g, axis)
    eps32 = float(np.finfo(np.float32).eps)
    kappa = {}
    for k in OUT_NAMES:
        a64 = getattr(o64, k)[inside]
        kappa[k] = float(np.abs(getattr(o32, k)[inside].astype(np.float64) - a64).max() / (eps32 * np.abs(a64).max()))
        assert kappa[k] > 0.5, (k, kappa[k])                # a yardstick, not an accident of one cell
    return kappa


def assert_within_rounding(blk, out, ref64, kappa, axis, what):
    """rho, u, v, E, p, c of a tuned sweep: at most 4 kappa eps_P of the field maximum from the fp64 reference on the input the
    kernel got. dt_cfl_out = min(dx / max(|u| + c), dy / max(|v| + c)): with u, v, c within their bounds each maximum moves by
    at most 4 eps (kappa_u max|u| + kappa_c max c) <= 8 max(kappa_u, kappa_c) eps max(|u| + c), as max(|u| + c) is at least
    max|u| and at least max c; the sum and the quotient (a reciprocal and a product in tuned arithmetic) add 2 eps: relative
    bound (8 max(kappa_u, kappa_v, kappa_c) + 2) eps. Prints what it measures (pytest -s); returns the worst share of a bound."""
    inside = blk.written_mask(axis, 0, (blk.nx, blk.ny)[axis])
    eps = float(np.finfo(blk.dtype).eps)
    measured = {}
    for k in OUT_NAMES:
        want = getattr(ref64, k)[inside].astype(np.float64)
        measured[k] = float(np.abs(out[k][inside].astype(np.float64) - want).max() / (eps * np.abs(want).max())), 4 * kappa[k]
    want = float(ref64.cfl())
    measured["dt"] = abs(float(out["dt"][0]) - want) / (eps * want), 8 * max(kappa["u"], kappa["v"], kappa["c"]) + 2
    print(f"\n{what}: " + ", ".join(f"{k} {r:.2f} eps (kappa {kappa[k]:.2f}: {r / kappa[k]:.2f} of it)" if k != "dt" else
                                     f"dt {r:.2f} eps (bound {b:.1f})" for k, (r, b) in measured.items()))
    for k, (r, b) in measured.items():
        assert r <= b, f"{what}: {k} is {r:.2f} eps of the field maximum from the fp64 reference, bound {b:.2f}"
    return max(r / b for r, b in measured.values())


# ---- a. exact arithmetic: the reference's bits --------------------------------------------------------------------------

def draw_exact_cases(seed, count):
    """``count`` cases dealt over precision x axis x shape in turn; every option comes from a shuffled deck that is refilled
    when empty, so each value of each option occurs, and occurs for each precision."""
    rng = random.Random(seed)
    decks = {}

    def deal(name, values):
        if not decks.get(name):
            decks[name] = list(values)
            rng.shuffle(decks[name])
        return decks[name].pop()

    combos = [(dt, ax, sh) for dt in DTYPES for ax in (0, 1) for sh in range(3)]
    cases = []
    for k in range(count):
        dtype, axis, sh = combos[k % len(combos)]
        nx, ny = SHAPES[axis][sh]
        scheme, limiter = deal(dtype + "scheme", SCHEMES)
        cases.append(dict(dtype=dtype, axis=axis, nx=nx, ny=ny, g=deal(dtype + "g", GHOSTS), scheme=scheme, limiter=limiter,
                          projection=deal(dtype + "proj", PROJECTIONS), eos=deal(dtype + "eos", EOSES),
                          emit=deal(dtype + "emit", EMITS), seed=rng.randint(0, 10 ** 6)))
    for dtype in DTYPES:                                   # what the issue of this test asks of the draw
        mine = [c for c in cases if c["dtype"] == dtype]
        assert {c["axis"] for c in mine} == {0, 1}
        assert {(c["scheme"], c["limiter"]) for c in mine} == set(SCHEMES)
        for key, values in (("projection", PROJECTIONS), ("eos", EOSES), ("emit", EMITS), ("g", GHOSTS)):
            assert {c[key] for c in mine} == set(values), (dtype, key)
    return cases


def case_id(c):
    return (f"{c['dtype']}-{'XY'[c['axis']]}-{c['nx']}x{c['ny']}-g{c['g']}-{c['scheme']}-{c['limiter']}-{c['projection']}-"
            f"{c['eos']}-p{c['emit'][0]}c{c['emit'][1]}")


@pytest.mark.parametrize("case", draw_exact_cases(SEED, N_CASES), ids=case_id)
def test_exact_sweep_of_a_random_state_is_the_oracles(blocks, case):
    """rho, u, v, E, p_out, c_out (in the four emit combinations) and dt_cfl_out of one exact sweep with both sides mirrored:
    the oracle's bits on the cells a sweep writes, the marker everywhere else."""
    c = case
    blk = blocks(c["nx"], c["ny"], c["g"], c["dtype"])
    opts = (c["axis"], c["scheme"], c["limiter"], c["projection"], c["eos"])
    f, ref, dt = reference(c["nx"], c["ny"], c["g"], *opts, c["dtype"], c["seed"])
    blk.upload(f)
    blk.mark_outputs()
    blk.sweep(*opts, True, dt, emit=c["emit"])
    check_outputs(blk, blk.fetch(), ref, c["axis"], emit=c["emit"])
    blk.mark_outputs()                                     # ... and without the reduction: the same cells, no scalar
    blk.sweep(*opts, True, dt, emit=c["emit"], emit_dt=False)
    check_outputs(blk, blk.fetch(), ref, c["axis"], emit=c["emit"], emit_dt=False)


# ---- b. boundaries -------------------------------------------------------------------------------------------------------

def garbage_ghosts(f, nx, ny, g, axis, bc, dtype):
    """The state with 1e100 (fp32: +inf) in the ghost cells of the mirrored sides and in every ghost cell across the axis,
    corners included: none of them may be read."""
    out = {}
    with np.errstate(over="ignore"):
        junk = np.dtype(dtype).type(1e100)
    for k in STATE:
        a = f[k].reshape(ny + 2 * g, nx + 2 * g).copy()
        keep = a[g:g + ny, g:g + nx].copy()
        lo_ghosts = a[g:g + ny, :g].copy() if axis == 0 else a[:g, g:g + nx].copy()
        hi_ghosts = a[g:g + ny, g + nx:].copy() if axis == 0 else a[g + ny:, g:g + nx].copy()
        a[:] = junk
        a[g:g + ny, g:g + nx] = keep
        if not bc[0]:                                      # a halo side: the neighbour's cells stay
            if axis == 0: a[g:g + ny, :g] = lo_ghosts
            else: a[:g, g:g + nx] = lo_ghosts
        if not bc[1]:
            if axis == 0: a[g:g + ny, g + nx:] = hi_ghosts
            else: a[g + ny:, g:g + nx] = hi_ghosts
        out[k] = a.ravel()
    return out


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("bc", [(1, 1), (1, 0), (0, 1), (0, 0)], ids=lambda b: f"bc{b[0]}{b[1]}")
@pytest.mark.parametrize("shape", range(3))
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_side_mirrors_the_right_cell_with_the_right_factor_or_reads_its_halo(blocks, dtype, axis, shape, bc, exact):
    """The two sides switched independently between mirror (low (-1, 1), high (1, -1)) and halo (random ghost cells, as a
    neighbour's) on states whose cells all differ (tests/test_sweep_reference.py shows that swapped factors or sides are
    another sweep): the high side lies in the partial last strip of the X shapes and in the last, partial run of every
    workgroup column of the Y shapes. Exact arithmetic gives the reference's bits; tuned arithmetic, in every launch form
    (two columns per lane, store exchange: the forms exact arithmetic never takes), the same bits in all forms and the
    reference within the per-sweep bound of test d. Then the same sweep with 1e100 in every ghost cell a mirror replaces
    and in every ghost cell across the axis: not a bit changes."""
    nx, ny = SHAPES[axis][shape]
    g = GHOSTS[(shape + axis) % 3]
    blk = blocks(nx, ny, g, dtype)
    opts = (axis, "GAD", "minmod", "euler_2nd", "perfect_gas")
    seed = 4000 + shape
    junk = "garbage in the unread ghosts: "
    if exact:
        f, ref, dt = reference(nx, ny, g, *opts, dtype, seed, bc=bc)
        for state, what in ((f, ""), (garbage_ghosts(f, nx, ny, g, axis, bc, dtype), junk)):
            blk.upload(state)
            blk.mark_outputs()
            blk.sweep(*opts, True, dt, bc=bc, emit=(1, 1))
            check_outputs(blk, blk.fetch(), ref, axis, emit=(1, 1), what=what)
        return
    f, ref64, dt = reference(nx, ny, g, *opts, dtype, seed, bc=bc, ref_dtype="float64")
    blk.upload(f)
    out = run_tuned_forms(blk, opts, dt, bc, "")
    assert_within_rounding(blk, out, ref64, kappa_of(nx, ny, g, *opts, seed, bc=bc), axis,
                           f"tuned {dtype} {'XY'[axis]} {nx}x{ny} g{g} bc{bc[0]}{bc[1]}")
    blk.upload(garbage_ghosts(f, nx, ny, g, axis, bc, dtype))
    again = run_tuned_forms(blk, opts, dt, bc, junk)
    for k in OUT_NAMES + ("dt",):
        assert np.array_equal(bits(again[k]), bits(out[k])), junk + k


def test_mirror_factors_other_than_unit_magnitude_are_refused(blocks):
    """The in-tile mirror evaluates the EOS of a ghost cell from the scaled velocities, the reference copies p and c: equal
    for factors of magnitude 1 only, and the entry point says so instead of computing something else."""
    nx, ny = X_SHAPES[2]
    blk = blocks(nx, ny, 4, "float64")
    f, _ref, dt = reference(nx, ny, 4, 0, "GAD", "minmod", "euler_2nd", "perfect_gas", "float64", 4002)
    blk.upload(f)
    for axis in (0, 1):
        blk.mark_outputs()
        blk.sweep(axis, "GAD", "minmod", "euler_2nd", "perfect_gas", True, dt, f_high=(0.5, -2.), expect=1)
        blk.sweep(axis, "GAD", "minmod", "euler_2nd", "perfect_gas", True, dt, f_low=(-1., 2.), expect=1)
        assert b"factor" in blk.dev._L.armon_hip_last_error()
        out = blk.fetch()
        for k in OUT_NAMES:
            assert (bits(out[k]) == MARKER["float64"]).all(), k           # refused before anything was launched
        # a halo side's factors are not read
        blk.sweep(axis, "GAD", "minmod", "euler_2nd", "perfect_gas", True, dt, bc=(1, 0), f_high=(0.5, -2.))
    blk.dev.wait()


# ---- c. partial sweeps write their piece and nothing else --------------------------------------------------------------------

def pieces_of(axis, n, lag):
    """An interior piece, one cell (in the middle and at either end), 8 cells at either end, and a piece that straddles a
    seam. X: strips of 120 cells start less than 16 cells below out_lo, so [1, 123) and anything longer holds a seam; Y: a
    piece of more than 32 rows is a run of 32 and a shorter one."""
    ps = [(lag, n - lag), (n // 2, n // 2 + 1), (0, 1), (n - 1, n), (0, 8), (n - 8, n)]
    ps.append((1, min(n, 132)) if axis == 0 else (2, min(n, 42)))
    return ps


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("shape", range(3))
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_partial_sweep_writes_its_piece_and_nothing_else(blocks, dtype, axis, shape, exact):
    """After every piece every cell of every output array outside (real cells x [out_lo, out_hi) along the axis) still holds
    the marker, every cell inside does not (exact arithmetic: it holds the full sweep's bits, and dt_cfl_out the minimum over
    the piece); arrays that were not asked for stay untouched."""
    nx, ny = SHAPES[axis][shape]
    g = GHOSTS[(shape + axis + 1) % 3]
    blk = blocks(nx, ny, g, dtype)
    scheme, limiter, projection = [("GAD", "superbee", "euler_2nd"), ("Godunov", "minmod", "euler"), ("GAD", "minmod", "euler")][shape]
    opts = (axis, scheme, limiter, projection, "perfect_gas")
    f, ref, dt = reference(nx, ny, g, *opts, dtype, 5000 + shape)
    blk.upload(f)
    n = (nx, ny)[axis]
    for k, (lo, hi) in enumerate(pieces_of(axis, n, lag_of(scheme, projection))):
        emit = EMITS[k % 4]
        blk.mark_outputs()
        blk.sweep(*opts, exact, dt, emit=emit, out_range=(lo, hi))
        check_outputs(blk, blk.fetch(), ref, axis, lo, hi, emit=emit, exact=exact, what=f"piece [{lo}, {hi}): ")


# ---- d. tuned arithmetic ------------------------------------------------------------------------------------------------

TUNED_CASES = [(dtype, axis, shape, g, scheme, limiter, projection, eos)
               for dtype in DTYPES for axis in (0, 1) for shape in range(3)
               for g, (scheme, limiter, projection, eos) in [[
                   (4, ("GAD", "minmod", "euler_2nd", "perfect_gas")), (6, ("GAD", "superbee", "euler_2nd", "bizarrium")),
                   (5, ("Godunov", "minmod", "euler", "perfect_gas"))][shape]]]
# the fp32 two-columns-per-lane march needs an even nx and an even ghost width: the Y shapes with g = 4 and g = 6 take it,
# (70, 101) with g = 5 cannot; one more case gives that shape both forms
TUNED_CASES.append(("float32", 1, 2, 4, "GAD", "no_limiter", "euler", "perfect_gas"))


@pytest.mark.parametrize("dtype,axis,shape,g,scheme,limiter,projection,eos", TUNED_CASES,
                         ids=lambda v: v if isinstance(v, str) else str(v))
def test_tuned_forms_agree_and_stay_within_the_rounding_of_the_operation(blocks, dtype, axis, shape, g, scheme, limiter,
                                                                          projection, eos):
    """Tuned arithmetic (what the benchmark runs), one sweep of a random state, both sides mirrored.

    Every form gives the same bits: the X sweep with either workgroup shape (ARMON_X_ROWS), the Y march with the store
    exchange forced on and off (ARMON_Y_SX) and, in fp32, with two columns per lane and with one (ARMON_Y_COLS1).

    Accuracy, in the precision's own units and with a yardstick that comes from the reference alone (kappa_of): for each field
    kappa = max|oracle32 - oracle64| / (eps32 max|oracle64|), both oracles on the fp32 rounding of this very input — how many
    roundings of the field maximum the operation itself costs when every step is rounded once. The tuned result in precision
    P may deviate from the fp64 reference (fp32: the fp64 oracle on the fp32 input; fp64: the exact oracle on the fp64 input)
    by at most 4 kappa eps_P max|field|: a shared reciprocal is within 1 ulp where a division is within 1/2, it is reused in
    a product, and FMA contraction changes which rounding is taken. dt_cfl_out: the bound that follows from those of u, v and
    c (assert_within_rounding).

    kappa of the cases of this file (test b included): 0.85-2.1 for rho, u, v, E, p, c of a perfect gas; Bizarrium 0.87-3.6
    for the state and 8.1-10.2 for p and c (its sound speed is the root of a difference of 1e10-sized terms).
    The deviations of the tuned kernels, as a share of kappa (the bound is 4), are printed by this test (pytest -s); no
    measured figures are recorded here."""
    nx, ny = SHAPES[axis][shape]
    blk = blocks(nx, ny, g, dtype)
    opts = (axis, scheme, limiter, projection, eos)
    seed = 6000 + shape
    f, ref64, dt = reference(nx, ny, g, *opts, dtype, seed, ref_dtype="float64")
    blk.upload(f)
    out = run_tuned_forms(blk, opts, dt, (1, 1), "")
    assert_within_rounding(blk, out, ref64, kappa_of(nx, ny, g, *opts, seed), axis,
                           f"tuned {dtype} {'XY'[axis]} {nx}x{ny} g{g} {scheme} {limiter} {projection} {eos}")


# ---- e. the CFL reduction finds one decisive cell wherever it sits -----------------------------------------------------------

def plant_cell(f, nx, ny, g, axis, eos, pos):
    """A copy of ``f`` whose cell ``pos`` (real coordinates) moves fast ACROSS the sweep axis — that velocity is only
    advected by the sweep, so the cell keeps the largest wave speed — with its total energy raised by the kinetic energy
    added, so that the internal energy (and the EOS) stays what it was."""
    out = {k: a.copy() for k, a in f.items()}
    i = (pos[1] + g) * (nx + 2 * g) + pos[0] + g
    ut = "v" if axis == 0 else "u"
    T = out[ut].dtype.type
    new = T(-2400. if eos == "bizarrium" else -8.)
    out["E"][i] += T(0.5) * (new * new - out[ut][i] * out[ut][i])
    out[ut][i] = new
    return out


def cfl_positions(axis, nx, ny):
    """First and last real cell; X: the last lane of the partial last strip in a middle row and the first cell of the second
    strip; Y: the first row of the second and of the last run in a column of the second workgroup (or the last column)."""
    ps = [(0, 0), (nx - 1, ny - 1)]
    if axis == 0:
        ps += [(nx - 1, ny // 2), (120, ny - 1)]
    else:
        x = min(nx - 1, 300)
        ps += [(x, 32), (x, 32 * ((ny - 1) // 32))]
    return ps


@pytest.mark.parametrize("where", range(4))
@pytest.mark.parametrize("shape", range(3))
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cfl_reduction_finds_the_one_decisive_cell(blocks, dtype, axis, shape, where):
    """One cell carries the minimum (asserted on the reference: its own step is smaller than every other cell's). dt_cfl_out
    of a full sweep is the reference's; and so is the minimum accumulated (dt_accumulate) over the sweep produced as a LAG-wide
    piece at either end and the interior between them, whichever of the three holds the cell."""
    nx, ny = SHAPES[axis][shape]
    g = GHOSTS[(shape + where) % 3]
    pos = cfl_positions(axis, nx, ny)[where]
    blk = blocks(nx, ny, g, dtype)
    scheme, limiter, projection = "GAD", "minmod", "euler_2nd"
    opts = (axis, scheme, limiter, projection, "perfect_gas")
    f, ref, dt = reference(nx, ny, g, *opts, dtype, 7000 + shape, plant=pos)
    # the planted cell decides: the reduction over everything but its row / column along the axis is larger
    n, lag = (nx, ny)[axis], lag_of(scheme, projection)
    a = pos[axis]
    assert ref.cfl(a, a + 1) == ref.cfl() and (a == 0 or ref.cfl(0, a) > ref.cfl()) and (a == n - 1 or ref.cfl(a + 1, n) > ref.cfl())
    cfl = (blk.cell_size(axis),) * 2                       # the same size both ways: the fastest cell decides, along or across
    blk.upload(f)
    blk.mark_outputs()
    blk.sweep(*opts, True, dt, cfl_sizes=cfl)
    check_outputs(blk, blk.fetch(), ref, axis)
    blk.mark_outputs()
    for k, piece in enumerate([(lag, n - lag), (0, lag), (n - lag, n)]):
        blk.sweep(*opts, True, dt, out_range=piece, accumulate=k > 0, cfl_sizes=cfl)
    check_outputs(blk, blk.fetch(), ref, axis)             # the three pieces together are the full sweep, bit for bit


# ---- f. within one flavour the X sweep and the Y march are the same function ---------------------------------------------------

# X on nx x ny against Y on ny x nx: three strips of 120 cells, the last partial, against eight runs of 32 rows, the last
# partial, one column per lane; one partial strip against three workgroups of 256 columns and two runs (fp32: two columns per lane)
TRANSPOSED_SHAPES = [(250, 9), (37, 530)]
TRANSPOSED_OPTIONS = [("GAD", "minmod", "euler_2nd", "perfect_gas"), ("GAD", "superbee", "euler_2nd", "bizarrium"),
                      ("Godunov", "minmod", "euler", "perfect_gas")]


@pytest.mark.parametrize("scheme,limiter,projection,eos", TRANSPOSED_OPTIONS, ids=lambda v: v)
@pytest.mark.parametrize("shape", TRANSPOSED_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
def test_x_sweep_and_y_march_of_the_transposed_state_give_the_same_bits(blocks, exact, dtype, shape, scheme, limiter, projection,
                                                                        eos):
    """Within one flavour the X sweep and the Y march are the same function: the X sweep of a random state and the Y march of
    its transpose (u and v exchanged, the same cell size along the axis, both sides mirrored with the factors (-1, +1))
    give the same rho, u <-> v, E, p_out and c_out on every real cell, bit for bit. Tuned arithmetic: both forms call the
    same stage functions (csrc/sweep_stages.hpp) and differ only in where an operand comes from. Exact arithmetic: both
    state the reference's operations. (The one place where an operand order depends on the axis is the reference's
    u^2 + v^2 of the exact EOS, and IEEE addition commutes.) Passes on the parent of the commit that added it, too: the
    four copies of the arithmetic had not drifted."""
    nx, ny = shape
    g = 4
    seed = 8000 + TRANSPOSED_SHAPES.index(shape)
    f = state_of(nx, ny, g, eos, dtype, seed)
    bx, by = blocks(nx, ny, g, dtype), blocks(ny, nx, g, dtype)
    assert bx.cell_size(0) == by.cell_size(1)
    dt = float(np.float32(rand_dt(eos, bx.cell_size(0))))
    mirror = dict(bc=(1, 1), f_low=(-1., 1.), f_high=(-1., 1.), emit=(1, 1))

    def transposed(a, shape_of_a):
        return np.ascontiguousarray(a.reshape(shape_of_a).T).ravel()

    bx.upload(f)
    bx.mark_outputs()
    bx.sweep(0, scheme, limiter, projection, eos, exact, dt, **mirror)
    along_x = bx.fetch()
    rows_x = (ny + 2 * g, nx + 2 * g)
    by.upload({k: transposed(f[{"u": "v", "v": "u"}.get(k, k)], rows_x) for k in STATE})
    by.mark_outputs()
    by.sweep(1, scheme, limiter, projection, eos, exact, dt, **mirror)
    along_y = by.fetch()
    inside = real_mask(nx, ny, g, 0)
    mark = MARKER[np.dtype(dtype).name]
    for k in OUT_NAMES:
        want = bits(along_x[k])[inside]
        got = bits(transposed(along_y[{"u": "v", "v": "u"}.get(k, k)], rows_x[::-1]))[inside]
        assert (want != mark).all() and (got != mark).all(), k
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{k}: {bad.size} of {want.size} real cells differ between the X sweep and the Y march"
