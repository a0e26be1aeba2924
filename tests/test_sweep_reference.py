"""tests/sweep_reference.py, the single-sweep reference of the fused-sweep GPU tests, against the oracle's own solver (CPU only).

``oracle.solve(fields=f, skip_init=True, cst_dt=True, Dt=dt, maxcycle=1, axis_splitting="X_only" | "Y_only")`` is one sweep
of the oracle on whatever ``f`` holds, with the EOS and the mirrors of the named test case. The helper must give its bits."""
import numpy as np
import pytest

from sweep_reference import STATE, rand_dt, rand_state, real_mask, reference_sweep

# Dirichlet flag per side L, R, B, T of each test case (ref src/tests.jl:150-211): the velocity normal to such a side is
# mirrored with -1, everything else with +1
DIRICHLET = {"Sod": (1, 1, 0, 0), "Sod_circ": (1, 1, 1, 1), "Sedov": (0, 0, 0, 0), "Bizarrium": (1, 0, 1, 1)}
NX, NY, G = 133, 71, 5


def factors(test, axis):
    lo, hi = DIRICHLET[test][2 * axis:2 * axis + 2]
    return (-1. if lo else 1., 1.), (-1. if hi else 1., 1.)


def solve_one_sweep(oracle, test, f, axis, dt, dtype, **opts):
    d = oracle.alloc_fields(NX, NY, G, dtype=dtype)
    for k in STATE:
        d[k][:] = f[k]
    oracle.solve(test=test, N=(NX, NY), nghost=G, fields=d, skip_init=True, cst_dt=True, Dt=dt, maxcycle=1,
                 axis_splitting="X_only" if axis == 0 else "Y_only", data_type=dtype, **opts)
    return d


def cell_size(oracle, test, axis, dtype):
    return dtype(oracle.DEFAULTS[test]["domain"][axis]) / dtype((NX, NY)[axis])      # as armon_oracle_solve computes it


def assert_is_the_solvers_sweep(oracle, test, f, axis, dt, dtype, scheme, limiter, projection):
    eos = "bizarrium" if test == "Bizarrium" else "perfect_gas"
    dx = cell_size(oracle, test, axis, dtype)
    cfl_dx, cfl_dy = cell_size(oracle, test, 0, dtype), cell_size(oracle, test, 1, dtype)
    want = solve_one_sweep(oracle, test, f, axis, dt, dtype, scheme=scheme, riemann_limiter=limiter, projection=projection)
    f_low, f_high = factors(test, axis)
    got = reference_sweep(f, NX, NY, G, axis, scheme, limiter, projection, eos, dt, dx, 1, 1, f_low, f_high, dtype,
                          cfl_dx=cfl_dx, cfl_dy=cfl_dy)
    rv = lambda a: oracle.real_view(a, NX, NY, G)
    for k in STATE:
        assert np.isfinite(rv(want[k])).all(), k
        assert np.array_equal(rv(getattr(got, k)), rv(want[k])), k
    # p and c of the solver's arrays after its sweep are those of the state before it: nothing evaluates the EOS afterwards
    assert np.array_equal(rv(got.p), rv(want["p"])) and np.array_equal(rv(got.c), rv(want["c"]))
    # ... and they are what the next cycle's time step is reduced from
    L = oracle.lib(f32=np.dtype(dtype) == np.float32)
    step = L.armon_oracle_dtCFL(oracle.domain_range(NX, NY, G), cfl_dx, cfl_dy, *(oracle.ptr(want[k]) for k in ("u", "v", "c")))
    assert got.cfl() == dtype(step) and np.isfinite(step) and step > 0
    return got


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("scheme,limiter,projection", [("GAD", "minmod", "euler_2nd"), ("GAD", "superbee", "euler"),
                                                       ("GAD", "no_limiter", "euler_2nd"), ("Godunov", "minmod", "euler")])
@pytest.mark.parametrize("test", ["Sod", "Sod_circ", "Sedov", "Bizarrium"])
def test_reference_sweep_is_the_oracle_solvers_sweep_on_random_fields(oracle, test, scheme, limiter, projection, axis, dtype):
    """Random fields, ghosts included (the mirrors must overwrite them): every mirror combination the test cases have, both
    EOS, every limiter, both projections."""
    eos = "bizarrium" if test == "Bizarrium" else "perfect_gas"
    f = rand_state(NX, NY, G, eos, dtype, seed=17 + axis)
    dt = rand_dt(eos, cell_size(oracle, test, axis, dtype))
    got = assert_is_the_solvers_sweep(oracle, test, f, axis, dt, dtype, scheme, limiter, projection)
    for k in STATE:                                   # no stage is hidden: every field moves by at least 0.1 % of its maximum, 1e4 times the fp32 rounding
        a, b = oracle.real_view(getattr(got, k), NX, NY, G), oracle.real_view(f[k], NX, NY, G)
        assert np.abs(a - b).max() > 1e-3 * np.abs(b).max(), k
    assert got.cfl_fresh_eos != got.cfl()             # the two readings of "the CFL step after the sweep" do differ


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("test", ["Sod", "Sod_circ", "Sedov", "Bizarrium"])
def test_reference_sweep_is_the_oracle_solvers_sweep_on_developed_physical_states(oracle, test, axis, dtype):
    """The state of each test case after 12 cycles (Sod: mirrors of -1 along x; Sedov: +1 everywhere; Bizarrium: -1 / +1 on
    the two x sides and its own EOS), then one more sweep with the step the solver would take."""
    run, f = oracle.solve(test=test, N=(NX, NY), nghost=G, maxcycle=12, data_type=dtype)
    assert_is_the_solvers_sweep(oracle, test, {k: f[k].copy() for k in STATE}, axis, dtype(run.last_dt), dtype,
                                "GAD", "minmod", "euler_2nd")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("eos", ["perfect_gas", "bizarrium"])
def test_reference_sweep_of_a_tile_is_the_sweep_of_the_block_it_was_cut_from(oracle, eos, axis, dtype):
    """bc = 0: a tile whose ghosts along the axis hold its neighbours' cells gives the cells the whole block gives — the EOS
    on the ghost layers is then the neighbour's EOS. Three tiles along the axis: (1, 0), (0, 0) and (0, 1) sides."""
    f = rand_state(NX, NY, G, eos, dtype, seed=23)
    dx = dtype(1.) / dtype((NX, NY)[axis])
    dt = rand_dt(eos, dx)
    f_low, f_high = (-1., 1.), (0.5, -2.)
    args = ("GAD", "superbee", "euler_2nd", eos, dt, dx)
    whole = reference_sweep(f, NX, NY, G, axis, *args, 1, 1, f_low, f_high, dtype)
    n = (NX, NY)[axis]
    cuts = [0, 40, 47, n]
    grid = lambda a: a.reshape(NY + 2 * G, NX + 2 * G)
    steps = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sl = (slice(None), slice(lo, hi + 2 * G)) if axis == 0 else (slice(lo, hi + 2 * G), slice(None))
        tile = {k: np.ascontiguousarray(grid(f[k])[sl]).ravel() for k in STATE}
        tnx, tny = (hi - lo, NY) if axis == 0 else (NX, hi - lo)
        got = reference_sweep(tile, tnx, tny, G, axis, *args, int(lo == 0), int(hi == n), f_low, f_high, dtype)
        for k in STATE + ("p", "c"):
            want = oracle.real_view(getattr(whole, k), NX, NY, G)
            want = want[:, lo:hi] if axis == 0 else want[lo:hi, :]
            assert np.array_equal(oracle.real_view(getattr(got, k), tnx, tny, G), want), (k, lo, hi)
        assert got.cfl() == whole.cfl(lo, hi)
        steps.append(got.cfl())
    assert min(steps) == whole.cfl()


@pytest.mark.parametrize("axis,nx,ny,g", [(0, 123, 5, 5), (1, 70, 101, 4)], ids=["X", "Y"])
def test_random_states_tell_the_mirrored_cells_and_the_factors_apart(axis, nx, ny, g):
    """What tests/test_gpu_sweep_random_state.py relies on when it mirrors low (-1, 1) and high (1, -1): on a random state the
    two factors of a side swapped, or the two sides swapped, are another sweep — every cell next to the high wall differs — so
    a kernel that confuses them cannot give the reference's bits by symmetry. Along x and along y (where the factor along the
    axis is v's)."""
    f = rand_state(nx, ny, g, "perfect_gas", np.float64, seed=4002)
    dx = 1. / (nx, ny)[axis]
    args = ("GAD", "minmod", "euler_2nd", "perfect_gas", rand_dt("perfect_gas", dx), dx, 1, 1)
    low, high = (-1., 1.), (1., -1.)
    ref = reference_sweep(f, nx, ny, g, axis, *args, low, high, np.float64)
    swapped_sides = reference_sweep(f, nx, ny, g, axis, *args, high, low, np.float64)
    swapped_parts = reference_sweep(f, nx, ny, g, axis, *args, low, high[::-1], np.float64)
    n = (nx, ny)[axis]
    wall = real_mask(nx, ny, g, axis, n - 1, n)
    for other in (swapped_sides, swapped_parts):
        for k in ("rho", "u", "v", "E"):
            assert (getattr(other, k)[wall] != getattr(ref, k)[wall]).all(), k
