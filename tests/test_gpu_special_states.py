"""One sweep of the real kernels on states made of special values (tests/special_states.py): zeros of both signs, a step, an
interface velocity of exactly 0, slope ratios of exactly 1, 1/2 and 2, subnormal velocities. tests/test_special_states_host.py
shows what the oracle does with them (finite; the signed zeros kept), so that nothing here passes on a reference that lost the
property.

Exact arithmetic, through the fused sweep and through the staged kernels in the order the solver runs them with
use_fused_sweep=False: the oracle's bits in rho, u, v, E, p, c and the CFL step, compared as integers — a zero of the other sign
is a difference. Tuned arithmetic: every launch form gives the same bits, stays finite, leaves a fluid at rest at rest, and stays
within the rounding of the operation. Shapes: tests/special_states.SHAPES, the smallest with a second, partial unit of each launch
form; ghost widths 4 and 5; both precisions; the three scheme triples of tests/special_states.TRIPLES; perfect gas; both sides
mirrored with the factor pairs of tests/test_gpu_sweep_random_state.py."""
import functools

import numpy as np
import pytest

import special_states as SS
from sweep_harness import F_HIGH, F_LOW, MARKER, OUT_NAMES, Block, bits, block_cache, check_outputs, run_tuned_forms
from sweep_reference import STATE, real_mask, uv_factors

pytestmark = pytest.mark.gpu

assert (F_LOW, F_HIGH) == (SS.F_LOW, SS.F_HIGH)
CASES = [(dtype, axis, nx, ny, g, state) for dtype in SS.DTYPES for axis in (0, 1) for (nx, ny) in SS.SHAPES[axis] for g in SS.GHOSTS
         for state in SS.STATES]
IDS = [f"{d}-{'XY'[a]}-{nx}x{ny}-g{g}-{SS.STATES[s]}" for d, a, nx, ny, g, s in CASES]


@pytest.fixture(scope="module")
def blocks():
    yield from block_cache()


class StagedBlock:
    """The staged path of one block: the kernels the solver runs for a sweep with use_fused_sweep=False, in its order, with the
    mirror factors of these tests (the solver takes them from its test case)."""

    NON_STATE = ("p", "c", "g", "us", "ps", "work_1", "work_2", "work_3", "work_4")

    def __init__(self, dev, nx, ny, g, dtype, triple):
        import armon_amd
        from armon_amd.solver import BlockGrid
        scheme, limiter, projection = triple
        self.nx, self.ny, self.g, self.dtype = nx, ny, g, np.dtype(dtype)
        self.params = armon_amd.ArmonParameters(test="Sod", N=(nx, ny), nghost=g, data_type=dtype, silent=5, ctx=dev.ctx,
                                                use_fused_sweep=False, exact_arithmetic=True, scheme=scheme,
                                                riemann_limiter=limiter, projection=projection)
        self.dev = self.params.device
        self.grid = BlockGrid(self.params)
        n = (nx + 2 * g) * (ny + 2 * g)
        self.marker = np.full(n, MARKER[self.dtype.name]).view(self.dtype)

    def sweep(self, f, axis, dt):
        """Upload ``f``, fill every other vector with the marker, run one sweep; returns rho, u, v, E, p, c and the CFL step."""
        from armon_amd import solver as S
        from armon_amd.blocking import Axis, first_side, last_side
        params, grid = self.params, self.grid
        for k in STATE:
            grid.data[k].copy_from_host(f[k])
        for k in self.NON_STATE:
            grid.data[k].copy_from_host(self.marker)
        ax = Axis.X if axis == 0 else Axis.Y
        dx = params.cell_size(axis)
        S.update_EOS(params, grid, ax)
        bs, p = params.block_size, grid.ptr
        for side, factors, sign in ((first_side(ax), F_LOW, -1), (last_side(ax), F_HIGH, 1)):
            uf, vf = uv_factors(axis, factors)
            S.check(params.fn("boundary_conditions")(self.dev.ctx, bs.border_domain(side).to_c(), sign * bs.stride_along(ax), bs.ghosts,
                                                     uf, vf, p("rho"), p("u"), p("v"), p("p"), p("c"), p("g"), p("E")))
        S.numerical_fluxes(params, grid, ax, dt, dx)
        S.cell_update(params, grid, ax, dt, dx)
        S.projection_remap(params, grid, ax, dt, dx)
        out = {"dt": np.array([S.local_time_step(params, grid)], dtype=self.dtype)}
        self.dev.wait()
        out.update({k: grid.data[k].to_host() for k in OUT_NAMES})
        return out


@pytest.fixture(scope="module")
def staged_blocks():
    from armon_amd.device import HIPDevice
    dev = HIPDevice(0)
    cache = {}

    def get(nx, ny, g, dtype, triple):
        key = (nx, ny, g, np.dtype(dtype).name, triple)
        if key not in cache:
            cache[key] = StagedBlock(dev, nx, ny, g, dtype, triple)
        return cache[key]

    yield get
    dev.wait()
    cache.clear()
    dev.close()


def assert_oracle_bits(out, ref, inside, pitch, what):
    for k in OUT_NAMES:
        got, want = bits(out[k]), bits(getattr(ref, k))
        bad = np.flatnonzero((got != want) & inside)
        assert bad.size == 0, (f"{what}{k}: {bad.size} real cells differ from the oracle's bits, first at flat index {bad[0]} (row pitch "
                               f"{pitch}): {out[k][bad[0]]!r} != {getattr(ref, k)[bad[0]]!r}")
    want = np.array([ref.cfl()], dtype=out["dt"].dtype)
    assert bits(out["dt"][:1])[0] == bits(want)[0] and np.isfinite(want[0]), f"{what}dt_cfl_out {out['dt'][0]!r} != {want[0]!r}"


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_exact_fused_sweep_of_a_special_state_is_the_oracles(blocks, dtype, axis, nx, ny, g, state):
    """armon_hip_sweep[_f32], exact: every output array starts as the marker; the written set is the real cells, and it holds the
    oracle's bits as integers — the -0 of a transverse velocity at rest included — in rho, u, v, E, p_out, c_out, dt_cfl_out."""
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    for triple in SS.TRIPLES:
        f, ref, dt = SS.special_reference(state, nx, ny, g, axis, triple, dtype)
        what = f"{SS.STATES[state]} {'-'.join(triple)}: "
        blk.upload(f)
        blk.mark_outputs()
        blk.sweep(axis, triple[0], triple[1], triple[2], "perfect_gas", True, dt, emit=(1, 1))
        out = blk.fetch()
        check_outputs(blk, out, ref, axis, emit=(1, 1), what=what)
        assert_oracle_bits(out, ref, inside, nx + 2 * g, what)


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_exact_staged_sweep_of_a_special_state_is_the_oracles(staged_blocks, dtype, axis, nx, ny, g, state):
    """The staged kernels (EOS, mirrors, fluxes, cell update, advection, projection, dtCFL) in the solver's order: the oracle's
    bits as integers on the real cells; every vector but the state starts as the marker, so nothing unwritten is read."""
    inside = real_mask(nx, ny, g, axis)
    for triple in SS.TRIPLES:
        f, ref, dt = SS.special_reference(state, nx, ny, g, axis, triple, dtype)
        out = staged_blocks(nx, ny, g, dtype, triple).sweep(f, axis, dt)
        assert_oracle_bits(out, ref, inside, nx + 2 * g, f"staged, {SS.STATES[state]} {'-'.join(triple)}: ")


# ---- tuned arithmetic --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def kappa_of(state, nx, ny, g, axis, triple):
    """Per field max|oracle32 - oracle64| / (eps32 max|oracle64|) over the real cells, both oracles on the fp32 form of the
    state (tests/test_gpu_sweep_random_state.kappa_of): from the two oracles alone. 0 where the field is 0 everywhere."""
    _f, o64, _dt = SS.special_reference(state, nx, ny, g, axis, triple, "float32", "float64")
    _f, o32, _dt = SS.special_reference(state, nx, ny, g, axis, triple, "float32", "float32")
    inside = real_mask(nx, ny, g, axis)
    eps32 = float(np.finfo(np.float32).eps)
    kappa = {}
    for k in OUT_NAMES:
        a64 = getattr(o64, k)[inside]
        top = np.abs(a64).max()
        kappa[k] = float(np.abs(getattr(o32, k)[inside].astype(np.float64) - a64).max() / (eps32 * top)) if top > 0 else 0.
    return kappa


@pytest.mark.parametrize("dtype,axis,nx,ny,g,state", CASES, ids=IDS)
def test_tuned_sweep_of_a_special_state(blocks, dtype, axis, nx, ny, g, state):
    """Tuned arithmetic, every launch form (ARMON_X_ROWS 0/1/2; ARMON_Y_SX 0/1/2 x ARMON_Y_COLS1 0/1): the same bits in all of
    them, each writing exactly the real cells; every output finite; wherever the fp64 oracle's velocity is +-0 the tuned one
    compares equal to 0 (a fluid at rest stays at rest).

    States 1 and 2: rho and E within 4 eps of their value — each of the two stages (cell update, projection) is a 1-ulp
    reciprocal and two products. States 3-5: at most 4 max(kappa, 1) eps max|field| from the fp64 oracle, kappa from the two
    oracles alone (the floor of 1: a degenerate state can make the two oracles agree exactly). State 6: the same for rho, E, p
    and c; the velocities, whose field maximum is subnormal, only have to be finite. Prints what it measures (pytest -s)."""
    blk = blocks(nx, ny, g, dtype)
    inside = real_mask(nx, ny, g, axis)
    eps = float(np.finfo(np.dtype(dtype)).eps)
    for triple in SS.TRIPLES:
        f, ref64, dt = SS.special_reference(state, nx, ny, g, axis, triple, dtype, "float64")
        what = f"tuned {dtype} {'XY'[axis]} {nx}x{ny} g{g} {SS.STATES[state]} {'-'.join(triple)}"
        blk.upload(f)
        out = run_tuned_forms(blk, (axis, triple[0], triple[1], triple[2], "perfect_gas"), dt, (1, 1), what + ": ")
        for k in OUT_NAMES:
            assert np.isfinite(out[k][inside]).all(), f"{what}: {k} is not finite in {(~np.isfinite(out[k][inside])).sum()} real cells"
        assert np.isfinite(out["dt"][0]) and out["dt"][0] > 0, f"{what}: dt_cfl_out {out['dt'][0]!r}"
        for k in ("u", "v"):
            rest = inside & (getattr(ref64, k) == 0)
            moved = np.flatnonzero(rest & (out[k] != 0))
            assert moved.size == 0, (f"{what}: {k} is {out[k][moved[0]]!r} in {moved.size} cells where the oracle's is a zero, "
                                     f"first at flat index {moved[0]}")
        if state in (1, 2):
            for k in ("rho", "E"):
                want = f[k][inside].astype(np.float64)
                worst = float((np.abs(out[k][inside].astype(np.float64) - want) / (eps * want)).max())
                print(f"\n{what}: {k} {worst:.2f} eps from its value (bound 4)")
                assert worst <= 4, f"{what}: {k} is {worst:.2f} eps from its value, bound 4"
            continue
        kappa = kappa_of(state, nx, ny, g, axis, triple)
        fields = ("rho", "E", "p", "c") if state == 6 else OUT_NAMES
        measured = {}
        for k in fields:
            want = getattr(ref64, k)[inside].astype(np.float64)
            top = np.abs(want).max()
            dev = float(np.abs(out[k][inside].astype(np.float64) - want).max())
            bound = 4 * max(kappa[k], 1.) * eps * top
            measured[k] = (dev / (eps * top) if top > 0 else dev, 4 * max(kappa[k], 1.))
            assert dev <= bound, f"{what}: {k} is {measured[k][0]:.2f} eps of the field maximum from the fp64 oracle, bound {measured[k][1]:.2f}"
        print(f"\n{what}: " + ", ".join(f"{k} {r:.2f} eps (bound {b:.1f})" for k, (r, b) in measured.items()))

