"""Physical diffusion without a GPU: the properties of the rule of include/armon_hip.h on its numpy
restatement (tests/diffusion_restated.py), and the host logic around it — sub-step counts, options and their refusals,
headers and digests, the drivers a diffusive run takes, and the exported symbols.

Bounds. Conservation: every step adds to each cell k·(face differences), whose sum over the cells telescopes exactly in real
arithmetic; what is left is the rounding of the update, a few eps per cell and step with either sign, and the issue's bound
for 400 steps is 8 eps·Σρ (measured with these seeds: printed, pytest -s). Decay of a single mode: the discrete factor is
exact for the scheme, so after 50 steps the result is the factor's power up to 50 roundings of eps·max|a| (measured 1.1e-15
for an amplitude of 1 in fp64)."""
import ctypes
import math

import numpy as np
import pytest

import armon_amd
from armon_amd import checkpoint
from armon_amd._lib import SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import diffusion_substeps, graph_cycles_usable, pair_usable

from diffusion_restated import FREE, WALL, step

EPS = float(np.finfo(np.float64).eps)


def random_state(nx=24, ny=20, seed=1):
    rng = np.random.default_rng(seed)
    rho = 1 + rng.random((ny, nx))
    u, v = rng.normal(size=(ny, nx)), rng.normal(size=(ny, nx))
    E = 3 + rng.random((ny, nx)) + 0.5 * (u * u + v * v)
    return rho, u, v, E, rng.random((ny, nx))


def content(rho, a):
    return math.fsum((rho.astype(np.float64) * a.astype(np.float64)).ravel())


# ---- the rule ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("periodic", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("factors", [WALL, FREE], ids=["walls", "freeflow"])
def test_a_uniform_state_is_a_fixed_point_bit_for_bit(dtype, periodic, factors):
    T = np.dtype(dtype).type
    one = np.ones((20, 24), dtype=dtype)
    rho, u, v, E, phi = (T(c) * one for c in (1.3, 0.7, -0.2, 2.5, 0.4))
    if factors is WALL:
        # a reflecting wall reverses the normal velocity: the uniform state that is a fixed point next to it has none
        u = u if periodic[0] else T(0) * one
        v = v if periodic[1] else T(0) * one
    nu, chi, D = 1e-2, 2e-2, 1.5e-2
    out = step(rho, u, v, E, [phi], 1e-3, 1 / 24, 1 / 20, nu, chi, [D], periodic, factors)
    for new, old in zip((out[0], out[1], out[2], out[3][0]), (u, v, E, phi)):
        assert new.dtype == old.dtype and new.tobytes() == old.tobytes()


def run_400(periodic, factors):
    rho, u, v, E, phi = random_state()
    nx, ny = rho.shape[1], rho.shape[0]
    dx, dy = 1 / nx, 1 / ny
    nu, chi, D = 1e-2, 2e-2, 1.5e-2
    dt = 0.5 / (2 * max(4 * nu / 3, chi, D) * (1 / dx ** 2 + 1 / dy ** 2))
    before = [content(rho, a) for a in (u, v, E, phi)]
    for _ in range(400):
        u, v, E, (phi,) = step(rho, u, v, E, [phi], dt, dx, dy, nu, chi, [D], periodic, factors)
    assert np.isfinite(u).all() and np.isfinite(E).all() and np.abs(u).max() < 10      # bounded at sigma = 0.5
    scale = EPS * float(rho.sum())
    return [abs(content(rho, a) - b) / scale for a, b in zip((u, v, E, phi), before)]


def test_periodic_random_state_conserves_momentum_energy_and_content():
    drift = run_400((True, True), WALL)
    print(f"\nperiodic: drift of sum(rho u, rho v, rho E, rho phi) after 400 steps = {drift} eps sum(rho) (bound 8)")
    assert max(drift) <= 8


def test_walls_conserve_energy_and_content_but_not_the_normal_momentum():
    drift = run_400((False, False), WALL)
    print(f"\nwalls: drift of sum(rho u, rho v, rho E, rho phi) after 400 steps = {drift} eps sum(rho) (bound 8 for E and phi)")
    assert drift[2] <= 8 and drift[3] <= 8
    assert drift[0] > 1e6 and drift[1] > 1e6            # the walls take the normal momentum up


def decay(N, steps, what, ny=4, coefficient=1e-2):
    """A single mode of wave number 2 pi along x on uniform rho = 1, periodic: → (result, initial mode, factor, dt)."""
    dx, dy = 1 / N, 1 / ny
    x = (np.arange(N) + 0.5) / N
    mode = np.tile(np.sin(2 * np.pi * x), (ny, 1))
    one, zero = np.ones((ny, N)), np.zeros((ny, N))
    dt = 0.25 * dx * dx / coefficient
    g = 1 - 4 * coefficient * dt / dx ** 2 * np.sin(np.pi * dx) ** 2
    nu = chi = D = 0.
    u, v, E, phi = zero, zero, 1.5 * one, zero
    if what == "v":
        nu, v, E = coefficient, mode, 1.5 * one + 0.5 * mode * mode
    elif what == "e":
        chi, E = coefficient, 1.5 * one + 0.5 * mode
    else:
        D, phi = coefficient, mode
    E0 = math.fsum(E.ravel())
    for _ in range(steps):
        u, v, E, (phi,) = step(one, u, v, E, [phi], dt, dx, dy, nu, chi, [D], (True, True))
    return dict(u=u, v=v, E=E, phi=phi, mode=mode, g=g, dt=dt, E0=E0)


def test_shear_wave_decays_by_the_exact_discrete_factor():
    r = decay(24, 50, "v")
    err = float(np.abs(r["v"] - r["g"] ** 50 * r["mode"]).max())
    drift = abs(math.fsum(r["E"].ravel()) - r["E0"]) / r["E0"]
    print(f"\nshear wave: |v - g^50 v0| = {err:.3g} (bound {50 * EPS:.3g}); relative drift of sum(E) = {drift:.3g}")
    assert err <= 50 * EPS
    assert drift <= 50 * EPS                               # the kinetic energy the wave loses is the heat the gas gains
    assert not r["u"].any()


def test_thermal_and_dye_modes_decay_likewise():
    r = decay(24, 50, "e")
    err = float(np.abs((r["E"] - 1.5) - r["g"] ** 50 * 0.5 * r["mode"]).max())
    print(f"\nthermal mode: {err:.3g} (bound {50 * EPS:.3g})")
    assert err <= 50 * EPS
    assert not r["u"].any() and not r["v"].any()
    r = decay(24, 50, "phi")
    err = float(np.abs(r["phi"] - r["g"] ** 50 * r["mode"]).max())
    print(f"dye mode: {err:.3g} (bound {50 * EPS:.3g})")
    assert err <= 50 * EPS
    assert r["E"].tobytes() == (1.5 * np.ones_like(r["E"])).tobytes()       # nu = chi = 0: the state is not touched


def test_the_gap_to_the_continuum_decay_falls_as_the_discrete_factor_predicts():
    nu, gaps, predicted = 1e-2, [], []
    for N, steps in ((16, 16), (32, 64), (64, 256)):     # the same time: steps·dt = 16·0.25/(256 nu)
        r = decay(N, steps, "v", coefficient=nu)
        exact = math.exp(-nu * (2 * math.pi) ** 2 * steps * r["dt"])
        amplitude = float(np.abs(r["v"]).max() / np.abs(r["mode"]).max())
        gaps.append(abs(amplitude - exact))
        predicted.append(abs(r["g"] ** steps - exact))
    print(f"\ngap to exp(-nu k^2 t) at N = 16, 32, 64: {gaps}; predicted {predicted}")
    for k in range(2):
        assert gaps[k] / gaps[k + 1] == pytest.approx(predicted[k] / predicted[k + 1], rel=1e-6)
        assert 3.5 < gaps[k] / gaps[k + 1] < 4.5           # second order in dx (and first in dt = dx²/4 nu)


# ---- host logic ------------------------------------------------------------------------------------------------------------------

def unit_cells(**kw):
    """dx = dy = 1: 2·(1/dx² + 1/dy²) = 4, so the diffusion number of a cycle is 4·kappa·dt."""
    return ArmonParameters(test="Sod", N=(16, 16), domain_size=(16., 16.), silent=5, **kw)


def test_diffusion_substeps_at_its_integer_boundaries():
    p = unit_cells(heat_diffusivity=0.25)                  # kappa = 1/4: number = dt, sigma = 0.5
    assert p.diffusive
    above = lambda x: float(np.nextafter(x, 2 * x))
    assert [diffusion_substeps(p, dt) for dt in (1e-9, 0.5, above(0.5), 1.0, above(1.0), 1.5, above(1.5))] == [1, 1, 2, 2, 3, 3, 4]
    p = unit_cells(viscosity=0.75, heat_diffusivity=0.5)   # kappa = 4 nu / 3 = 1
    assert [diffusion_substeps(p, dt) for dt in (0.125, above(0.125), 0.25)] == [1, 2, 2]
    p = unit_cells(scalars=[armon_amd.Scalar("dye", diffusivity=2.0), armon_amd.Scalar("ink")], diffusion_number=1.0)
    assert p.scalar_diffusivities == (2.0, 0.0)
    assert [diffusion_substeps(p, dt) for dt in (0.125, above(0.125))] == [1, 2]
    assert diffusion_substeps(unit_cells(), 1.0) == 0 and not unit_cells().diffusive
    p = unit_cells(heat_diffusivity=0.25, diffusion_max_substeps=3)
    assert diffusion_substeps(p, 1.5) == 3
    with pytest.raises(SolverException, match=r"dt = 2\.0.*diffusion number 2\.0.*needs 4 sub-steps.*diffusion_max_substeps = 3") as e:
        diffusion_substeps(p, 2.0)
    assert e.value.category == "time"


def test_the_parameter_overrides_the_problem_as_gravity_does():
    state = armon_amd.State(1., p=1.)
    prob = armon_amd.Problem("p", state, viscosity=0.01, heat_diffusivity=0.02)
    p = ArmonParameters(test=prob, N=(8, 8), silent=5)
    assert (p.viscosity, p.heat_diffusivity, p.diffusive) == (0.01, 0.02, True)
    p = ArmonParameters(test=prob, N=(8, 8), silent=5, viscosity=0., heat_diffusivity=0.)
    assert (p.viscosity, p.heat_diffusivity, p.diffusive) == (0., 0., False)
    p = ArmonParameters(test=prob, N=(8, 8), silent=5, viscosity=0.5, data_type=np.float32)
    assert p.viscosity == 0.5 and p.heat_diffusivity == float(np.float32(0.02))       # rounded to the data type
    rho = np.ones((8, 8))
    arr = armon_amd.Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, viscosity=0.25, scalars=[armon_amd.Scalar("a", array=rho, diffusivity=0.125)])
    p = ArmonParameters(test=arr, N=(8, 8), silent=5)
    assert (p.viscosity, p.scalar_diffusivities, p.diffusive) == (0.25, (0.125,), True)


@pytest.mark.parametrize("kw,message", [
    (dict(viscosity=-1.), "viscosity takes a finite number >= 0"),
    (dict(viscosity=float("nan")), "viscosity takes a finite number >= 0"),
    (dict(heat_diffusivity=float("inf")), "heat_diffusivity takes a finite number >= 0"),
    (dict(heat_diffusivity="1"), "heat_diffusivity takes a finite number >= 0"),
    (dict(viscosity=1e300, data_type=np.float32), "viscosity = 1e\\+300 is not finite in float32"),
    (dict(viscosity=0.1, use_fused_sweep=False), "runs behind the fused sweeps only"),
    (dict(viscosity=0.1, compare=True), "runs behind the fused sweeps only"),
    (dict(viscosity=0.1, diffusion_number=0.), "diffusion_number must be a number in \\(0, 1\\]"),
    (dict(viscosity=0.1, diffusion_number=1.5), "diffusion_number must be a number in \\(0, 1\\]"),
    (dict(diffusion_max_substeps=0), "diffusion_max_substeps must be an integer >= 1"),
    (dict(diffusion_max_substeps=2.5), "diffusion_max_substeps must be an integer >= 1"),
])
def test_option_refusals(kw, message):
    with pytest.raises(SolverException, match=message) as e:
        ArmonParameters(test="Sod", N=(16, 16), silent=5, **kw)
    assert e.value.category == "config"


def test_scalar_and_problem_refusals_and_use_mpi(monkeypatch):
    for bad in (-0.1, float("nan"), float("inf"), "x", True):
        with pytest.raises(SolverException, match="the diffusivity of the scalar 'dye' takes a finite number >= 0"):
            armon_amd.Scalar("dye", diffusivity=bad)
    with pytest.raises(SolverException, match="viscosity takes a finite number >= 0"):
        armon_amd.Problem("p", armon_amd.State(1., p=1.), viscosity=-1e-3)
    with pytest.raises(SolverException, match="heat_diffusivity takes a finite number >= 0"):
        armon_amd.Problem("p", armon_amd.State(1., p=1.), heat_diffusivity=float("nan"))
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)          # a process group of one rank, as far as the options look
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    ArmonParameters(test="Sod", N=(16, 16), silent=5, use_MPI=True, P=(1, 1))          # (a rank without diffusion is accepted)
    for kw in (dict(viscosity=0.1), dict(heat_diffusivity=0.1)):
        with pytest.raises(SolverException, match="physical diffusion is not supported for ranks of a process group") as e:
            ArmonParameters(test="Sod", N=(16, 16), silent=5, use_MPI=True, P=(1, 1), **kw)
        assert e.value.category == "config"


@pytest.mark.parametrize("kw", [dict(viscosity=0.1), dict(heat_diffusivity=0.1),      # (a scalar of any kind is refused there already)
                                dict(test=armon_amd.Problem("p", armon_amd.State(1., p=1.), viscosity=0.1))])
def test_a_tile_group_refuses_in_its_constructor_before_anything_is_created(kw, monkeypatch):
    from armon_amd import _lib, multi_tile
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was loaded before the refusal"))
    kw = dict(dict(test="Sod", N=(32, 32), silent=5), **kw)
    with pytest.raises(SolverException, match="physical diffusion is not supported for a tile group") as e:
        multi_tile.TileGroup((2, 1), **kw)
    assert e.value.category == "config"


def test_headers_and_digests_change_only_with_a_non_zero_coefficient():
    rho = np.ones((8, 8))
    prob = lambda **kw: armon_amd.Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, **kw)
    dye = lambda D: [armon_amd.Scalar("dye", array=rho, diffusivity=D)]
    base = ArmonParameters(test=prob(scalars=dye(0.)), N=(8, 8), silent=5)
    plain = ArmonParameters(test=armon_amd.Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, scalars=[armon_amd.Scalar("dye", array=rho)]),
                            N=(8, 8), silent=5)
    zero = ArmonParameters(test=prob(scalars=dye(0.), viscosity=0., heat_diffusivity=0.), N=(8, 8), silent=5, viscosity=0., heat_diffusivity=0.)
    assert checkpoint.bit_options(base) == checkpoint.bit_options(plain) == checkpoint.bit_options(zero)
    assert "diffusion" not in checkpoint.bit_options(zero) and "diffusion" not in zero.test.description
    assert base.test.digest == plain.test.digest == zero.test.digest
    seen = {base.test.digest}
    for kw, want in ((dict(viscosity=0.25), {"nu": (0.25).hex(), "chi": (0.).hex(), "scalars": {}}),
                     (dict(heat_diffusivity=0.5), {"nu": (0.).hex(), "chi": (0.5).hex(), "scalars": {}}),
                     (dict(scalars=dye(0.125)), {"nu": (0.).hex(), "chi": (0.).hex(), "scalars": {"dye": (0.125).hex()}})):
        p = ArmonParameters(test=prob(**dict(dict(scalars=dye(0.)), **kw)), N=(8, 8), silent=5)
        options = checkpoint.bit_options(p)
        assert options["diffusion"] == want and p.test.description["diffusion"] == want
        assert p.test.digest not in seen
        seen.add(p.test.digest)
        assert {k: v for k, v in options.items() if k not in ("diffusion", "problem_digest")} == \
               {k: v for k, v in checkpoint.bit_options(base).items() if k != "problem_digest"}
        with pytest.raises(SolverException, match="was written with diffusion = None, this run has diffusion = "):
            checkpoint.check_same_diffusion(p, checkpoint.bit_options(base), "the file")
        checkpoint.check_same_diffusion(p, options, "the file")
    # a built-in case: the parameter alone
    sod = ArmonParameters(test="Sod", N=(16, 16), silent=5, viscosity=0.01)
    assert checkpoint.bit_options(sod)["diffusion"] == {"nu": (0.01).hex(), "chi": (0.).hex(), "scalars": {}}
    assert "diffusion" not in checkpoint.bit_options(ArmonParameters(test="Sod", N=(16, 16), silent=5, viscosity=0.))


def test_a_diffusive_run_keeps_the_pair_cycle_and_leaves_the_graph():
    kw = dict(test="Sod", N=(64, 64), silent=5, placement_min_bytes=0, graph_cycles=True)
    p = ArmonParameters(viscosity=0.01, **kw)
    assert p.diffusive and pair_usable(p) and not graph_cycles_usable(p)
    assert pair_usable(ArmonParameters(**kw))


def test_the_symbols_are_exported_and_bound():
    from armon_amd._lib import ALT_LIB_PATH, SIGNATURES, DiffuseDesc
    for path in (armon_amd.LIB_PATH, ALT_LIB_PATH):
        L = ctypes.CDLL(path)
        assert hasattr(L, "armon_hip_diffuse") and hasattr(L, "armon_hip_diffuse_f32")
    assert "armon_hip_diffuse" in SIGNATURES and "armon_hip_diffuse_f32" in SIGNATURES
    assert ctypes.sizeof(DiffuseDesc) == 16 + 8 + 16 + 64 + 5 * 8 + 32 + 8 * 8 + 64
