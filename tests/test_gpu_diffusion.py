"""Physical diffusion on the GPU: armon_hip_diffuse against the numpy restatement of its rule
(tests/diffusion_restated.py) bit for bit, the refusals of the C ABI, and whole runs of a lone block against the restated
cycle driver.

One step: every output starts as a NaN marker (compared as integers) and every ghost cell of every input holds a NaN of
another payload, so what the step writes — the real cells of its outputs —, what it must leave alone — ghosts, padding, the
inputs — and that it reads no ghost (a NaN would spread into the real cells) are checked cell by cell. Shapes: the kernel
gives a wave a strip of 62 columns, a workgroup 4 strips (248 columns) and a run of 64 rows, so nx = 61..63, 123..125,
247..249 and ny = 63..65 stand at its own boundaries, beside the sizes the issue names."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from diffusion_restated import FREE, WALL, run_cycles, step, substeps

pytestmark = pytest.mark.gpu

MARKER = {"float64": np.uint64(0x7ff8dead0000beef), "float32": np.uint32(0x7fc0beef)}
GHOST = {"float64": np.uint64(0x7ff80000000dead1), "float32": np.uint32(0x7fc0dea1)}     # what the ghosts of the inputs hold
DTYPES = ("float64", "float32")
STATE = ("rho", "u", "v", "E")
NU, CHI, DS = 1e-2, 2e-2, (1.5e-2, 0.5e-2, 3e-2, 1e-2)


def A():
    import armon_amd
    return armon_amd


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.fixture(scope="module")
def dev():
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.wait()
    d.close()


def fn(dev, dtype):
    return getattr(dev._L, "armon_hip_diffuse" + ("_f32" if dtype == "float32" else ""))


def last_error(dev):
    return dev._L.armon_hip_last_error().decode()


def ghosted(real, g, dtype):
    ny, nx = real.shape
    full = np.empty((ny + 2 * g, nx + 2 * g), dtype=dtype)
    bits(full)[...] = GHOST[dtype]
    full[g:g + ny, g:g + nx] = real
    return full.ravel()


def random_inputs(nx, ny, g, dtype, ns, seed):
    rng = np.random.default_rng(seed)
    rho = 1 + rng.random((ny, nx))
    u, v = rng.normal(size=(ny, nx)), rng.normal(size=(ny, nx))
    E = 3 + rng.random((ny, nx)) + 0.5 * (u * u + v * v)
    real = dict(rho=rho.astype(dtype), u=u.astype(dtype), v=v.astype(dtype), E=E.astype(dtype))
    phis = [rng.uniform(-1., 2., (ny, nx)).astype(dtype) for _ in range(ns)]
    return real, phis


def sides_of(x, y):
    """``x, y`` each one of 'periodic', 'wall', 'free', 'wall-free', 'free-wall' → (periodic, factors)."""
    def pair(kind, k):
        lo, hi = (kind.split("-") * 2)[:2] if kind != "periodic" else ("free", "free")
        return [WALL[k] if lo == "wall" else FREE[k], WALL[k + 1] if hi == "wall" else FREE[k + 1]]
    return (x == "periodic", y == "periodic"), tuple(pair(x, 0) + pair(y, 2))


def descriptor(nx, ny, g, periodic, factors, dt, dx, dy, nu, chi, Ds):
    from armon_amd._lib import DiffuseDesc
    d = DiffuseDesc()
    d.nx, d.ny, d.nghost, d.ns = nx, ny, g, len(Ds)
    for k in range(4):
        d.periodic[k] = int(periodic[k // 2])
        d.u_factor[k], d.v_factor[k] = factors[k]
    d.dt, d.dx, d.dy, d.nu, d.chi = dt, dx, dy, nu, chi
    for k, D in enumerate(Ds):
        d.D[k] = D
    return d


class Step:
    """The arrays of one launch on the device: inputs uploaded, outputs marked."""

    def __init__(self, dev, nx, ny, g, dtype, real, phis, with_state=True, with_rho_out=True):
        self.dev, self.nx, self.ny, self.g, self.dtype = dev, nx, ny, g, dtype
        n = (nx + 2 * g) * (ny + 2 * g)
        self.marker = np.empty(n, dtype=dtype)
        bits(self.marker)[...] = MARKER[dtype]
        self.host = {k: ghosted(real[k], g, dtype) for k in STATE}
        self.host_phi = [ghosted(p, g, dtype) for p in phis]
        self.inp = {k: dev.from_host(self.host[k]) for k in (STATE if with_state else ("rho",))}
        self.out = {k: dev.from_host(self.marker) for k in ((STATE if with_rho_out else STATE[1:]) if with_state else ())}
        self.phi = [dev.from_host(a) for a in self.host_phi]
        self.phi_out = [dev.from_host(self.marker) for _ in phis]

    def fill(self, d):
        for k, a in self.inp.items():
            setattr(d, k, a.ptr)
        for k, a in self.out.items():
            setattr(d, k + "_out", a.ptr)
        for k, (a, b) in enumerate(zip(self.phi, self.phi_out)):
            d.phi[k], d.phi_out[k] = a.ptr, b.ptr
        return d

    def launch(self, d, dtype, expect=0):
        rc = fn(self.dev, dtype)(self.dev.ctx, C.byref(d))
        msg = last_error(self.dev)
        assert rc == expect, (rc, msg)
        self.dev.wait()
        return msg

    def inside(self):
        m = np.zeros((self.ny + 2 * self.g, self.nx + 2 * self.g), dtype=bool)
        m[self.g:self.g + self.ny, self.g:self.g + self.nx] = True
        return m.ravel()

    def assert_inputs_untouched(self):
        for k, a in self.inp.items():
            assert np.array_equal(bits(a.to_host()), bits(self.host[k])), f"the input {k} was modified"
        for k, a in enumerate(self.phi):
            assert np.array_equal(bits(a.to_host()), bits(self.host_phi[k])), f"the input phi[{k}] was modified"

    def assert_nothing_written(self):
        self.assert_inputs_untouched()
        for k, a in list(self.out.items()) + list(enumerate(self.phi_out)):
            assert (bits(a.to_host()) == MARKER[self.dtype]).all(), f"the output {k} was written"

    def assert_output(self, name, got, want_real):
        inside, mark = self.inside(), MARKER[self.dtype]
        want = ghosted(want_real, self.g, self.dtype)
        assert np.isfinite(want_real).all(), f"the restatement of {name} is not finite"
        stray = np.flatnonzero((bits(got) != mark) & ~inside)
        assert stray.size == 0, f"{name}: {stray.size} cells written outside the real cells, first at {stray[0]}"
        bad = np.flatnonzero((bits(got) != bits(want)) & inside)
        assert bad.size == 0, (f"{name}: {bad.size} of {inside.sum()} real cells differ from the restatement, first at flat index "
                               f"{bad[0]} (pitch {self.nx + 2 * self.g}): {got[bad[0]]!r} != {want[bad[0]]!r}")

    def free(self):
        self.dev.wait()
        for a in list(self.inp.values()) + list(self.out.values()) + self.phi + self.phi_out:
            a.free()


def check_one_step(dev, dtype, nx, ny, g=4, x="wall", y="wall", nu=NU, chi=CHI, ns=1, seed=7, with_rho_out=True):
    """One launch on a random state against the restatement; returns the outputs (host arrays) by name."""
    T = np.dtype(dtype).type
    periodic, factors = sides_of(x, y)
    dx, dy = float(T(1) / T(nx)), float(T(1) / T(ny))
    Ds = DS[:ns]
    kappa = max([4 * nu / 3, chi] + list(Ds))
    dt = float(T(0.4 / (2 * kappa * (1 / dx ** 2 + 1 / dy ** 2))))
    real, phis = random_inputs(nx, ny, g, dtype, ns, seed)
    state = nu != 0 or chi != 0
    S = Step(dev, nx, ny, g, dtype, real, phis, with_state=state, with_rho_out=with_rho_out)
    try:
        d = S.fill(descriptor(nx, ny, g, periodic, factors, dt, dx, dy, nu, chi, Ds))
        S.launch(d, dtype)
        u, v, E, new = step(real["rho"], real["u"], real["v"], real["E"], phis, dt, dx, dy, nu, chi, Ds, periodic, factors)
        S.assert_inputs_untouched()
        got = {}
        if state:
            for k, want in (("u", u), ("v", v), ("E", E)) + ((("rho", real["rho"]),) if with_rho_out else ()):
                got[k] = S.out[k].to_host()
                S.assert_output(k, got[k], want)
        for k, want in enumerate(new):
            got[f"phi{k}"] = S.phi_out[k].to_host()
            S.assert_output(f"phi[{k}]", got[f"phi{k}"], want)
        return got
    finally:
        S.free()


# ---- one step against the restatement --------------------------------------------------------------------------------------------

KINDS = ("periodic", "wall", "free", "wall-free")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("x,y", list(itertools.product(KINDS, KINDS)) + [("free-wall", "free-wall")])
def test_every_combination_of_sides(dev, dtype, x, y):
    check_one_step(dev, dtype, 70, 67, x=x, y=y, ns=1)      # two strips, two runs: every corner and side of the block


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nu,chi,ns", [(NU, CHI, 0), (NU, 0., 0), (0., CHI, 0), (0., 0., 1), (0., 0., 4), (NU, CHI, 1), (NU, CHI, 2),
                                       (NU, CHI, 3), (NU, CHI, 4)])
def test_which_planes_diffuse(dev, dtype, nu, chi, ns):
    check_one_step(dev, dtype, 70, 67, x="periodic", y="wall-free", nu=nu, chi=chi, ns=ns)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nu,chi", [(0., 0.), (NU, CHI)], ids=["planes", "state+planes"])
def test_four_planes_in_one_launch_are_four_launches_of_one(dev, dtype, nu, chi):
    nx, ny, g = 70, 67, 4
    T = np.dtype(dtype).type
    periodic, factors = sides_of("wall", "periodic")
    dx, dy = float(T(1) / T(nx)), float(T(1) / T(ny))
    dt = float(T(0.4 / (2 * max(4 * nu / 3, chi, *DS) * (1 / dx ** 2 + 1 / dy ** 2))))
    real, phis = random_inputs(nx, ny, g, dtype, 4, 11)
    S = Step(dev, nx, ny, g, dtype, real, phis, with_state=nu != 0 or chi != 0)
    try:
        S.launch(S.fill(descriptor(nx, ny, g, periodic, factors, dt, dx, dy, nu, chi, DS)), dtype)
        together = [a.to_host() for a in S.phi_out]
        for k in range(4):
            S.phi_out[0].copy_from_host(S.marker)
            d = S.fill(descriptor(nx, ny, g, periodic, factors, dt, dx, dy, nu, chi, DS[k:k + 1]))
            d.phi[0], d.phi_out[0] = S.phi[k].ptr, S.phi_out[0].ptr
            S.launch(d, dtype)
            assert np.array_equal(bits(S.phi_out[0].to_host()), bits(together[k])), f"plane {k}: ns = 1 and ns = 4 differ"
    finally:
        S.free()


SHAPES = ([(1, 1), (1, 7), (7, 1), (2, 2)] + [(nx, 5) for nx in (61, 62, 63, 64, 65, 123, 124, 125, 127, 128, 129, 247, 248, 249)]
          + [(5, ny) for ny in (63, 64, 65, 127, 128, 129)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [4, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_and_ghost_widths(dev, dtype, g, shape):
    k = SHAPES.index(shape)
    x, y = KINDS[k % 4], KINDS[(k // 4 + k) % 4]
    check_one_step(dev, dtype, *shape, g=g, x=x, y=y, ns=1 + k % 2, seed=100 + k)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,x,y", [((300007, 3), "periodic", "wall"), ((300007, 3), "wall-free", "periodic"),
                                       ((3, 70001), "wall", "periodic"), ((3, 70001), "periodic", "free-wall")],
                         ids=lambda s: str(s).replace(" ", ""))
def test_long_axes(dev, dtype, shape, x, y):
    check_one_step(dev, dtype, *shape, x=x, y=y, ns=1)


def test_without_rho_out_the_density_is_not_copied(dev):
    got = check_one_step(dev, "float64", 70, 9, with_rho_out=False)
    assert "rho" not in got and set(got) == {"u", "v", "E", "phi0"}


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------------------

def refusals():
    def field(name, value, message):
        return (f"{name}={value!r}", lambda d, S: setattr(d, name, value), message)

    def item(name, k, value, message):
        return (f"{name}[{k}]={value!r}", lambda d, S: getattr(d, name).__setitem__(k, value), message)

    nan, inf = float("nan"), float("inf")
    cases = [field("ns", -1, "ns"), field("ns", 5, "ns"), field("nx", 0, "empty block"), field("ny", 0, "empty block"),
             field("ny", 65535 * 64 + 1, "oversized block"), field("nghost", -1, "nghost"),
             field("dt", -1e-3, "dt"), field("dt", nan, "dt"), field("dt", inf, "dt"),
             field("nu", -1., "nu"), field("nu", nan, "nu"), field("chi", -1., "chi"), field("chi", inf, "chi"),
             item("D", 0, -1., r"D\[0\]"), item("D", 1, nan, r"D\[1\]"),
             field("dx", 0., "dx"), field("dy", nan, "dy"),
             item("u_factor", 0, 0.5, r"u_factor\[0\]"), item("v_factor", 3, 0., r"v_factor\[3\]"), item("u_factor", 2, nan, r"u_factor\[2\]"),
             item("periodic", 0, 1, "periodic flag on one side of the x axis only"),
             item("periodic", 3, 1, "periodic flag on one side of the y axis only")]
    for name in ("rho", "u", "v", "E", "u_out", "v_out", "E_out"):
        cases.append(field(name, None, f"{name} is NULL"))
    cases += [item("phi", 1, None, r"phi\[1\] is NULL"), item("phi_out", 0, None, r"phi_out\[0\] is NULL")]
    cases += [("u_out=u", lambda d, S: setattr(d, "u_out", S.inp["u"].ptr), "aliasing"),
              ("E_out=v_out", lambda d, S: setattr(d, "E_out", S.out["v"].ptr), "aliasing"),
              ("rho_out=rho", lambda d, S: setattr(d, "rho_out", S.inp["rho"].ptr), "aliasing"),
              ("phi_out[1]=phi[0]", lambda d, S: d.phi_out.__setitem__(1, S.phi[0].ptr), "aliasing"),
              ("phi_out[0]=E_out", lambda d, S: d.phi_out.__setitem__(0, S.out["E"].ptr), "aliasing")]
    return cases


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_c_abi_refuses_before_any_launch_and_writes_nothing(dev, dtype):
    import re
    nx, ny, g = 20, 9, 4
    real, phis = random_inputs(nx, ny, g, dtype, 2, 3)
    S = Step(dev, nx, ny, g, dtype, real, phis)
    try:
        good = lambda: S.fill(descriptor(nx, ny, g, (False, False), WALL, 1e-5, 1 / nx, 1 / ny, NU, CHI, DS[:2]))
        for name, spoil, message in refusals():
            d = good()
            spoil(d, S)
            msg = S.launch(d, dtype, expect=1)             # ARMON_ERR_INVALID_ARG
            assert re.search(message, msg), (name, msg)
        assert fn(dev, dtype)(None, C.byref(good())) == 1 and "ctx is NULL" in last_error(dev)
        assert fn(dev, dtype)(dev.ctx, None) == 1 and "descriptor is NULL" in last_error(dev)
        S.assert_nothing_written()
        S.launch(good(), dtype)                                # and the descriptor they spoiled runs
        assert not (bits(S.out["u"].to_host()) == MARKER[dtype]).all()
    finally:
        S.free()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_zero_coefficients_launch_nothing(dev, dtype):
    nx, ny, g = 20, 9, 4
    real, phis = random_inputs(nx, ny, g, dtype, 2, 3)
    S = Step(dev, nx, ny, g, dtype, real, phis)
    try:
        d = S.fill(descriptor(nx, ny, g, (False, False), WALL, 1e-5, 1 / nx, 1 / ny, 0., 0., (0., 0.)))
        S.launch(d, dtype)
        S.assert_nothing_written()
        d = descriptor(nx, ny, g, (False, False), WALL, 1e-5, 1 / nx, 1 / ny, 0., 0., (0., 0.))       # no pointer at all
        assert fn(dev, dtype)(dev.ctx, C.byref(d)) == 0
    finally:
        S.free()


# ---- whole runs on a lone block ----------------------------------------------------------------------------------------------------

N = (48, 36)


def shear_layer(dtype, seed=5):
    """A shear layer with a perturbed interface, a dye on one side of it and a second field; values exact in ``dtype``."""
    nx, ny = N
    y, x = np.meshgrid((np.arange(ny) + 0.5) / ny, (np.arange(nx) + 0.5) / nx, indexing="ij")
    rng = np.random.default_rng(seed)
    band = np.tanh((0.25 - np.abs(y - 0.5)) * 12)
    rho = 1.5 + 0.5 * band + 0.02 * rng.uniform(-1, 1, x.shape)
    u = 0.5 * band + 0.02 * rng.uniform(-1, 1, x.shape)
    v = 0.05 * np.sin(4 * np.pi * x) + 0.02 * rng.uniform(-1, 1, x.shape)
    E = 2.5 / (0.4 * rho) + 0.5 * (u * u + v * v)
    s = {k: a.astype(dtype).astype(np.float64) for k, a in dict(rho=rho, u=u, v=v, E=E).items()}
    phis = {"dye": (0.5 + 0.5 * band).astype(dtype).astype(np.float64), "tag": rng.uniform(0., 1., x.shape).astype(dtype).astype(np.float64)}
    return s, phis


def problem_of(s, phis, D=DS[0], boundaries="Dirichlet", **kw):
    scalars = [A().Scalar("dye", array=phis["dye"], diffusivity=D), A().Scalar("tag", array=phis["tag"])]
    return A().Problem.from_arrays(s["rho"], s["u"], s["v"], E=s["E"], boundaries=boundaries, scalars=scalars, maxtime=1e9, **kw)


def run(**kw):
    kw.setdefault("silent", 5)
    kw.setdefault("N", N)
    stats = A().armon(A().ArmonParameters(return_data=True, **kw))
    host = stats.data.device_to_host(STATE)
    out = {k: stats.data.real_view(host[k]).copy() for k in STATE}
    for name in stats.scalars:
        out["s:" + name] = stats.data.scalar(name)
    return stats, out


def same_bits(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


SIDES = {"walls": ("Dirichlet",) * 4, "periodic-x": ("Periodic", "Periodic", "Dirichlet", "Dirichlet"),
         "periodic-y": ("Dirichlet", "Dirichlet", "Periodic", "Periodic"), "periodic": ("Periodic",) * 4}


@pytest.mark.parametrize("dtype,splitting,sides,gravity,nu", [
    ("float64", "Sequential", "walls", (0., 0.), NU), ("float32", "Sequential", "periodic-x", (0.3, -0.7), NU),
    ("float64", "Strang", "periodic-y", (0., 0.), NU), ("float32", "Strang", "walls", (0., -0.5), NU),
    ("float64", "X_only", "periodic", (0.4, 0.), NU), ("float32", "X_only", "walls", (0., 0.), NU),
    ("float64", "Sequential", "walls", (0., -0.5), 0.1125), ("float32", "Sequential", "periodic", (0., 0.), 0.1125)])
def test_exact_runs_are_the_restated_cycles(dtype, splitting, sides, gravity, nu):
    from armon_amd.blocking import Axis
    from armon_amd.solver import split_axes
    nx, ny = N
    g, cycles, Dt = 4, 6, 1e-3
    T = np.dtype(dtype).type
    s, phis = shear_layer(dtype)
    periodic = (SIDES[sides][0] == "Periodic", SIDES[sides][2] == "Periodic")
    stats, out = run(test=problem_of(s, phis, boundaries=SIDES[sides]), data_type=dtype, axis_splitting=splitting, exact_arithmetic=True,
                     maxcycle=cycles, cst_dt=True, Dt=Dt, nghost=g, viscosity=nu, heat_diffusivity=CHI, gravity=gravity)
    sizes = (float(T(1.) / T(nx)), float(T(1.) / T(ny)))
    n = substeps(T(Dt), sizes[0], sizes[1], T(nu), T(CHI), [T(DS[0])])
    assert n == (3 if nu > NU else 1)

    def flat(a):
        full = np.zeros((ny + 2 * g, nx + 2 * g), dtype=dtype)
        full[g:g + ny, g:g + nx] = a
        return full.ravel()
    order = lambda cycle: tuple((0 if axis == Axis.X else 1, f) for axis, f in split_axes(splitting, cycle))
    want, state, launches = run_cycles({k: flat(s[k]) for k in STATE}, [flat(phis["dye"]), flat(phis["tag"])], [DS[0], 0.], nx, ny, g,
                                       order, cycles, Dt, sizes, "GAD", "minmod", "euler_2nd", "perfect_gas", dtype, nu, CHI,
                                       gravity=gravity, periodic=periodic)
    assert stats.cycles == cycles and stats.diffusion_steps == launches == cycles * n
    time = T(0)
    for _ in range(cycles):
        time = T(time + T(Dt))
    assert stats.final_time == time
    real = lambda a: a.reshape(ny + 2 * g, -1)[g:g + ny, g:g + nx]
    for k in STATE:
        assert same_bits(out[k], real(state[k])), k
    for name, w in zip(("dye", "tag"), want):
        assert same_bits(out["s:" + name], real(w)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_coefficients_are_a_run_without_the_options(dtype, tmp_path):
    from armon_amd import checkpoint
    s, phis = shear_layer(dtype)
    kw = dict(data_type=dtype, maxcycle=8, cfl=0.4, checkpoint_at_end=True, checkpoint_file="ck")
    plain_problem = A().Problem.from_arrays(s["rho"], s["u"], s["v"], E=s["E"], maxtime=1e9,
                                            scalars=[A().Scalar("dye", array=phis["dye"]), A().Scalar("tag", array=phis["tag"])])
    plain, want = run(test=plain_problem, output_dir=str(tmp_path / "a"), **kw)
    zero, got = run(test=problem_of(s, phis, D=0., viscosity=0., heat_diffusivity=0.), viscosity=0., heat_diffusivity=0.,
                    output_dir=str(tmp_path / "b"), **kw)
    assert zero.diffusion_steps == 0 and (zero.cycles, zero.final_time, zero.last_dt) == (plain.cycles, plain.final_time, plain.last_dt)
    for k in want:
        assert same_bits(got[k], want[k]), k
    assert zero.data.params.test.digest == plain.data.params.test.digest
    a, b = (open(os.path.join(str(tmp_path / d), "ck_000008.ckpt"), "rb").read() for d in "ab")
    assert a == b
    assert "diffusion" not in checkpoint.read_header(os.path.join(str(tmp_path / "b"), "ck_000008.ckpt"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_tuned_diffusive_run_differs_from_the_inviscid_one(dtype):
    s, phis = shear_layer(dtype)
    kw = dict(data_type=dtype, maxcycle=8, cfl=0.4)
    _, free = run(test=problem_of(s, phis, D=0.), **kw)
    stats, out = run(test=problem_of(s, phis), viscosity=NU, heat_diffusivity=CHI, **kw)
    assert stats.diffusion_steps >= 8
    for k in ("u", "v", "E", "s:dye"):
        assert not same_bits(out[k], free[k]), k
    assert np.isfinite(out["E"]).all()
    # the dye alone: the state of the inviscid run, another dye
    only, dyed = run(test=problem_of(s, phis), **kw)
    assert only.diffusion_steps >= 8
    for k in STATE + ("s:tag",):
        assert same_bits(dyed[k], free[k]), k
    assert not same_bits(dyed["s:dye"], free["s:dye"])


@pytest.mark.parametrize("compress", [False, True], ids=["dense", "packed"])
def test_checkpoint_and_restart_continue_bit_for_bit(tmp_path, compress):
    from armon_amd import checkpoint
    s, phis = shear_layer("float64")
    prob = lambda: problem_of(s, phis, boundaries=SIDES["periodic-x"])
    kw = dict(cfl=0.4, axis_splitting="Strang", viscosity=NU, heat_diffusivity=CHI, gravity=(0., -0.5))
    whole, want = run(test=prob(), maxcycle=12, **kw)
    run(test=prob(), maxcycle=6, checkpoint_at_end=True, checkpoint_compress=compress, output_dir=str(tmp_path), checkpoint_file="ck", **kw)
    path = os.path.join(str(tmp_path), "ck_000006.ckpt")
    header = checkpoint.read_header(path)
    assert header["diffusion"] == {"nu": float(NU).hex(), "chi": float(CHI).hex(), "scalars": {"dye": float(DS[0]).hex()}}
    resumed, got = run(test=prob(), maxcycle=12, restart_from=path, **kw)
    assert (resumed.cycles, resumed.final_time, resumed.last_dt) == (whole.cycles, whole.final_time, whole.last_dt)
    for k in want:
        assert same_bits(got[k], want[k]), k
    with pytest.raises(A()._lib.SolverException, match="diffusion"):
        run(test=prob(), maxcycle=12, restart_from=path, **dict(kw, viscosity=2 * NU))
    other, _ = run(test=prob(), maxcycle=1, **dict(kw, viscosity=2 * NU))
    with pytest.raises(A()._lib.SolverException, match="diffusion"):
        other.data.compare_state(path, rtol=0.)


def test_a_diffusive_run_keeps_the_pair_cycle_and_falls_back_from_the_graph():
    s, _ = shear_layer("float64")
    prob = lambda: A().Problem.from_arrays(s["rho"], s["u"], s["v"], E=s["E"], maxtime=1e9)
    kw = dict(maxcycle=10, cfl=0.4, placement_min_bytes=0, placement_tries=1, viscosity=NU, heat_diffusivity=CHI)
    seen = []
    stats, want = run(test=prob(), **kw)
    assert stats.data.pair_cycles > 0 and stats.diffusion_steps >= 10
    graph, got = run(test=prob(), graph_cycles=True, **kw)
    assert (graph.cycles, graph.final_time, graph.diffusion_steps) == (stats.cycles, stats.final_time, stats.diffusion_steps)
    for k in STATE:
        assert same_bits(got[k], want[k]), k
    # kernel callbacks see the step (and send the cycle through the single sweeps: the same bits)
    class Seen:
        def start(self, name):
            seen.append(name)

        def end(self, name):
            pass
    params = A().ArmonParameters(test=prob(), N=N, silent=5, return_data=True, **kw)
    params.kernel_callbacks.append(Seen())
    single = A().armon(params)
    host = single.data.device_to_host(STATE)
    assert single.data.pair_cycles == 0 and "diffuse" in seen
    for k in STATE:
        assert same_bits(single.data.real_view(host[k]).copy(), want[k]), k


def test_a_tile_group_and_ranks_refuse(monkeypatch):
    from armon_amd import multi_tile
    with pytest.raises(A()._lib.SolverException, match="physical diffusion is not supported for a tile group"):
        multi_tile.TileGroup((2, 1), test="Sod", N=(64, 64), silent=5, viscosity=NU)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)          # a process group of one rank, as far as the options look
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    with pytest.raises(A()._lib.SolverException, match="physical diffusion is not supported for ranks of a process group"):
        A().ArmonParameters(test="Sod", N=(64, 64), silent=5, viscosity=NU, use_MPI=True, P=(1, 1))
