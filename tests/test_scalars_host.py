"""Passive scalars, host side (CPU only): the restatement of the scalar sweep against the oracle's own transverse velocity, the
validation of ``Scalar`` / ``Problem`` / ``ArmonParameters(scalars=...)``, and the header and digest rules."""
import hashlib
import json
import re
import os

import numpy as np
import pytest

from scalars_restated import mirror_plus, restated_sweep, run_cycles, wrap_periodic
from sweep_reference import STATE, rand_dt, rand_state, real_mask, reference_sweep

NX, NY, G = 37, 23, 4
F_LOW, F_HIGH = (-1., 1.), (1., 1.)           # (along, across): the transverse factor of every boundary type here is +1


# ---- the restatement ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("axis", [0, 1], ids=["X", "Y"])
@pytest.mark.parametrize("scheme,limiter,projection,eos", [("GAD", "minmod", "euler_2nd", "perfect_gas"), ("GAD", "minmod", "euler", "bizarrium"),
                                                           ("GAD", "superbee", "euler_2nd", "bizarrium"), ("Godunov", "minmod", "euler", "perfect_gas"),
                                                           ("GAD", "no_limiter", "euler_2nd", "perfect_gas")])
@pytest.mark.parametrize("bc", [(1, 1), (0, 1), (0, 0)])
def test_a_plane_that_holds_the_transverse_velocity_gets_the_oracles(oracle, scheme, limiter, projection, eos, axis, dtype, bc):
    f = rand_state(NX, NY, G, eos, dtype, 7)
    T = np.dtype(dtype).type
    dx = float(T(1.) / T((NX, NY)[axis]))
    dt = float(np.float32(rand_dt(eos, dx)))
    args = (NX, NY, G, axis, scheme, limiter, projection, eos, dt, dx, bc[0], bc[1], F_LOW, F_HIGH, dtype)
    ref = reference_sweep(f, *args)
    t_name = "v" if axis == 0 else "u"
    (got, same), new = restated_sweep(f, [f[t_name], f[t_name].copy()], *args)
    inside = real_mask(NX, NY, G, axis)
    view = lambda a: a.view(np.uint64 if a.dtype == np.float64 else np.uint32)[inside]
    assert np.isfinite(got[inside]).all()
    assert np.array_equal(view(got), view(getattr(ref, t_name)))
    assert np.array_equal(view(same), view(got))
    for k in STATE:                                        # and the state it carries the planes with is the oracle's
        assert np.array_equal(view(new[k]), view(getattr(ref, k))), k


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_uniform_plane_stays_uniform_to_rounding_and_the_content_is_conserved(oracle, dtype):
    """What the issue measured on the oracle: a uniform 0.7 moves by 2 ulp in one sweep, the content Σρφ of a walled block
    by less than 1 eps. The bounds the GPU tests use, 4 eps per sweep, hold for the restatement itself."""
    f = rand_state(NX, NY, G, "perfect_gas", dtype, 11)
    T = np.dtype(dtype).type
    eps = float(np.finfo(T).eps)
    rng = np.random.default_rng(3)
    planes = [np.full(f["rho"].size, T(0.7)), rng.uniform(0.5, 1.5, f["rho"].size).astype(T)]
    inside = real_mask(NX, NY, G, 0)
    for axis in (0, 1):
        dx = float(T(1.) / T((NX, NY)[axis]))
        dt = float(np.float32(rand_dt("perfect_gas", dx)))
        (uniform, random_), new = restated_sweep(f, planes, NX, NY, G, axis, "GAD", "minmod", "euler_2nd", "perfect_gas", dt, dx, 1, 1,
                                                 (-1., 1.), (-1., 1.), dtype)        # walls: nothing crosses the sides
        dev = float(np.abs(uniform[inside].astype(np.float64) - 0.7).max() / (eps * 0.7))
        before = float((f["rho"][inside].astype(np.float64) * planes[1][inside].astype(np.float64)).sum())
        after = float((new["rho"][inside].astype(np.float64) * random_[inside].astype(np.float64)).sum())
        print(f"\n{dtype} axis {axis}: uniform plane off by {dev:.2f} eps, content drift {abs(after - before) / (eps * before):.2f} eps")
        assert dev <= 4 and abs(after - before) <= 4 * eps * before


def test_the_cycle_driver_wraps_and_mirrors(oracle):
    a = np.arange((NX + 2 * G) * (NY + 2 * G), dtype=np.float64)
    m = mirror_plus(a, NX, NY, G, 0, 1, 0).reshape(NY + 2 * G, -1)
    assert np.array_equal(m[:, G - 1], m[:, G]) and np.array_equal(m[:, 0], m[:, 2 * G - 1])
    assert np.array_equal(m[:, G + NX:], a.reshape(NY + 2 * G, -1)[:, G + NX:])            # the other side is left alone
    w = wrap_periodic(a, NX, NY, G, 1).reshape(NY + 2 * G, -1)
    assert np.array_equal(w[:G], w[NY:NY + G]) and np.array_equal(w[G + NY:], w[G:2 * G])
    # an X_only run carries v unchanged by anything but the remap: a plane that starts as v ends as v
    f = rand_state(NX, NY, G, "perfect_gas", "float64", 5)
    order = lambda cycle: ((0, 1.0),)
    for periodic in ((False, False), (True, False)):
        (phi,), new = run_cycles(f, [f["v"]], NX, NY, G, order, 3, 1e-3, (1. / NX, 1. / NY), "GAD", "minmod", "euler_2nd", "perfect_gas",
                                 "float64", {0: (F_LOW, F_LOW), 1: ((-1., 1.), (-1., 1.))}, periodic=periodic)
        inside = real_mask(NX, NY, G, 0)
        assert np.array_equal(phi[inside], new["v"][inside]) and not np.array_equal(phi[inside], f["v"][inside])


# ---- Scalar, Problem, ArmonParameters ----------------------------------------------------------------------------------------

def config_error(match):
    from armon_amd._lib import SolverException
    return pytest.raises(SolverException, match=match)


def test_scalar_validation():
    from armon_amd import Box, Disc, Scalar
    s = Scalar("dye", 0.25, [(Disc((0.5, 0.5), 0.2), 1.), (Box(x=(0, 0.1)), -3.)])
    assert s.name == "dye" and s.background == 0.25 and len(s.regions) == 2 and s.array is None
    assert Scalar("a", array=np.zeros((4, 6))).array.shape == (4, 6)
    for bad in ("", 3, None):
        with config_error("non-empty string"):
            Scalar(bad)
    with config_error("must not contain ':'"):
        Scalar("s:dye")
    for bad in (float("nan"), float("inf"), "x"):
        with config_error("background"):
            Scalar("a", bad)
    with config_error("a value of the scalar"):
        Scalar("a", 0., [(Disc((0, 0), 1.), float("inf"))])
    with config_error("pair \\(shape, value\\)"):
        Scalar("a", 0., [(1., Disc((0, 0), 1.))])
    with config_error("NaN or an infinity"):
        Scalar("a", array=np.array([[1., np.nan]]))
    with config_error("2-D array"):
        Scalar("a", array=np.zeros(5))
    with config_error("not both"):
        Scalar("a", regions=[(Disc((0, 0), 1.), 1.)], array=np.zeros((2, 2)))


def test_where_scalars_are_given_and_every_config_error():
    from armon_amd import ArmonParameters, Disc, Problem, Scalar, State
    dye = Scalar("dye", 0., [(Disc((0.5, 0.5), 0.2), 1.)])
    tag = Scalar("tag", array=np.ones((16, 12)))
    prob = Problem("two", State(1., p=1.), [(Disc((0.5, 0.5), 0.2), State(2., p=2.))], scalars=[dye])
    p = ArmonParameters(test=prob, N=(12, 16), scalars=[tag])
    assert p.scalar_names == ("dye", "tag") and p.test.scalars[1].array.dtype == np.float64
    assert ArmonParameters(test="Sod", N=(12, 16), scalars=[dye], data_type="float32").scalar_names == ("dye",)
    assert ArmonParameters(test="Sod", N=(12, 16)).scalar_names == ()
    rho = np.ones((16, 12))
    arr = Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, scalars={"heavy": (rho > 0).astype(float)})
    p = ArmonParameters(test=arr, N=(12, 16), data_type="float32")
    assert p.scalar_names == ("heavy",) and p.test.scalars[0].array.dtype == np.float32
    five = [Scalar(f"s{k}") for k in range(5)]
    with config_error("at most 4"):
        ArmonParameters(test="Sod", N=(12, 16), scalars=five)
    with config_error("at most 4"):
        ArmonParameters(test=Problem("p", State(1., p=1.), scalars=five[:3]), N=(12, 16), scalars=five[3:])
    with config_error("given twice"):
        ArmonParameters(test=prob, N=(12, 16), scalars=[Scalar("dye")])
    with config_error("list of Scalar"):
        ArmonParameters(test="Sod", N=(12, 16), scalars=["dye"])
    with config_error("the array has the shape \\(16, 12\\)"):
        ArmonParameters(test="Sod", N=(16, 12), scalars=[tag])
    with config_error("the scalar 'heavy' has the shape"):
        Problem.from_arrays(rho, 0 * rho, 0 * rho, p=rho, scalars={"heavy": np.ones((3, 3))})
    with config_error("not finite in float32"):
        ArmonParameters(test="Sod", N=(12, 16), data_type="float32", scalars=[Scalar("big", 1e300)])
    with config_error("use_fused_sweep=False"):
        ArmonParameters(test="Sod", N=(12, 16), scalars=[dye], use_fused_sweep=False)
    with config_error("scalar:nope"):
        ArmonParameters(test="Sod", N=(12, 16), scalars=[dye], image_at_end=True, image_quantity=["rho", "scalar:nope"])
    p = ArmonParameters(test="Sod", N=(12, 16), scalars=[dye], image_at_end=True, image_quantity=["scalar:dye", "rho"])
    assert p.image_quantity == ("scalar:dye", "rho") and p.image_reduce["scalar:dye"] == "mean"


def test_ranks_and_tile_groups_refuse_scalars(monkeypatch):
    import torch.distributed as dist
    from armon_amd import ArmonParameters, Scalar
    from armon_amd.multi_tile import TileGroup
    with config_error("tile group"):          # in its own constructor, before anything is created on a device
        TileGroup((2, 1), test="Sod", N=(16, 16), scalars=[Scalar("dye")])
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    with config_error("use_MPI=true"):
        ArmonParameters(test="Sod", N=(16, 16), scalars=[Scalar("dye")], use_MPI=True, P=(1, 1))


def test_a_run_with_scalars_takes_neither_the_pair_nor_the_graph():
    from armon_amd import ArmonParameters, Scalar
    from armon_amd.solver import graph_cycles_usable, pair_usable
    kw = dict(test="Sod", N=(64, 64), graph_cycles=True, silent=5, placement_min_bytes=0)
    plain, dyed = ArmonParameters(**kw), ArmonParameters(**kw, scalars=[Scalar("dye")])
    assert pair_usable(plain) and not pair_usable(dyed)
    monkey = type("D", (), {"owns_ctx": True})()
    plain._device = dyed._device = monkey
    assert graph_cycles_usable(plain) and not graph_cycles_usable(dyed)


# ---- headers and digests -------------------------------------------------------------------------------------------------

def implosion(**kw):
    from armon_amd import HalfPlane, Problem, State
    return Problem("implosion", State(1., p=1.), [(HalfPlane((1, 1), 0.15), State(0.125, p=0.14))], domain_size=(0.3, 0.3),
                   maxtime=2.5, samples=4, **kw)


def test_digests_and_headers_without_scalars_are_todays():
    from armon_amd import ArmonParameters, checkpoint
    # recorded from the commit before passive scalars existed
    p = ArmonParameters(test=implosion(), N=(16, 16))
    assert p.test.digest == "e1c6f291115ab960f3b5c9c4e7f99891c868e5791c73340129568c83fee49b0d"
    assert "scalars" not in p.test.description
    p32 = ArmonParameters(test=implosion(), N=(16, 16), data_type="float32", gravity=(0., -1.))
    assert p32.test.digest == "a5c575bc49e637d0c15fe7c2618112f59bda36a68597b9db86eb57ac1d81bb8f"
    plain = checkpoint.bit_options(ArmonParameters(test="Sod", N=(16, 16)))
    assert json.dumps(plain, sort_keys=True) == (
        '{"Dt": "0x0.0p+0", "N": [16, 16], "axis_splitting": "Sequential", "cfl": "0x1.e666666666666p-1", "cst_dt": false, '
        '"data_type": "float64", "domain_size": ["0x1.0000000000000p+0", "0x1.0000000000000p+0"], "eos": "perfect_gas", '
        '"exact_arithmetic": false, "origin": ["0x0.0p+0", "0x0.0p+0"], "periodic": [false, false], "projection": "euler_2nd", '
        '"riemann_limiter": "minmod", "scheme": "GAD", "test": "Sod", "use_fused_sweep": true}')
    assert checkpoint.plane_names(p) == ("rho", "u", "v", "E")
    assert checkpoint.plane_names(ArmonParameters(test="Sod", N=(16, 16), use_fused_sweep=False)) == ("rho", "u", "v", "E", "c")


def test_scalars_enter_the_digest_the_header_and_the_planes():
    from armon_amd import ArmonParameters, Disc, Scalar, checkpoint
    dye = Scalar("dye", 0., [(Disc((0.1, 0.1), 0.05), 1.)])
    p = ArmonParameters(test=implosion(scalars=[dye]), N=(16, 16), scalars=[Scalar("tag", 2.)])
    d = p.test.description
    assert [s["name"] for s in d["scalars"]] == ["dye", "tag"] and d["scalars"][1]["background"] == (2.).hex()
    assert p.test.digest == hashlib.sha256(json.dumps(d, sort_keys=True).encode("utf-8")).hexdigest()
    assert p.test.digest != ArmonParameters(test=implosion(), N=(16, 16)).test.digest
    other = ArmonParameters(test=implosion(scalars=[Scalar("dye", 0., [(Disc((0.1, 0.1), 0.06), 1.)])]), N=(16, 16), scalars=[Scalar("tag", 2.)])
    assert other.test.digest != p.test.digest                         # another dye is another problem
    opts = checkpoint.bit_options(p)
    assert opts["scalars"] == ["dye", "tag"]
    assert checkpoint.plane_names(p) == ("rho", "u", "v", "E", "s:dye", "s:tag")
    built_in = ArmonParameters(test="Sod", N=(16, 16), scalars=[dye])
    assert checkpoint.bit_options(built_in)["scalars"] == ["dye"] and checkpoint.bit_options(built_in)["test"] == "Sod"


def test_check_compatible_refuses_other_scalar_names():
    from armon_amd import ArmonParameters, Scalar, checkpoint, compare
    dyed = ArmonParameters(test="Sod", N=(16, 16), scalars=[Scalar("dye")])
    plain = ArmonParameters(test="Sod", N=(16, 16))
    header = dict(checkpoint.bit_options(dyed), cycle=0, time=(0.).hex())
    checkpoint.check_compatible(dyed, header, "file")
    with config_error("scalars = \\['dye'\\], this run has scalars = \\[\\]"):
        checkpoint.check_compatible(plain, header, "file")
    with config_error("scalars = \\['dye'\\], this run has scalars = \\['ink'\\]"):
        checkpoint.check_compatible(ArmonParameters(test="Sod", N=(16, 16), scalars=[Scalar("ink")]), header, "file")
    with config_error("scalars = \\[\\], this run has scalars = \\['dye'\\]"):
        checkpoint.check_compatible(dyed, dict(checkpoint.bit_options(plain), cycle=0, time=(0.).hex()), "file")
    with config_error("scalars"):
        checkpoint.check_same_scalars(ArmonParameters(test="Sod", N=(16, 16), scalars=[Scalar("a"), Scalar("b")]),
                                      {"scalars": ["b", "a"]}, "the other grid")        # plane order is part of it


def test_a_damaged_scalars_key_is_an_io_error(tmp_path):
    from armon_amd import checkpoint
    from armon_amd._lib import SolverException
    good = dict(N=[4, 4], data_type="float64", planes=["rho"], digests={"rho": "0"}, cycle=0, time=(0.).hex(), current_dt=(0.).hex(),
                next_cycle_dt=(0.).hex(), pending_dt=None)
    checkpoint._check_header(dict(good, scalars=["dye"]), "file")
    for bad in ([], ["a:b"], [""], "dye", ["a"] * 5):
        with pytest.raises(SolverException, match="damaged checkpoint header: scalars"):
            checkpoint._check_header(dict(good, scalars=bad), "file")


def test_the_abi_declares_the_scalar_entry_points():
    from armon_amd._lib import SIGNATURES
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "armon_hip.h")).read()
    assert "#define ARMON_MAX_SCALARS 4" in header
    for name in ("sweep_scalars", "sweep_scalars_f32", "init_scalar_regions", "init_scalar_regions_f32"):
        assert re.search(r"ARMON_API int armon_hip_%s\(" % name, header), name
        assert "armon_hip_" + name in SIGNATURES
