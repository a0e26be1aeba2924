"""Derived fields and in-situ images, the parts that need no GPU: the ``image_*`` options, ``derived.render``, the PNG writer
and reader of io.py, and the numpy restatement of the per-cell rule on a field whose derivatives are known."""
import struct
import zlib

import numpy as np
import pytest

import armon_amd
from armon_amd import ArmonParameters, SolverException
from armon_amd import derived
from armon_amd import io as aio


def params(**kw):
    return ArmonParameters(test="Sedov", N=(64, 48), silent=5, **kw)


# ---- options ---------------------------------------------------------------------------------------------------------------
def test_defaults_resolve_as_documented():
    p = params()
    assert (p.image_step, p.image_at_end, p.state_image) == (0, False, False)
    assert p.image_quantity == ("grad_rho",) and p.image_reduce == {"grad_rho": "max"}
    assert p.image_transfer == {"grad_rho": "schlieren"} and p.image_range is None and p.image_file == "image"
    assert p.image_factor == (1, 1)
    p = params(image_step=5, image_quantity=["grad_rho", "vorticity", "mach"])
    assert p.state_image and p.use_fused_sweep
    assert p.image_quantity == ("grad_rho", "vorticity", "mach")
    assert p.image_reduce == {"grad_rho": "max", "vorticity": "mean", "mach": "mean"}
    assert p.image_transfer == {"grad_rho": "schlieren", "vorticity": "linear", "mach": "linear"}
    p = params(image_at_end=True, image_quantity="mach", image_reduce="min", image_transfer="log", image_range=(0.5, 2),
               image_file="frame", image_coarsen=(4, 2))
    assert p.state_image and p.image_quantity == ("mach",) and p.image_reduce == {"mach": "min"}
    assert p.image_transfer == {"mach": "log"} and p.image_range == (0.5, 2.0) and p.image_file == "frame"
    assert p.image_factor == (4, 2)
    p = params(image_quantity=["grad_rho", "p"], image_reduce={"p": "max"}, image_transfer={"grad_rho": "linear"})
    assert p.image_reduce == {"grad_rho": "max", "p": "max"} and p.image_transfer == {"grad_rho": "linear", "p": "linear"}


@pytest.mark.parametrize("N, factor", [((16384, 16384), 8), ((1000, 300), 1), ((5000, 100), 4), ((2048, 2048), 1), ((2049, 7), 2)])
def test_image_coarsen_default(N, factor):
    assert ArmonParameters(test="Sod", N=N, silent=5).image_factor == (factor, factor)


def test_image_coarsen_follows_output_coarsen_unless_given():
    assert params(output_coarsen=(4, 2)).image_factor == (4, 2)
    assert params(output_coarsen=(4, 2), image_coarsen=8).image_factor == (8, 8)


BAD = [dict(image_step=-1), dict(image_step=1.5), dict(image_step=True), dict(image_step="3"),
       dict(image_at_end="yes"), dict(image_at_end=1),
       dict(image_quantity="schlieren"), dict(image_quantity=["rho", "nope"]), dict(image_quantity=[]), dict(image_quantity=3),
       dict(image_quantity=["rho", "rho"]), dict(image_quantity=[1, 2]),
       dict(image_quantity=["rho", "p", "e", "speed", "mach", "grad_rho", "vorticity", "divergence", "rho"]),
       dict(image_reduce="median"), dict(image_reduce=1), dict(image_reduce={"rho": "max"}), dict(image_reduce={"grad_rho": "avg"}),
       dict(image_coarsen=0), dict(image_coarsen=-2), dict(image_coarsen=1.5), dict(image_coarsen=(2, 0)), dict(image_coarsen=(1, 2, 3)),
       dict(image_coarsen="4"),
       dict(image_transfer="gamma"), dict(image_transfer=2), dict(image_transfer={"rho": "linear"}), dict(image_transfer={"grad_rho": "cube"}),
       dict(image_range=(1, 1)), dict(image_range=(2, 1)), dict(image_range=(0, float("inf"))), dict(image_range=(float("nan"), 1)),
       dict(image_range=(1, 2, 3)), dict(image_range=5), dict(image_range=("a", "b")), dict(image_range=(False, True)),
       dict(image_file=""), dict(image_file="a/b"), dict(image_file=3)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v!r}" for d in BAD for k, v in d.items()])
def test_bad_image_options_are_configuration_errors(bad):
    with pytest.raises(SolverException) as e:
        params(**bad)
    assert e.value.category == "config"


def test_images_are_refused_for_ranks_of_a_process_group(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    params(use_MPI=True, image_quantity="mach")         # the options alone take no frame
    for kw in (dict(image_step=2), dict(image_at_end=True)):
        with pytest.raises(SolverException) as e:
            params(use_MPI=True, **kw)
        assert e.value.category == "config" and "image_step" in e.value.msg and "use_MPI" in e.value.msg


def test_graph_replay_steps_aside_for_image_frames():
    import types

    def usable(**kw):
        p = ArmonParameters(test="Sod", N=(8, 8), graph_cycles=True, silent=5, **kw)
        p._device = types.SimpleNamespace(owns_ctx=True)
        return armon_amd.solver.graph_cycles_usable(p)
    assert usable() and usable(image_quantity="mach")
    assert not usable(image_step=3) and not usable(image_at_end=True)


def test_a_misaligned_image_factor_of_a_tile_is_a_configuration_error():
    ArmonParameters(test="Sod", N=(48, 40), silent=5, tile_of=(1, (2, 2)), image_step=2, image_coarsen=4)
    ArmonParameters(test="Sod", N=(48, 40), silent=5, tile_of=(1, (2, 2)), image_coarsen=7)       # no frame is taken
    with pytest.raises(SolverException) as e:
        ArmonParameters(test="Sod", N=(48, 40), silent=5, tile_of=(1, (2, 2)), image_step=2, image_coarsen=7)
    assert e.value.category == "config"


def test_solver_stats_has_an_images_field_with_a_default():
    s = armon_amd.solver.SolverStats(1.0, 0.1, 3, 0.5, 100, 1.0)
    assert s.images == []
    assert armon_amd.solver.SolverStats(1.0, 0.1, 3, 0.5, 100, 1.0, images=["a.png"]).images == ["a.png"]


def test_request_normalisation():
    assert derived.QUANTITIES == ("rho", "p", "e", "speed", "mach", "grad_rho", "vorticity", "divergence")
    assert derived.normalize_request("rho") == (("rho",), ("mean",))
    assert derived.normalize_request(["rho", "p"], {"p": "min"}) == (("rho", "p"), ("mean", "min"))
    for bad in (([], "mean"), (["x"], "mean"), (["rho"], "sum"), (["rho"], {"p": "max"}), (["rho", "rho"], "mean")):
        with pytest.raises(SolverException):
            derived.normalize_request(*bad)


# ---- render ----------------------------------------------------------------------------------------------------------------
def test_render_linear_with_automatic_and_fixed_range():
    plane = np.array([[0., 1., 2.], [3., 4., 8.]])
    img = derived.render(plane)
    assert img.dtype == np.uint8 and img.shape == (2, 3)
    # row 0 of the plane is the bottom row of the image; 255 d / 8, rounded half to even
    assert img.tolist() == [[96, 128, 255], [0, 32, 64]]
    img = derived.render(plane, lo=1, hi=3)
    assert img.tolist() == [[255, 255, 255], [0, 0, 128]]                   # clipped on both sides; 127.5 rounds to 128
    assert derived.render(plane.astype(np.float32)).tolist() == derived.render(plane).tolist()


def test_render_log():
    plane = np.array([[1e-3, 1e-2, 1e-1, 1., 0., -5.]])
    img = derived.render(plane, transfer="log")
    # zero and negative values are clipped at the smallest positive value, 1e-3 -> black
    assert img.tolist() == [[0, 85, 170, 255, 0, 0]]
    img = derived.render(plane, lo=1e-2, hi=1., transfer="log")
    assert img.tolist() == [[0, 0, 128, 255, 0, 0]]
    assert derived.render(np.array([[0., -1.]]), transfer="log").tolist() == [[0, 0]]      # no positive value at all


def test_render_schlieren_is_dark_where_the_gradient_is_large():
    plane = np.array([[0., 0.1, 1.0], [0.05, 0.5, 0.2]])
    img = derived.render(plane, transfer="schlieren")
    want = np.rint(255.0 * np.exp(-15.0 * plane / 1.0)).astype(np.uint8)[::-1]
    assert np.array_equal(img, want)
    assert img[1, 0] == 255 and img[1, 2] == 0 and img[0, 0] == int(np.rint(255 * np.exp(-0.75)))
    fixed = derived.render(plane, lo=0., hi=0.5, transfer="schlieren")
    assert np.array_equal(fixed, np.rint(255.0 * np.exp(-15.0 * np.clip(plane / 0.5, 0, 1))).astype(np.uint8)[::-1])


@pytest.mark.parametrize("transfer", ["linear", "log", "schlieren"])
def test_render_nan_pixels_and_constant_planes(transfer):
    plane = np.array([[1., np.nan, 4.], [np.inf, 2., -np.inf]])
    with np.errstate(all="raise"):                      # nothing is divided by zero, no invalid operation escapes
        img = derived.render(plane, transfer=transfer)
        flat = derived.render(np.full((3, 4), 2.5), transfer=transfer)
        nothing = derived.render(np.full((2, 2), np.nan), transfer=transfer)
    assert img[1, 1] == 0 and img[0, 0] == 0 and img[0, 2] == 0             # the non-finite pixels (rows flipped)
    top, bottom = (0, 255) if transfer == "schlieren" else (255, 0)
    assert img[1, 2] == top and img[1, 0] == bottom                         # the range is the finite one: 1 .. 4
    assert flat.shape == (3, 4) and (flat == (255 if transfer == "schlieren" else 0)).all()
    assert (nothing == 0).all()


def test_render_refuses_an_unknown_transfer():
    with pytest.raises(SolverException):
        derived.render(np.zeros((2, 2)), transfer="gamma")


# ---- PNG -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (257, 130)])
def test_png_round_trip(tmp_path, shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    path = str(tmp_path / "a.png")
    assert aio.write_png_gray8(path, img) == path
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    # walk the chunks by hand: length, type, payload, CRC-32 of type + payload
    at, kinds = 8, []
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + payload) & 0xffffffff
        kinds.append(kind)
        if kind == b"IHDR":
            assert struct.unpack(">IIBBBBB", payload) == (shape[1], shape[0], 8, 0, 0, 0, 0)
        at += 12 + n
    assert at == len(data) and kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and b"IDAT" in kinds
    raw = zlib.decompress(b"".join(p for k, p, ok in aio.read_png_chunks(path) if k == b"IDAT"))
    assert len(raw) == shape[0] * (shape[1] + 1) and set(raw[::shape[1] + 1]) == {0}      # filter 0 in front of every row
    back = aio.read_png_gray8(path)
    assert back.dtype == np.uint8 and np.array_equal(back, img)


def test_png_reader_refuses_damage_and_writer_refuses_other_arrays(tmp_path):
    path = str(tmp_path / "a.png")
    aio.write_png_gray8(path, np.arange(12, dtype=np.uint8).reshape(3, 4))
    data = bytearray(open(path, "rb").read())
    data[20] ^= 1                                       # inside IHDR: its CRC no longer matches
    open(path, "wb").write(bytes(data))
    with pytest.raises(ValueError):
        aio.read_png_gray8(path)
    open(path, "wb").write(b"not a png")
    with pytest.raises(ValueError):
        aio.read_png_gray8(path)
    for bad in (np.zeros((2, 2)), np.zeros(4, dtype=np.uint8), np.zeros((0, 3), dtype=np.uint8)):
        with pytest.raises(ValueError):
            aio.write_png_gray8(path, bad)


# ---- the numpy restatement of the rule -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_planes_on_a_field_with_known_derivatives(dtype):
    T = dtype
    ny, nx, dx, dy = 6, 9, T(0.25), T(0.5)
    X = (np.arange(nx, dtype=T)[None, :] * dx) + np.zeros((ny, 1), dtype=T)
    Y = (np.arange(ny, dtype=T)[:, None] * dy) + np.zeros((1, nx), dtype=T)
    rho, u, v = T(1) + T(2) * X + T(4) * Y, T(3) * Y, T(5) * X           # linear: every difference quotient is exact
    E = T(2) + T(0.5) * (u * u + v * v)
    d = derived.reference_planes(rho, u, v, E, dx, dy, 1.4)
    assert all(a.dtype == dtype and a.shape == (ny, nx) for a in d.values())
    assert np.array_equal(d["grad_rho"], np.full((ny, nx), np.sqrt(T(20)), dtype=T))       # one-sided at the edges too
    assert np.array_equal(d["vorticity"], np.full((ny, nx), 2, dtype=T))
    assert np.array_equal(d["divergence"], np.zeros((ny, nx), dtype=T))
    assert np.allclose(d["e"], 2) and np.allclose(d["p"], 0.4 * rho * 2, rtol=1e-6)
    assert np.allclose(d["mach"], d["speed"] / np.sqrt(1.4 * d["p"] / rho), rtol=1e-6)
    one = derived.reference_planes(rho[:1, :1], u[:1, :1], v[:1, :1], E[:1, :1], dx, dy, 1.4)      # no neighbour at all
    assert one["grad_rho"][0, 0] == 0 and one["vorticity"][0, 0] == 0 and one["divergence"][0, 0] == 0
