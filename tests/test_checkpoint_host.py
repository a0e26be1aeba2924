"""Checkpoint / restart, the parts that need no GPU: the file header, the options, the digest's host restatement and the
sanity return of the new entry points."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import armon_amd
from armon_amd import checkpoint as ck
from armon_amd._lib import SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import graph_cycles_usable


def header_of(params, **over):
    h = dict(ck.bit_options(params))
    h.update(version=ck.VERSION, planes=list(ck.plane_names(params)), cycle=7, time=ck.hexfloat(0.1), current_dt=ck.hexfloat(1e-3),
             next_cycle_dt=ck.hexfloat(math.inf), pending_dt=ck.hexfloat(0.0123456789),
             digests={f: f"{k:016x}" for k, f in enumerate(ck.plane_names(params))})
    h.update(over)
    return h


def write_file(path, params, header, fill=0.5):
    nx, ny = params.global_grid
    with open(path, "wb") as f:
        ck.write_header(f, header)
        f.write(np.full(len(ck.plane_names(params)) * nx * ny, fill, dtype=params.data_type).tobytes())


@pytest.mark.parametrize("value", [0.1, 1e-300, 5e-324, -0.0, math.inf, 1 / 3, float(np.float32(0.1))])
def test_hex_floats_carry_every_bit(value):
    back = ck.unhex(ck.hexfloat(value))
    assert np.float64(back).tobytes() == np.float64(value).tobytes()


@pytest.mark.parametrize("fused", [True, False])
def test_header_round_trip(tmp_path, fused):
    params = ArmonParameters(test="Sedov", N=(10, 6), use_fused_sweep=fused, axis_splitting="Godunov")
    header = header_of(params, initial_mass=ck.hexfloat(1.25), initial_energy=ck.hexfloat(3.5))
    path = tmp_path / "a.ckpt"
    write_file(path, params, header)
    raw = open(path, "rb").read()
    assert raw[:8] == b"ARMONCKP" and int.from_bytes(raw[8:12], "little") == ck.VERSION
    assert len(raw) == 16 + 4096 + (4 if fused else 5) * 60 * 8
    back = ck.read_header(path)
    assert back == header
    assert ck.unhex(back["next_cycle_dt"]) == math.inf and ck.unhex(back["pending_dt"]) == 0.0123456789
    assert back["planes"] == ["rho", "u", "v", "E"] + ([] if fused else ["c"])
    ck.check_compatible(params, back, path)


def test_damaged_files_are_io_errors(tmp_path):
    params = ArmonParameters(test="Sod", N=(8, 8))
    path = tmp_path / "a.ckpt"
    write_file(path, params, header_of(params))
    raw = open(path, "rb").read()
    for name, data in (("short", raw[:-1]), ("magic", b"ARMONCKQ" + raw[8:]), ("version", raw[:8] + b"\x09" + raw[9:]),
                       ("tiny", raw[:5])):
        bad = tmp_path / name
        open(bad, "wb").write(data)
        with pytest.raises(SolverException) as e:
            ck.read_header(bad)
        assert e.value.category == "io", name
    with pytest.raises(SolverException) as e:
        ck.read_header(tmp_path / "missing.ckpt")
    assert e.value.category == "io"


@pytest.mark.parametrize("change", [dict(N=None), dict(N=[8]), dict(N=[8, "8"]), dict(N=[0, 8]), dict(planes=None), dict(planes="rho"),
                                    dict(planes=[1, 2]), dict(data_type=None), dict(data_type="int8"), dict(data_type=[1]),
                                    dict(digests=None), dict(digests={"rho": "0"}), dict(pending_dt=...), dict(pending_dt=1.5),
                                    dict(pending_dt="zz"), dict(time=None), dict(current_dt="0x"), dict(next_cycle_dt=3),
                                    dict(cycle=None), dict(cycle="7"), dict(cycle=-1), dict(initial_mass="0x1p0")])
def test_a_header_that_parses_but_is_damaged_is_an_io_error(tmp_path, change):
    params = ArmonParameters(test="Sod", N=(8, 8))
    header = header_of(params)
    for k, v in change.items():
        if v is None or v is ...:
            del header[k]
        else:
            header[k] = v
    path = tmp_path / "a.ckpt"
    write_file(path, params, header)
    with pytest.raises(SolverException) as e:
        ck.read_header(path)
    assert e.value.category == "io", change
    with open(path, "wb") as f:                     # JSON that is not an object at all
        ck.write_header(f, [1, 2, 3])
    with pytest.raises(SolverException) as e:
        ck.read_header(path)
    assert e.value.category == "io"


def test_short_writes_are_completed_or_reported(tmp_path, monkeypatch):
    import os
    data = bytes(range(256)) * 4
    real, calls = os.pwrite, []

    def three_bytes_at_a_time(fd, buf, off):
        calls.append(off)
        return real(fd, bytes(buf[:3]), off)
    fd = os.open(tmp_path / "f", os.O_RDWR | os.O_CREAT)
    try:
        monkeypatch.setattr(os, "pwrite", three_bytes_at_a_time)
        ck._pwrite_all(fd, memoryview(data), 10)
        monkeypatch.setattr(os, "pwrite", lambda fd, buf, off: 0)
        with pytest.raises(OSError):
            ck._pwrite_all(fd, memoryview(data), 10)
    finally:
        monkeypatch.undo()
        os.close(fd)
    assert len(calls) == -(-len(data) // 3) and open(tmp_path / "f", "rb").read() == bytes(10) + data


def test_a_periodic_group_does_not_take_a_plain_file():
    plain = ArmonParameters(test="Sod", N=(16, 16), tile_of=(0, (2, 1)))
    wrapped = ArmonParameters(test="Sod", N=(16, 16), tile_of=(0, (2, 1)), periodic=(True, False))
    with pytest.raises(SolverException) as e:
        ck.check_compatible(wrapped, header_of(plain), "x.ckpt")
    assert e.value.category == "config" and "periodic" in e.value.msg


@pytest.mark.parametrize("field,other", [("N", dict(N=(8, 10))), ("data_type", dict(data_type=np.float32)),
                                         ("riemann_limiter", dict(riemann_limiter="superbee")),
                                         ("use_fused_sweep", dict(use_fused_sweep=False)),
                                         ("exact_arithmetic", dict(exact_arithmetic=True)),
                                         ("axis_splitting", dict(axis_splitting="Strang")), ("cfl", dict(cfl=0.3)),
                                         ("test", dict(test="Sedov"))])
def test_a_header_from_another_run_is_a_config_error_naming_the_field(tmp_path, field, other):
    base = dict(test="Sod", N=(16, 16))
    header = header_of(ArmonParameters(**{**base, **other}))
    with pytest.raises(SolverException) as e:
        ck.check_compatible(ArmonParameters(**base), header, "x.ckpt")
    assert e.value.category == "config" and field in e.value.msg
    # what may differ: ghost width, decomposition, limits of the run, output options
    free = ArmonParameters(**base, nghost=6, maxcycle=100, maxtime=1.0, tile_of=(1, (2, 2)), output_dir="elsewhere")
    ck.check_compatible(free, header_of(ArmonParameters(**base)), "x.ckpt")


def test_a_checkpoint_that_leaves_nothing_to_run_is_refused():
    params = ArmonParameters(test="Sod", N=(8, 8), maxcycle=7)
    with pytest.raises(SolverException) as e:
        ck.check_compatible(params, header_of(params), "x.ckpt")
    assert e.value.category == "config"
    params = ArmonParameters(test="Sod", N=(8, 8), maxtime=0.05)
    with pytest.raises(SolverException) as e:
        ck.check_compatible(params, header_of(params), "x.ckpt")
    assert e.value.category == "config"


def test_option_defaults_and_validation():
    p = ArmonParameters(test="Sod", N=(8, 8))
    assert (p.checkpoint_step, p.checkpoint_file, p.checkpoint_at_end, p.restart_from) == (0, "checkpoint", False, None)
    p = ArmonParameters(test="Sod", N=(8, 8), checkpoint_step=3, checkpoint_file="ck", checkpoint_at_end=True,
                        restart_from="a.ckpt", output_dir="out")
    assert (p.checkpoint_step, p.checkpoint_file, p.checkpoint_at_end, p.restart_from) == (3, "ck", True, "a.ckpt")
    assert ck.checkpoint_path(p, 12) == "out/ck_000012.ckpt"
    for bad in (dict(checkpoint_step=-1), dict(checkpoint_step=1.5), dict(restart_from="a", compare=True),
                dict(restart_from="a", is_ref=True), dict(checkpoint_file="")):
        with pytest.raises(SolverException) as e:
            ArmonParameters(test="Sod", N=(8, 8), **bad)
        assert e.value.category == "config", bad


def test_graph_replay_steps_aside_for_checkpoints_only():
    def usable(**kw):
        p = ArmonParameters(test="Sod", N=(8, 8), graph_cycles=True, silent=5, **kw)
        p._device = types.SimpleNamespace(owns_ctx=True)          # no context is needed to decide
        return graph_cycles_usable(p)
    assert usable() is True                                      # the defaults leave it as it was
    assert usable(animation_step=2) is False
    assert usable(checkpoint_step=2) is False
    assert usable(checkpoint_at_end=True) is False
    assert usable(restart_from="a.ckpt") is False
    assert graph_cycles_usable(ArmonParameters(test="Sod", N=(8, 8))) is False


def test_new_entry_points_are_bound_and_refuse_a_null_context():
    from armon_amd._lib import SIGNATURES
    for name in ("state_pack", "state_unpack"):
        for suffix in ("", "_f32"):
            assert "armon_hip_" + name + suffix in SIGNATURES
    L = armon_amd.lib()
    vars_ = (C.c_void_p * 1)()
    for fn in (L.armon_hip_state_pack, L.armon_hip_state_unpack, L.armon_hip_state_pack_f32, L.armon_hip_state_unpack_f32):
        assert fn(None, 16, 4, 8, 8, 1, vars_, 0, 0, 8, 8, 0, 8, None, None) == 1


def mix64_int(z):
    """The issue's mix64 in Python integers."""
    m = (1 << 64) - 1
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 & m
    z ^= z >> 27
    z = z * 0x94d049bb133111eb & m
    return z ^ (z >> 31)


def test_digest_helper_against_hand_computed_terms():
    m = (1 << 64) - 1
    assert mix64_int(0) == 0
    assert int(ck.mix64(np.uint64(1))) == mix64_int(1)
    # three terms by hand: (value, k, gx, gy, NX)
    one, mzero, f32 = 0x3ff0000000000000, 0x8000000000000000, 0x3fc00000     # 1.0, -0.0, float32(1.5)
    t0 = mix64_int((one + mix64_int(8 * 0 + 0 + 1)) & m)                       # cell 0 of plane 0
    t1 = mix64_int((mzero + mix64_int(8 * (2 * 7 + 3) + 2 + 1)) & m)           # cell (3, 2) of a 7-wide domain, plane 2
    t2 = mix64_int((f32 + mix64_int(8 * (1 * 5 + 4) + 3 + 1)) & m)             # fp32: 32 bits zero-extended
    assert ck.digest_reference(np.array([[1.0]]), 0) == t0
    assert ck.digest_reference(np.array([[-0.0]]), 2, global_nx=7, origin=(3, 2)) == t1
    assert ck.digest_reference(np.array([[1.5]], dtype=np.float32), 3, global_nx=5, origin=(4, 1)) == t2
    assert ck.digest_reference(np.array([[0.0]]), 2, global_nx=7, origin=(3, 2)) != t1          # -0.0 is not +0.0
    # a sum of terms, mod 2^64, and additive over a split of the domain
    a = np.arange(12, dtype=np.float64).reshape(3, 4) - 5
    whole = ck.digest_reference(a, 1)
    terms = sum(mix64_int((int(a[j, i].view(np.uint64)) + mix64_int(8 * (j * 4 + i) + 2)) & m) for j in range(3) for i in range(4))
    assert whole == terms & m
    parts = ck.digest_reference(a[:, :3], 1, global_nx=4) + ck.digest_reference(a[:, 3:], 1, global_nx=4, origin=(3, 0))
    assert whole == parts & m
