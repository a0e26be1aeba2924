"""Packed checkpoints on the GPU (``checkpoint_compress`` / ``save_state(compress=True)``, file version 2): a run restarted
from one continues bit for bit, a packed file expands to the unpacked file of the same state byte for byte whatever the
decomposition that wrote it, loads into any decomposition, and compares like the unpacked one. The chunks are predicted
with the codec restated in tests/xorplane_restated.py, the file is parsed here from its description, never through the
package's reader."""
import json
import os

import numpy as np
import pytest

import xorplane_restated as xr

pytestmark = pytest.mark.gpu

STATE = ("rho", "u", "v", "E")
OUT = STATE + ("p",)
N = (100, 76)                       # uneven: 3 x 1 and 2 x 2 tiles differ in size
DATA_OFFSET = 16 + 4096
PATHS = {"staged": dict(use_fused_sweep=False), "exact": dict(exact_arithmetic=True), "tuned": dict()}
CASES = {"Sedov": dict(test="Sedov", axis_splitting="Godunov"), "Bizarrium": dict(test="Bizarrium", axis_splitting="Sequential")}


def real_fields(grid, names=OUT):
    host = grid.device_to_host(names)
    return {k: grid.real_view(host[k]).copy() for k in names}


def run(**kw):
    import armon_amd
    kw.setdefault("silent", 5)
    stats = armon_amd.armon(armon_amd.ArmonParameters(return_data=True, **kw))
    return stats, real_fields(stats.data)


def assert_same(a, b, what=""):
    (sa, fa), (sb, fb) = a, b
    assert (sa.cycles, sa.final_time, sa.last_dt) == (sb.cycles, sb.final_time, sb.last_dt), what
    for k in OUT:
        assert fa[k].tobytes() == fb[k].tobytes(), (what, k)


def parse(path):
    """→ (version, header, index records as lists of 8 integers, the file's length)."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"ARMONCKP"
    version = int.from_bytes(raw[8:12], "little")
    header = json.loads(raw[16:16 + int.from_bytes(raw[12:16], "little")])
    records = []
    if version == 2:
        at, count = header["index_offset"], header["index_count"]
        assert header["codec"] == "xorplane16" and len(raw) == at + 64 * count
        records = np.frombuffer(raw[at:], dtype="<u8").reshape(count, 8).tolist()
    return version, header, records, len(raw)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("path", list(PATHS))
def test_a_run_restarted_from_a_packed_checkpoint_continues_bit_for_bit(tmp_path, path, case, dtype):
    kw = dict(N=(64, 52), data_type=dtype, **PATHS[path], **CASES[case])
    a = run(maxcycle=13, **kw)
    b = run(maxcycle=7, checkpoint_at_end=True, checkpoint_compress=True, output_dir=str(tmp_path), **kw)
    file = tmp_path / "checkpoint_000007.ckpt"
    version, header, records, _ = parse(file)
    assert b[0].cycles == 7 and version == 2 and header["cycle"] == 7
    assert header["planes"] == list(STATE) + ([] if kw.get("use_fused_sweep", True) else ["c"])
    assert len(records) == len(header["planes"])                      # one band: one chunk per plane
    c = run(maxcycle=13, restart_from=str(file), **kw)
    assert a[0].cycles == 13
    assert_same(c, a, "restart from a packed checkpoint")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_packed_file_expands_to_the_unpacked_one(tmp_path, dtype):
    from armon_amd import checkpoint
    stats, _ = run(N=N, test="Sedov", maxcycle=13, data_type=dtype)
    grid = stats.data
    a, b, b2, e = (str(tmp_path / n) for n in ("a.ckpt", "b.ckpt", "b2.ckpt", "e.ckpt"))
    grid.save_state(a)
    hb = grid.save_state(b, compress=True, band_rows=30)
    grid.save_state(b2, compress=True, band_rows=30)
    assert open(b, "rb").read() == open(b2, "rb").read()              # the stream is a function of the state and the bands
    assert parse(a)[0] == 1 and parse(b)[0] == 2
    plain = checkpoint.expand(b, e)
    assert open(e, "rb").read() == open(a, "rb").read()
    assert plain == parse(a)[1] and hb == parse(b)[1]
    assert os.path.getsize(b) < os.path.getsize(a)
    # chunks back to back from DATA_OFFSET, 8-byte aligned, in the order they were written: bands, then planes
    _, header, records, size = parse(b)
    at = DATA_OFFSET
    want = [(q, r0, rows) for r0, rows in ((0, 30), (30, 30), (60, 16)) for q in range(4)]
    assert len(records) == len(want)
    for (q, codec, col0, row0, wnx, wny, off, nbytes), (wq, r0, rows) in zip(records, want):
        assert (q, col0, row0, wnx, wny, off) == (wq, 0, r0, 100, rows, at)
        at += (nbytes + 7) // 8 * 8
    assert at == header["index_offset"]


@pytest.mark.parametrize("path", ["staged", "exact"])
def test_packed_files_do_not_depend_on_the_decomposition(tmp_path, path):
    """Files packed by 3 x 1 and 2 x 2 tile groups expand to the single block's unpacked file; the file packed by 2 x 2 loads
    into 3 x 1, into a single block and under another ghost width, and every restart ends where the uninterrupted run ends."""
    from armon_amd import checkpoint
    from armon_amd.multi_tile import TileGroup
    kw = dict(N=N, test="Sedov", axis_splitting="Godunov", silent=5, **PATHS[path])
    a = run(maxcycle=13, **kw)
    run(maxcycle=7, checkpoint_at_end=True, checkpoint_file="block", output_dir=str(tmp_path), **kw)
    block = open(tmp_path / "block_000007.ckpt", "rb").read()
    digests = parse(tmp_path / "block_000007.ckpt")[1]["digests"]
    for P in ((3, 1), (2, 2)):
        name = f"group{P[0]}{P[1]}"
        group = TileGroup(P, maxcycle=7, checkpoint_step=7, checkpoint_file=name, checkpoint_compress=True, output_dir=str(tmp_path), **kw)
        try:
            group.run()
        finally:
            group.close()
        version, header, records, _ = parse(tmp_path / f"{name}_000007.ckpt")
        assert version == 2 and header["digests"] == digests
        assert len(records) == P[0] * P[1] * len(header["planes"])
        checkpoint.expand(tmp_path / f"{name}_000007.ckpt", tmp_path / f"{name}.plain")
        assert open(tmp_path / f"{name}.plain", "rb").read() == block, P
    packed = str(tmp_path / "group22_000007.ckpt")
    group = TileGroup((3, 1), maxcycle=13, restart_from=packed, **kw)
    try:
        stats = group.run()
        assert_same((stats, group.gather(OUT)), a, "2 x 2 -> 3 x 1")
        header = group.load_state(packed)                              # the digests of what was loaded matched the header's
        names = tuple(header["planes"])
        assert ["%016x" % d for d in group.state_digest(names)] == [digests[f] for f in names]
    finally:
        group.close()
    assert_same(run(maxcycle=13, restart_from=packed, **kw), a, "2 x 2 -> block")
    assert_same(run(maxcycle=13, nghost=6, restart_from=packed, **kw), a, "2 x 2 -> block with another ghost width")


def test_a_chunk_that_would_expand_is_written_raw(tmp_path):
    """fp32 Sod_circ 100 x 76 after 13 cycles: smooth and fully 2-D, some planes encode to more than their raw bytes. The file
    holds, band by band and plane by plane, exactly what the restated codec predicts — the encoding where it is smaller, the
    raw plane otherwise — and is never larger than the unpacked file plus its index."""
    from armon_amd import checkpoint
    stats, fields = run(N=N, test="Sod_circ", axis_splitting="Strang", maxcycle=13, data_type="float32")
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    stats.data.save_state(a)
    stats.data.save_state(b, compress=True, band_rows=40)
    _, header, records, size = parse(b)
    raw = open(b, "rb").read()
    codecs = []
    it = iter(records)
    for r0, rows in ((0, 40), (40, 36)):
        for q, f in enumerate(STATE):
            cut = np.ascontiguousarray(fields[f][r0:r0 + rows])
            encoded, _ = xr.encode_fast(cut)
            want = encoded if len(encoded) < cut.nbytes else cut.tobytes()
            rq, codec, col0, row0, wnx, wny, off, nbytes = next(it)
            assert (rq, codec, col0, row0, wnx, wny, nbytes) == (q, int(len(encoded) < cut.nbytes), 0, r0, 100, rows, len(want)), (f, r0)
            assert raw[off:off + nbytes] == want, (f, r0)
            codecs.append(codec)
    assert 0 in codecs, "no plane of this state expands: the test no longer covers the raw fallback"
    assert size <= os.path.getsize(a) + 64 * len(records)
    checkpoint.expand(b, tmp_path / "e.ckpt")
    assert open(tmp_path / "e.ckpt", "rb").read() == open(a, "rb").read()
    c = run(N=N, test="Sod_circ", axis_splitting="Strang", maxcycle=20, data_type="float32", restart_from=b)
    assert_same(c, run(N=N, test="Sod_circ", axis_splitting="Strang", maxcycle=20, data_type="float32"), "restart with raw chunks")


def test_compare_state_takes_a_packed_file(tmp_path):
    """The records, and the listing, against the packed file are those against the unpacked one: for a block and for tile
    groups, for the same state and for a state that differs in every cell."""
    from armon_amd.multi_tile import TileGroup
    kw = dict(N=N, test="Sedov", axis_splitting="Godunov", silent=5)
    ref, _ = run(maxcycle=9, **kw)
    a, b = str(tmp_path / "a.ckpt"), str(tmp_path / "b.ckpt")
    ref.data.save_state(a)
    ref.data.save_state(b, compress=True, band_rows=20)
    same = ref.data.compare_state(b, rtol=0.0)
    assert not same.different and same == ref.data.compare_state(a, rtol=0.0)
    assert all(same[f].raw[:3] == (N[0] * N[1], 0, 0) for f in STATE)
    other, _ = run(maxcycle=13, **kw)
    want = other.data.compare_state(a, rtol=0.0, band_rows=7)
    assert want.different and other.data.compare_state(b, rtol=0.0) == want
    assert other.data.compare_state(b, rtol=1e-3, atol={"rho": 1e-6, "u": 0.0, "v": 0.0, "E": 1e-9}, limit=3) == \
        other.data.compare_state(a, rtol=1e-3, atol={"rho": 1e-6, "u": 0.0, "v": 0.0, "E": 1e-9}, limit=3)
    assert other.data.compare_state(b, rtol=0.0, names=("E", "u"), limit=0) == other.data.compare_state(a, rtol=0.0, names=("E", "u"), limit=0)
    for P in ((2, 2), (3, 1)):
        group = TileGroup(P, maxcycle=13, **kw)
        try:
            group.run()
            assert group.compare_state(b, rtol=0.0) == want, P
        finally:
            group.close()


def test_a_flipped_payload_byte_is_a_digest_mismatch(tmp_path):
    import armon_amd
    kw = dict(N=N, test="Sedov", axis_splitting="Godunov")
    stats, _ = run(maxcycle=7, **kw)
    b = str(tmp_path / "b.ckpt")
    stats.data.save_state(b, compress=True)
    _, header, records, _ = parse(b)
    raw = bytearray(open(b, "rb").read())
    q, codec, _, _, wnx, wny, off, nbytes = records[0]
    assert codec == 1
    words = off + 2 * xr.shape_of(wny, wnx, 8)[2]
    assert words < off + nbytes
    raw[words] ^= 0x02                                                # lane 1 of the chunk's first word: the tables still add up
    bad = str(tmp_path / "bad.ckpt")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(armon_amd.SolverException) as e:
        run(maxcycle=13, restart_from=bad, **kw)
    assert e.value.category == "io" and "digest mismatch" in e.value.msg and bad in e.value.msg
    raw[words] ^= 0x02
    raw[off + 3] ^= 0x01                                             # a base value
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(armon_amd.SolverException) as e:
        run(maxcycle=13, restart_from=bad, **kw)
    assert e.value.category == "io" and "digest mismatch" in e.value.msg


def test_the_default_writes_version_1(tmp_path):
    kw = dict(N=(64, 52), test="Sedov", axis_splitting="Godunov", maxcycle=7)
    stats, _ = run(checkpoint_at_end=True, output_dir=str(tmp_path), **kw)
    assert stats.data.params.checkpoint_compress is False
    a = str(tmp_path / "a.ckpt")
    stats.data.save_state(a)
    stats.data.save_state(str(tmp_path / "c.ckpt"), compress=False)
    by_option = open(tmp_path / "checkpoint_000007.ckpt", "rb").read()
    assert parse(a)[0] == 1 and by_option == open(a, "rb").read() == open(tmp_path / "c.ckpt", "rb").read()
    assert not any(k in parse(a)[1] for k in ("codec", "index_offset", "index_count"))
    packed, _ = run(checkpoint_compress=True, **kw)
    packed.data.save_state(str(tmp_path / "d.ckpt"))                   # None = take the option
    packed.data.save_state(str(tmp_path / "e.ckpt"), compress=False)
    assert parse(tmp_path / "d.ckpt")[0] == 2 and open(tmp_path / "e.ckpt", "rb").read() == by_option
