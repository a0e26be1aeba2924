#!/usr/bin/env python3
"""What a packed checkpoint costs: on Sedov and Sod states a few hundred cycles in, armon_hip_plane_encode and
armon_hip_plane_decode over the bands of checkpoint.py's pipeline (512 rows at 16384² fp64, four planes), next to
armon_hip_state_pack on the same bands and to armon_hip_stream_copy4 on the same four vectors, launches interleaved,
event-timed, medians, in one process; then the wall time and the file size of whole save_state / load_state, packed and
unpacked, three of each. Prints ONE JSON line (kept as profiles/checkpoint_codec_bench.json).

    python tools/codec_bench.py [--n 16384] [--dtype float64] [--cycles 300] [--launches 10] [--tests Sedov,Sod] [--dir DIR]

Bar: the median packed save_state of the Sedov state is no slower than the median unpacked one by more than the unpacked
saves' own spread, (max - min) / median over their three repeats."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import checkpoint, plane_codec  # noqa: E402
from armon_amd._lib import check  # noqa: E402
from armon_amd.solver import STATE_VARS  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def kernels(params, grid, launches, warmup):
    """Event-timed medians (ms, over all bands) of state_pack, plane_encode, plane_decode and stream_copy4 → dict."""
    dev, nx = params.device, params.N[0]
    item = params.data_type.itemsize
    nvars = len(STATE_VARS)
    band_rows, bands = checkpoint._bands(params, nvars, None)
    bound = plane_codec.bound(band_rows, nx, item)
    stage, back = dev.empty(nvars * band_rows * nx, params.data_type), dev.empty(band_rows * nx, params.data_type)
    enc, sizes, digest, status = dev.empty(nvars * bound, np.uint8), dev.zeros(8, np.uint64), dev.zeros(8, np.uint64), dev.zeros(2, np.uint32)
    encode, decode = params.fn("plane_encode"), params.fn("plane_decode")
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    t = {"pack": [], "encode": [], "decode": [], "copy4": []}
    encoded = 0
    for k in range(warmup + launches):
        ms = dict.fromkeys(t, 0.0)
        encoded = 0
        for r0, rows in bands:
            dev.event_record(20)
            checkpoint._move(params, grid, STATE_VARS, (0, r0, nx, rows), stage, digest)
            dev.event_record(21)
            check(encode(dev.ctx, C.c_void_p(stage.ptr), nvars, rows, nx, C.c_void_p(enc.ptr), bound, C.c_void_p(sizes.ptr)))
            dev.event_record(22)
            dev.wait()
            used = [int(v) for v in sizes.to_host()[:nvars]]
            encoded += sum(used)
            dev.event_record(23)
            for q in range(nvars):
                check(decode(dev.ctx, C.c_void_p(enc.ptr + q * bound), used[q], rows, nx, 0, 0, nx, rows, C.c_void_p(back.ptr),
                             C.c_void_p(status.ptr)))
            dev.event_record(24)
            dev.wait()
            ms["pack"] += dev.event_elapsed_ms(20, 21)
            ms["encode"] += dev.event_elapsed_ms(21, 22)
            ms["decode"] += dev.event_elapsed_ms(23, 24)
        dev.event_record(25)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(26)
        dev.wait()
        ms["copy4"] = dev.event_elapsed_ms(25, 26)
        if k >= warmup:
            for name in t:
                t[name].append(ms[name])
    assert status.to_host()[0] == 0
    for a in (stage, back, enc, sizes, digest, status):
        a.free()
    out = {"band_rows": band_rows, "bands": len(bands), "encoded_bytes": encoded, "raw_bytes": nvars * nx * params.N[1] * item}
    for name, v in t.items():
        out[name + "_ms"] = round(median(v), 4)
        out[name + "_ms_min"], out[name + "_ms_max"] = round(min(v), 4), round(max(v), 4)
    return out


def files(grid, directory, repeats=3):
    """Wall seconds of ``repeats`` save_state and load_state, unpacked and packed, interleaved → dict."""
    out = {}
    with tempfile.TemporaryDirectory(dir=directory) as d:
        t = {"save_s": [], "load_s": [], "packed_save_s": [], "packed_load_s": []}
        for _ in range(repeats):
            for prefix, compress in (("", False), ("packed_", True)):
                path = os.path.join(d, prefix + "bench.ckpt")
                grid.params.wait()
                t0 = time.perf_counter()
                grid.save_state(path, compress=compress)
                t[prefix + "save_s"].append(time.perf_counter() - t0)
                out[prefix + "file_bytes"] = os.path.getsize(path)
                t0 = time.perf_counter()
                grid.load_state(path)
                t[prefix + "load_s"].append(time.perf_counter() - t0)
                os.unlink(path)
        for name, v in t.items():
            out[name] = [round(x, 3) for x in v]
        spread = (max(t["save_s"]) - min(t["save_s"])) / median(t["save_s"])
        out["save_spread"] = round(spread, 4)
        out["packed_over_unpacked_save"] = round(median(t["packed_save_s"]) / median(t["save_s"]), 4)
        out["accepted"] = bool(median(t["packed_save_s"]) <= median(t["save_s"]) * (1 + spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--cycles", type=int, default=300)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tests", default="Sedov,Sod")
    ap.add_argument("--no-io", action="store_true", help="skip the save_state / load_state timings")
    ap.add_argument("--dir", default=None, help="where the checkpoints of the save / load timings are written (removed afterwards)")
    a = ap.parse_args()
    res = {"tool": "codec_bench", "N": [a.n, a.n], "dtype": a.dtype, "cycles": a.cycles, "launches": a.launches, "warmup": a.warmup,
           "states": {}}
    for test in a.tests.split(","):
        stats = armon_amd.armon(armon_amd.ArmonParameters(test=test, N=(a.n, a.n), data_type=a.dtype, maxcycle=a.cycles, silent=5,
                                                          return_data=True, placement_tries=0))
        grid = stats.data
        res["device"] = grid.params.device.name
        entry = kernels(grid.params, grid, a.launches, a.warmup)
        entry["ratio"] = round(entry["raw_bytes"] / entry["encoded_bytes"], 3)
        if not a.no_io:
            grid.params.maxcycle = a.cycles + 1          # load_state refuses a file that leaves the run nothing to do
            entry.update(files(grid, a.dir))
        res["states"][test] = entry
        del grid, stats
    if "Sedov" in res["states"] and "accepted" in res["states"]["Sedov"]:
        res["accepted"] = res["states"]["Sedov"]["accepted"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
