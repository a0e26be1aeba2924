#!/usr/bin/env python3
"""What a checkpoint costs on the device: armon_hip_state_pack with its digest over the four state planes, band by band into
device staging (the bands of checkpoint.py's pipeline), and the digest alone, against armon_hip_stream_copy4 on the same four
vectors in the same process (the same bytes: 4 read + 4 written), launches interleaved, event-timed, medians; and, once, the
wall time of a whole save_state and load_state (bound by the disk: for the record only). Prints ONE JSON line.

    python tools/checkpoint_bench.py [--n 16384] [--dtype float64] [--launches 30] [--no-io] [--dir DIR]

Bar: pack_ms <= copy4_ms * (1 + spread), spread = (max - min) / median of the copy over its repeats in this process."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import checkpoint  # noqa: E402
from armon_amd.solver import STATE_VARS, BlockGrid, init_test  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-io", action="store_true", help="skip the one timing of save_state / load_state")
    ap.add_argument("--dir", default=None, help="where the checkpoint of the save / load timing is written (removed afterwards)")
    a = ap.parse_args()
    params = armon_amd.ArmonParameters(test="Sod", N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0)
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    band_rows, bands = checkpoint._bands(params, 4, None)
    stage = dev.empty(4 * band_rows * a.n, params.data_type)
    digest = dev.zeros(8, np.uint64)
    t_pack, t_digest, t_copy = [], [], []
    for k in range(a.warmup + a.launches):
        dev.event_record(20)
        for r0, rows in bands:
            checkpoint._move(params, grid, STATE_VARS, (0, r0, a.n, rows), stage, digest)
        dev.event_record(21)
        for r0, rows in bands:
            checkpoint._move(params, grid, STATE_VARS, (0, r0, a.n, rows), None, digest)
        dev.event_record(22)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(23)
        if k >= a.warmup:
            t_pack.append(dev.event_elapsed_ms(20, 21))
            t_digest.append(dev.event_elapsed_ms(21, 22))
            t_copy.append(dev.event_elapsed_ms(22, 23))
    pack_ms, digest_ms, copy4_ms = median(t_pack), median(t_digest), median(t_copy)
    spread = (max(t_copy) - min(t_copy)) / copy4_ms
    item = np.dtype(params.data_type).itemsize
    res = {"tool": "checkpoint_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "launches": a.launches,
           "warmup": a.warmup, "band_rows": band_rows, "bands": len(bands),
           "pack_ms": round(pack_ms, 4), "pack_ms_min": round(min(t_pack), 4), "pack_ms_max": round(max(t_pack), 4),
           "digest_only_ms": round(digest_ms, 4),
           "copy4_ms": round(copy4_ms, 4), "copy4_ms_min": round(min(t_copy), 4), "copy4_ms_max": round(max(t_copy), 4),
           "copy4_spread": round(spread, 4), "pack_over_copy4": round(pack_ms / copy4_ms, 4),
           "pack_GBps": round(8 * a.n * a.n * item / pack_ms / 1e6, 1), "copy4_GBps": round(8 * nb / copy4_ms / 1e6, 1),
           "accepted": bool(pack_ms <= copy4_ms * (1 + spread))}
    stage.free()
    digest.free()
    if not a.no_io:
        with tempfile.TemporaryDirectory(dir=a.dir) as d:
            path = os.path.join(d, "bench.ckpt")
            dev.wait()
            t0 = time.perf_counter()
            grid.save_state(path)
            res["save_state_s"] = round(time.perf_counter() - t0, 2)
            res["file_bytes"] = os.path.getsize(path)
            t0 = time.perf_counter()
            grid.load_state(path)
            res["load_state_s"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
