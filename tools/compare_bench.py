#!/usr/bin/env python3
"""What a state comparison costs on the device: armon_hip_state_compare over the four state planes against a dense reference in
device staging, band by band (the bands of checkpoint.py's pipeline), against armon_hip_stream_copy4 on the same four vectors in
the same process (the same bytes moved: the compare reads 4 + 4 planes, the copy reads 4 and writes 4), launches interleaved,
event-timed, medians; and, once each, the wall time of a whole compare_state(path) (bound by the disk and PCIe: for the record
only) and compare_state(other_grid). Prints ONE JSON line.

    python tools/compare_bench.py [--n 16384] [--dtype float64] [--launches 30] [--no-io] [--dir DIR]

Bar: compare_ms <= copy4_ms * (1 + spread), spread = (max - min) / median of the copy over its repeats in this process."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import checkpoint, compare  # noqa: E402
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
    ap.add_argument("--no-io", action="store_true", help="skip the one timing of compare_state(path) and compare_state(grid)")
    ap.add_argument("--dir", default=None, help="where the checkpoint of the file timing is written (removed afterwards)")
    a = ap.parse_args()
    params = armon_amd.ArmonParameters(test="Sod", N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0)
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    band_rows, bands = checkpoint._bands(params, 4, None)
    # the reference of every band: the state itself, packed once (a clean comparison: the case whose cost matters)
    stages, digest = [], dev.zeros(8, np.uint64)
    for r0, rows in bands:
        stage = dev.empty(4 * rows * a.n, params.data_type)
        checkpoint._move(params, grid, STATE_VARS, (0, r0, a.n, rows), stage, digest)
        stages.append(stage)
    diff = dev.empty(64, np.uint64)
    t_cmp, t_copy = [], []
    for k in range(a.warmup + a.launches):
        compare._reset(params, diff, 4)
        dev.event_record(20)
        for (r0, rows), stage in zip(bands, stages):
            compare._compare_window(params, grid, STATE_VARS, (0, r0, a.n, rows), stage.ptr, 1e-10, 0.0, diff)
        dev.event_record(21)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(22)
        if k >= a.warmup:
            t_cmp.append(dev.event_elapsed_ms(20, 21))
            t_copy.append(dev.event_elapsed_ms(21, 22))
    records = compare._records(params, diff, 4)
    assert all(r == (a.n * a.n, 0, 0, compare.NONE, 0, compare.NONE, 0, compare.NONE) for r in records), records
    cmp_ms, copy4_ms = median(t_cmp), median(t_copy)
    spread = (max(t_copy) - min(t_copy)) / copy4_ms
    item = np.dtype(params.data_type).itemsize
    res = {"tool": "compare_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "launches": a.launches,
           "warmup": a.warmup, "band_rows": band_rows, "bands": len(bands),
           "compare_ms": round(cmp_ms, 4), "compare_ms_min": round(min(t_cmp), 4), "compare_ms_max": round(max(t_cmp), 4),
           "copy4_ms": round(copy4_ms, 4), "copy4_ms_min": round(min(t_copy), 4), "copy4_ms_max": round(max(t_copy), 4),
           "copy4_spread": round(spread, 4), "compare_over_copy4": round(cmp_ms / copy4_ms, 4),
           "compare_GBps": round(8 * a.n * a.n * item / cmp_ms / 1e6, 1), "copy4_GBps": round(8 * nb / copy4_ms / 1e6, 1),
           "accepted": bool(cmp_ms <= copy4_ms * (1 + spread))}
    for s in stages + [digest, diff]:
        s.free()
    if not a.no_io:
        with tempfile.TemporaryDirectory(dir=a.dir) as d:
            path = os.path.join(d, "bench.ckpt")
            grid.save_state(path)
            dev.wait()
            t0 = time.perf_counter()
            clean = grid.compare_state(path)
            res["compare_state_file_s"] = round(time.perf_counter() - t0, 2)
            res["file_bytes"] = os.path.getsize(path)
        t0 = time.perf_counter()
        clean = clean.merge(grid.compare_state(grid))
        res["compare_state_grid_s"] = round(time.perf_counter() - t0, 2)
        res["clean"] = not clean.different
    print(json.dumps(res))


if __name__ == "__main__":
    main()
