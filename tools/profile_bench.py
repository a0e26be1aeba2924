#!/usr/bin/env python3
"""What an in-situ profile costs on the device: the main pass of armon_hip_profile over a Sedov state a few cycles in, for
X (width 16 and width 1: every column its own bin), Y (width 16), R (dr = 4 dx) and R (dr = dx), and the bounds pass, against armon_hip_stream_copy4 on the same four
vectors in the same process — launches interleaved, event-timed, medians. The pass reads 32 B per fp64 cell where the copy
moves 64. Prints ONE JSON line.

    python tools/profile_bench.py [--n 16384] [--dtype float64] [--launches 30] [--cycles 3]

Yardstick: the copy and its own spread, (max - min) / median over its repeats in this process."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import profile as prof  # noqa: E402
from armon_amd._lib import check  # noqa: E402
from armon_amd.solver import STATE_VARS  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=3)
    a = ap.parse_args()
    params = armon_amd.ArmonParameters(test="Sedov", N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0, maxcycle=a.cycles,
                                       return_data=True)
    grid = armon_amd.armon(params).data
    dev = params.device
    tile, window = (params, grid), (0, 0, a.n, a.n)
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    dx = float(params.cell_size(0))
    cases = {"x_w16": ("x", dict(width=16)), "x_w1": ("x", dict(width=1)), "y_w16": ("y", dict(width=16)), "r_dr4": ("r", dict(dr=4 * dx)), "r_dr1": ("r", dict(dr=dx))}
    item = np.dtype(params.data_type).itemsize
    res = {"tool": "profile_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "cycles": a.cycles, "launches": a.launches,
           "warmup": a.warmup}
    t_copy_all = []

    def timed(launch):
        t_pass, t_copy = [], []
        for k in range(a.warmup + a.launches):
            dev.event_record(20)
            launch()
            dev.event_record(21)
            dev.stream_copy4(src, dst, nb)
            dev.event_record(22)
            dev.wait()
            if k >= a.warmup:
                t_pass.append(dev.event_elapsed_ms(20, 21))
                t_copy.append(dev.event_elapsed_ms(21, 22))
        t_copy_all.extend(t_copy)
        return t_pass

    def report(name, t):
        res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = round(median(t), 4), round(min(t), 4), round(max(t), 4)
        res[name + "_GBps"] = round(4 * a.n * a.n * item / median(t) / 1e6, 1)

    for name, (kind, kw) in cases.items():
        spec = prof.make_spec(params, kind, **kw)
        scale = prof.default_scale(prof.state_bounds([tile], spec))
        c_spec = prof._c_spec(spec, scale)
        bins = dev.empty(spec[2] * prof.WORDS, np.uint64)
        check(dev._L.armon_hip_profile_reset(dev.ctx, spec[2], C.c_void_p(bins.ptr)))
        report(name, timed(lambda: prof._call("profile", params, grid, window, c_spec, bins)))
        res[name + "_bins"] = spec[2]
        dev.wait()
        raw = bins.to_host().reshape(spec[2], prof.WORDS)
        runs = a.warmup + a.launches                       # every launch merged the same cells into the same bins
        assert int(raw[:, prof.W_N].sum()) == runs * a.n * a.n and not raw[:, prof.W_BAD].any(), name
        bins.free()
    spec = prof.make_spec(params, "r", dr=dx)
    c_spec, bounds = prof._c_spec(spec, (0,) * 5), dev.zeros(5, np.uint64)
    report("bounds_r", timed(lambda: prof._call("profile_bounds", params, grid, window, c_spec, bounds)))
    bounds.free()
    copy4_ms = median(t_copy_all)
    spread = (max(t_copy_all) - min(t_copy_all)) / copy4_ms
    res.update({"copy4_ms": round(copy4_ms, 4), "copy4_ms_min": round(min(t_copy_all), 4), "copy4_ms_max": round(max(t_copy_all), 4),
                "copy4_spread": round(spread, 4), "copy4_GBps": round(8 * nb / copy4_ms / 1e6, 1)})
    for name in list(cases) + ["bounds_r"]:
        res[name + "_over_copy4"] = round(res[name + "_ms"] / copy4_ms, 4)
        res[name + "_under_copy4"] = bool(res[name + "_ms"] <= copy4_ms * (1 + spread))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
