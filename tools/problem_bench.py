#!/usr/bin/env python3
"""What a user-defined problem costs at the start of a run: armon_hip_init_test + armon_hip_init_regions (what
solver.init_test runs for a Problem) against armon_hip_init_test alone (what it runs for a built-in case), on the same block,
event-timed, launches interleaved, medians. Three problems: 1 region with 1 sample per cell and axis, 8 regions with 1, 8
regions with 4. Prints ONE JSON line. No bar: the kernels run once per run.

    python tools/problem_bench.py [--n 16384] [--dtype float64] [--launches 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import armon_amd  # noqa: E402
from armon_amd import Box, Disc, Ellipse, HalfPlane, Problem, State  # noqa: E402
from armon_amd.solver import BlockGrid, _init_test_kernel  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def regions(n):
    shapes = [HalfPlane((1, 1), 0.6), Disc((0.5, 0.5), r=0.3), Box(x=(0.1, 0.4), y=(0.55, 0.9)), Ellipse((0.7, 0.3), (0.2, 0.1)),
              HalfPlane((0.6, -0.8), -0.3), Box(x=(0.6, float("inf")), y=(0.6, 0.8)), Disc((0.2, 0.2), r=0.15), Ellipse((0.5, 0.8), (0.3, 0.05))]
    return [(s, State(1. + 0.25 * k, u=0.1 * k, p=1.)) for k, s in enumerate(shapes[:n])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    variants = {"1_region_1_sample": (1, 1), "8_regions_1_sample": (8, 1), "8_regions_4_samples": (8, 4)}
    common = dict(N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0)
    plain = armon_amd.ArmonParameters(test="Sod", **common)
    grid = BlockGrid(plain)
    dev = plain.device
    runs = {"init_test": plain}
    for name, (n, samples) in variants.items():
        runs[name] = armon_amd.ArmonParameters(test=Problem(name, State(1., p=1.), regions(n), samples=samples), ctx=dev.ctx, **common)
    times = {name: [] for name in runs}
    for k in range(a.warmup + a.launches):
        for name, params in runs.items():
            dev.event_record(20)
            _init_test_kernel(params, grid)
            dev.event_record(21)
            dev.wait()
            if k >= a.warmup:
                times[name].append(dev.event_elapsed_ms(20, 21))
    base = median(times["init_test"])
    res = {"tool": "problem_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "launches": a.launches, "warmup": a.warmup,
           "init_test_ms": round(base, 4), "init_test_ms_min": round(min(times["init_test"]), 4), "init_test_ms_max": round(max(times["init_test"]), 4)}
    for name in variants:
        t = median(times[name])
        res[name] = {"ms": round(t, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4),
                     "regions_only_ms": round(t - base, 4), "over_init_test": round(t / base, 4)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
