#!/usr/bin/env python3
"""What a body force costs on the device: the kick armon_hip_body_force for gx only, gy only and both
(2 + 2, 2 + 2 and 3 + 3 planes read + written) against armon_hip_stream_copy4 (4 read + 4 written: the same-device yardstick
of DESIGN.md) on the same block in the same process, launches interleaved, event-timed, medians; and the cycle of the
benchmark's configuration (Sod, GAD + minmod + euler_2nd, Sequential, fused sweeps) with and without gravity = (0, -1), on the
same grid — the same placement of its vectors —, event-timed per cycle. fp64 and fp32. Prints ONE JSON line.

    python tools/body_force_bench.py [--n 16384] [--launches 30] [--cycles 30] [--dtypes float64 float32]

Expectation from the bytes alone: a one-component kick moves half of what the copy moves and should take about half its
time; a cycle with it about a quarter longer than its two 64 B / cell sweeps alone."""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd._lib import check  # noqa: E402
from armon_amd.blocking import Axis  # noqa: E402
from armon_amd.solver import STATE_VARS, BlockGrid, init_test, solver_cycle  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(name, v, res):
    res[name + "_ms"] = round(median(v), 4)
    res[name + "_ms_min"] = round(min(v), 4)
    res[name + "_ms_max"] = round(max(v), 4)


def time_cycles(params, grid, cycles, warmup):
    """Event-timed ms of each of ``cycles`` cycles from the initial state (after ``warmup`` untimed ones)."""
    dev, gdt = params.device, grid.global_dt
    init_test(params, grid, tune=False)
    gdt.reset()
    grid.dt_inflight.clear()
    ms = []
    for k in range(warmup + cycles):
        dev.event_record(24)
        solver_cycle(params, grid, last_cycle=False)
        dev.event_record(25)
        gdt.next_cycle()
        dev.event_sync(25)
        if k >= warmup:
            ms.append(dev.event_elapsed_ms(24, 25))
    params.wait()
    return ms


def bench(n, dtype, launches, warmup, cycles):
    params = armon_amd.ArmonParameters(test="Sod", N=(n, n), scheme="GAD", riemann_limiter="minmod", projection="euler_2nd",
                                       axis_splitting="Sequential", nghost=4, maxtime=1e9, maxcycle=10 ** 9, silent=5,
                                       data_type=dtype, gravity=(0., -1.))
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    res = {"device": dev.name, "N": [n, n], "placement": None if grid.placement is None else grid.placement.get("chosen_ms")}
    # the cycle, without and with the force, on the same grid
    for name, forced in (("cycle", False), ("cycle_forced", True), ("cycle_again", False)):
        params.forced = forced
        stats(name, time_cycles(params, grid, cycles, 3), res)
    params.forced = True
    res["forced_over_unforced"] = round(res["cycle_forced_ms"] / min(res["cycle_ms"], res["cycle_again_ms"]), 4)
    # the kick alone, against the copy
    r = params.block_size.domain_range(*params.steps_ranges[Axis.X].real_domain).to_c()
    kick = params.fn("body_force")
    u, v, E = (grid.ptr(f) for f in ("u", "v", "E"))
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    dt = 1e-6
    forms = {"kick_x": (1., 0.), "kick_y": (0., -1.), "kick_xy": (1., -1.)}
    times = {k: [] for k in list(forms) + ["copy4"]}
    for k in range(warmup + launches):
        slot = 26
        dev.event_record(slot)
        for name, (gx, gy) in forms.items():
            check(kick(dev.ctx, r, dt, gx, gy, u, v, E))
            slot += 1
            dev.event_record(slot)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(slot + 1)
        dev.event_sync(slot + 1)
        if k >= warmup:
            for i, name in enumerate(times):
                times[name].append(dev.event_elapsed_ms(26 + i, 27 + i))
    for name, t in times.items():
        stats(name, t, res)
    item = np.dtype(dtype).itemsize
    cells = n * n
    for name, planes in (("kick_x", 4), ("kick_y", 4), ("kick_xy", 6)):
        res[name + "_GBps"] = round(planes * cells * item / res[name + "_ms"] / 1e6, 1)
        res[name + "_over_copy4"] = round(res[name + "_ms"] / res["copy4_ms"], 4)
    res["copy4_GBps"] = round(8 * nb / res["copy4_ms"] / 1e6, 1)
    dev.wait()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    a = ap.parse_args()
    out = {"tool": "body_force_bench", "launches": a.launches, "warmup": a.warmup, "cycles": a.cycles}
    for dtype in a.dtypes:
        res = bench(a.n, dtype, a.launches, a.warmup, a.cycles)
        out["device"] = res.pop("device")
        out[dtype] = res
        gc.collect()                        # the block's vectors go before the next precision allocates its own
    print(json.dumps(out))


if __name__ == "__main__":
    main()
