#!/usr/bin/env python3
"""What periodic sides cost on a lone block: the X wrap and the Y wrap alone (armon_hip_periodic_ghosts, 4
vectors, all nghost = 4 layers), event-timed; and the cycle of the benchmark's configuration (Sod, GAD + minmod + euler_2nd,
Sequential, fused sweeps) with walls, with periodic = (True, False), (False, True), (True, True), and with walls again, on the
same grid — the same placement of its vectors —, event-timed per cycle. fp64 and fp32, medians of 30 after 3. Prints ONE JSON
line.

    python tools/periodic_bench.py [--n 16384] [--launches 30] [--cycles 30] [--dtypes float64 float32]

Expectation from the bytes alone: the Y wrap moves 2 x 4 x 4 rows of n cells (8 MB at 16384², fp64), the X wrap touches about
2 x n partly-used lines per vector, against 17 GB per sweep: what a periodic axis adds to a cycle is launch latency, and for
periodic Y the pair path's non-temporal march that the two single sweeps do not have (fp64; about 2 % of the Y sweep)."""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import armon_amd  # noqa: E402
from armon_amd.blocking import Axis  # noqa: E402
from armon_amd.solver import STATE_VARS, BlockGrid, init_test, pair_cycle, periodic_ghosts, solver_cycle  # noqa: E402


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
                                       data_type=dtype)
    grid = BlockGrid(params)            # built with walls: its vectors hold the pair's intermediate where the pair is usable
    init_test(params, grid)
    dev = params.device
    res = {"device": dev.name, "N": [n, n], "placement": None if grid.placement is None else grid.placement.get("chosen_ms")}
    # the cycle under each set of sides, on the same grid and placement (the block's own axes are flipped in place)
    for name, wrap in (("cycle_walls", (False, False)), ("cycle_periodic_x", (True, False)), ("cycle_periodic_y", (False, True)),
                       ("cycle_periodic_xy", (True, True)), ("cycle_walls_again", (False, False))):
        params.periodic = params.wrap = wrap
        res[name + "_pair"] = bool(pair_cycle(params, grid))
        stats(name, time_cycles(params, grid, cycles, warmup), res)
    params.periodic = params.wrap = (False, False)
    walls = min(res["cycle_walls_ms"], res["cycle_walls_again_ms"])
    for name in ("cycle_periodic_x", "cycle_periodic_y", "cycle_periodic_xy"):
        res[name + "_over_walls"] = round(res[name + "_ms"] / walls, 4)
    # the wraps alone
    times = {"wrap_x": [], "wrap_y": []}
    for k in range(warmup + launches):
        dev.event_record(26)
        periodic_ghosts(params, grid, Axis.X, STATE_VARS)
        dev.event_record(27)
        periodic_ghosts(params, grid, Axis.Y, STATE_VARS)
        dev.event_record(28)
        dev.event_sync(28)
        if k >= warmup:
            times["wrap_x"].append(dev.event_elapsed_ms(26, 27))
            times["wrap_y"].append(dev.event_elapsed_ms(27, 28))
    for name, t in times.items():
        stats(name, t, res)
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
    out = {"tool": "periodic_bench", "launches": a.launches, "warmup": a.warmup, "cycles": a.cycles}
    for dtype in a.dtypes:
        res = bench(a.n, dtype, a.launches, a.warmup, a.cycles)
        out["device"] = res.pop("device")
        out[dtype] = res
        gc.collect()                        # the block's vectors go before the next precision allocates its own
    print(json.dumps(out))


if __name__ == "__main__":
    main()
