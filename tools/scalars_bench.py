#!/usr/bin/env python3
"""What passive scalars cost on the device: the X and the Y scalar sweep armon_hip_sweep_scalars with ns = 1 and
ns = 4 planes ((32 + 16 ns) B per fp64 cell) against the state sweeps armon_hip_sweep of the same descriptors (64 B per cell)
and armon_hip_stream_copy4 (4 read + 4 written: the same-device yardstick of DESIGN.md) on the same block in the same
process, launches interleaved, event-timed, medians; and the cycle of the benchmark's configuration (Sod, GAD + minmod +
euler_2nd, Sequential, fused sweeps, tuned arithmetic) with 0, 1 and 4 scalars, event-timed per cycle — the cycle without
scalars on a grid of its own (it takes armon_hip_sweep_pair where that applies; a run with scalars takes the two single
sweeps). fp64 and fp32. Prints ONE JSON line.

    python tools/scalars_bench.py [--n 16384] [--launches 30] [--cycles 30] [--dtypes float64 float32]

Expectation from the bytes alone: a scalar sweep takes (32 + 16 ns) / 64 of its state sweep; a cycle with one scalar about
1.75 x the plain one."""
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
from armon_amd.solver import SCALAR_SWEEPS, STATE_VARS, BlockGrid, init_test, solver_cycle, sweep_desc  # noqa: E402


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


def parameters(n, dtype, names):
    return armon_amd.ArmonParameters(test="Sod", N=(n, n), scheme="GAD", riemann_limiter="minmod", projection="euler_2nd",
                                     axis_splitting="Sequential", nghost=4, maxtime=1e9, maxcycle=10 ** 9, silent=5, data_type=dtype,
                                     scalars=[armon_amd.Scalar(name, 0.25, [(armon_amd.Disc((0.5, 0.5), 0.3), 1.)]) for name in names])


def bench(n, dtype, launches, warmup, cycles, transports=("remap",)):
    res = {"N": [n, n]}
    # the plain cycle, on a grid without scalars
    params = parameters(n, dtype, [])
    grid = BlockGrid(params)
    init_test(params, grid)
    res["device"] = params.device.name
    stats("cycle_0", time_cycles(params, grid, cycles, 3), res)
    res["cycle_0_pair_cycles"] = grid.pair_cycles
    del grid
    gc.collect()
    # the cycles with 1 and 4 scalars, on one grid: the same placement of its vectors
    params = parameters(n, dtype, ["a", "b", "c", "d"])
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    all_planes = grid.scalar_planes
    for transport in transports:
        params.scalar_transport = transport                # (solver.scalar_sweep reads it launch by launch)
        sub = res if len(transports) == 1 else res.setdefault(transport, {})
        for ns in (1, 4, 1):
            grid.scalar_planes = all_planes[:ns]
            stats(f"cycle_{ns}" if f"cycle_{ns}_ms" not in sub else f"cycle_{ns}_again", time_cycles(params, grid, cycles, 3), sub)
        grid.scalar_planes = all_planes
        for ns in (1, 4):
            sub[f"cycle_{ns}_over_cycle_0"] = round(sub[f"cycle_{ns}_ms"] / res["cycle_0_ms"], 4)
        # the sweeps alone: state X, scalars X (1, 4), state Y, scalars Y (1, 4), the copy
        init_test(params, grid, tune=False)
        dt = 1e-3 * params.cell_size(0)
        descs = {"x": sweep_desc(params, grid, Axis.X, dt, params.cell_size(0)), "y": sweep_desc(params, grid, Axis.Y, dt, params.cell_size(1))}
        sweep, scalars = params.fn("sweep"), params.fn(SCALAR_SWEEPS[transport])
        phi_in = (C.c_void_p * 4)(*[grid.data[f].ptr for f in all_planes])
        phi_out = (C.c_void_p * 4)(*[grid.alt[f].ptr for f in all_planes])
        src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
        nb = src[0].nbytes & ~15
        names = ["sweep_x", "scalars_x_1", "scalars_x_4", "sweep_y", "scalars_y_1", "scalars_y_4", "copy4"]
        times = {k: [] for k in names}
        for k in range(warmup + launches):
            slot = 26
            dev.event_record(slot)
            for axis in "xy":
                check(sweep(dev.ctx, C.byref(descs[axis])))
                dev.event_record(slot + 1)
                check(scalars(dev.ctx, C.byref(descs[axis]), 1, phi_in, phi_out))
                dev.event_record(slot + 2)
                check(scalars(dev.ctx, C.byref(descs[axis]), 4, phi_in, phi_out))
                dev.event_record(slot + 3)
                slot += 3
            dev.stream_copy4(src, dst, nb)
            dev.event_record(slot + 1)
            dev.event_sync(slot + 1)
            if k >= warmup:
                for i, name in enumerate(names):
                    times[name].append(dev.event_elapsed_ms(26 + i, 27 + i))
        for name, t in times.items():
            stats(name, t, sub)
        item = np.dtype(dtype).itemsize
        cells = n * n
        sub["copy4_GBps"] = round(8 * nb / sub["copy4_ms"] / 1e6, 1)
        for axis in "xy":
            sub[f"sweep_{axis}_GBps"] = round(8 * cells * item / sub[f"sweep_{axis}_ms"] / 1e6, 1)
            for ns in (1, 4):
                key = f"scalars_{axis}_{ns}"
                sub[key + "_GBps"] = round((4 + 2 * ns) * cells * item / sub[key + "_ms"] / 1e6, 1)
                sub[key + "_over_sweep"] = round(sub[key + "_ms"] / sub[f"sweep_{axis}_ms"], 4)
                sub[key + "_bytes_over_sweep"] = round((4 + 2 * ns) / 8, 4)
    dev.wait()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--transport", nargs="+", choices=sorted(SCALAR_SWEEPS), default=["remap"])
    a = ap.parse_args()
    out = {"tool": "scalars_bench", "launches": a.launches, "warmup": a.warmup, "cycles": a.cycles, "transport": a.transport}
    for dtype in a.dtypes:
        res = bench(a.n, dtype, a.launches, a.warmup, a.cycles, a.transport)
        out["device"] = res.pop("device")
        out[dtype] = res
        gc.collect()                        # the block's vectors go before the next precision allocates its own
    print(json.dumps(out))


if __name__ == "__main__":
    main()
