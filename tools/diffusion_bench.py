#!/usr/bin/env python3
"""What physical diffusion costs on the device: one step armon_hip_diffuse for the state alone (64 B per fp64
cell: rho, u, v, E read and written), for one plane alone (rho and the plane read, the plane written: 24 B) and for the state
with four planes (128 B), against armon_hip_stream_copy4 (4 read + 4 written: the same 64 B per cell) and the two state
sweeps armon_hip_sweep of the same block, in the same process, launches interleaved, event-timed, medians; and the cycle of
the benchmark's configuration (Sod, GAD + minmod + euler_2nd, Sequential, fused sweeps, tuned arithmetic) without and with
diffusion (nu = chi small enough for one sub-step per cycle), event-timed per cycle, each on a grid of its own. fp64 and
fp32. Prints ONE JSON line.

    python tools/diffusion_bench.py [--n 16384] [--launches 30] [--cycles 30] [--dtypes float64 float32]

Expectation from the bytes alone: a state step takes the time of copy4."""
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
from armon_amd.solver import STATE_VARS, BlockGrid, diffuse_desc, init_test, solver_cycle, sweep_desc  # noqa: E402


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


def parameters(n, dtype, kappa=0., names=()):
    return armon_amd.ArmonParameters(test="Sod", N=(n, n), scheme="GAD", riemann_limiter="minmod", projection="euler_2nd",
                                     axis_splitting="Sequential", nghost=4, maxtime=1e9, maxcycle=10 ** 9, silent=5, data_type=dtype,
                                     viscosity=kappa, heat_diffusivity=kappa,
                                     scalars=[armon_amd.Scalar(name, 0.25, [(armon_amd.Disc((0.5, 0.5), 0.3), 1.)], diffusivity=kappa)
                                              for name in names])


def bench(n, dtype, launches, warmup, cycles):
    res = {"N": [n, n]}
    kappa = 0.05 / n                                   # one sub-step per cycle at the CFL step of Sod: 4 kappa dt / dx² < 0.5
    for key, k in (("cycle_plain", 0.), ("cycle_diffusive", kappa)):
        params = parameters(n, dtype, k)
        grid = BlockGrid(params)
        init_test(params, grid)
        res["device"] = params.device.name
        stats(key, time_cycles(params, grid, cycles, 3), res)
        res[key + "_pair_cycles"] = grid.pair_cycles
        res[key + "_diffusion_steps"] = grid.diffusion_steps
        del grid
        gc.collect()
    res["cycle_diffusive_over_plain"] = round(res["cycle_diffusive_ms"] / res["cycle_plain_ms"], 4)
    # the steps alone, on a block with four diffusing planes
    params = parameters(n, dtype, kappa, ["a", "b", "c", "d"])
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    dt = 1e-3 * params.cell_size(0)
    descs = {"x": sweep_desc(params, grid, Axis.X, dt, params.cell_size(0)), "y": sweep_desc(params, grid, Axis.Y, dt, params.cell_size(1))}
    full = diffuse_desc(params, grid, dt)
    state = diffuse_desc(params, grid, dt)
    state.ns = 0
    plane = diffuse_desc(params, grid, dt)
    plane.ns, plane.nu, plane.chi = 1, 0., 0.
    plane.rho_out = plane.u_out = plane.v_out = plane.E_out = None     # what a dye-only run launches: no copy of rho
    sweep, diffuse = params.fn("sweep"), params.fn("diffuse")
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    names = ["sweep_x", "sweep_y", "diffuse_state", "diffuse_plane", "diffuse_state_4", "copy4"]
    times = {k: [] for k in names}
    for k in range(warmup + launches):
        dev.event_record(26)
        check(sweep(dev.ctx, C.byref(descs["x"])))
        dev.event_record(27)
        check(sweep(dev.ctx, C.byref(descs["y"])))
        dev.event_record(28)
        check(diffuse(dev.ctx, C.byref(state)))
        dev.event_record(29)
        check(diffuse(dev.ctx, C.byref(plane)))
        dev.event_record(30)
        check(diffuse(dev.ctx, C.byref(full)))
        dev.event_record(31)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(32)
        dev.event_sync(32)
        if k >= warmup:
            for i, name in enumerate(names):
                times[name].append(dev.event_elapsed_ms(26 + i, 27 + i))
    for name, t in times.items():
        stats(name, t, res)
    item = np.dtype(dtype).itemsize
    cells = n * n
    res["copy4_GBps"] = round(8 * nb / res["copy4_ms"] / 1e6, 1)
    for key, words in (("sweep_x", 8), ("sweep_y", 8), ("diffuse_state", 8), ("diffuse_plane", 3), ("diffuse_state_4", 16)):
        res[key + "_GBps"] = round(words * cells * item / res[key + "_ms"] / 1e6, 1)
    for key in ("diffuse_state", "diffuse_plane", "diffuse_state_4"):
        res[key + "_over_copy4"] = round(res[key + "_ms"] / res["copy4_ms"], 4)
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
    out = {"tool": "diffusion_bench", "launches": a.launches, "warmup": a.warmup, "cycles": a.cycles}
    for dtype in a.dtypes:
        res = bench(a.n, dtype, a.launches, a.warmup, a.cycles)
        out["device"] = res.pop("device")
        out[dtype] = res
        gc.collect()                        # the block's vectors go before the next precision allocates its own
    print(json.dumps(out))


if __name__ == "__main__":
    main()
