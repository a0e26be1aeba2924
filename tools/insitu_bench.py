#!/usr/bin/env python3
"""What a reduced-output frame costs on the device: armon_hip_coarsen (5 vectors read, (fx fy) times fewer written) against
armon_hip_stream_copy4 (4 read + 4 written: the same-device yardstick of DESIGN.md) on the same vectors in the same
process, launches interleaved, event-timed, medians; and, once, what a frame cost before — BlockGrid.device_to_host of the
six saved vectors (host clock around synchronous copies). Prints ONE JSON line.

    python tools/insitu_bench.py [--n 16384] [--factor 16 16] [--dtype float64] [--launches 30] [--no-d2h]

Acceptance of the feature: coarsen_ms <= copy4_ms (the coarsening moves 5/8 of the copy's bytes)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd._lib import check  # noqa: E402
from armon_amd.parameters import coarse_shape  # noqa: E402
from armon_amd.solver import SAVED_VARS, STATE_VARS, BlockGrid, init_test  # noqa: E402


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--factor", type=int, nargs=2, default=(16, 16))
    ap.add_argument("--dtype", default="float64")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-d2h", action="store_true", help="skip the one timing of the six whole-field copies to the host")
    a = ap.parse_args()
    assert a.launches >= 20
    params = armon_amd.ArmonParameters(test="Sod", N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0)
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    fx, fy = a.factor
    cnx, cny = coarse_shape(params.N, (fx, fy))
    out = dev.empty(5 * cnx * cny, params.data_type)
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    g, pitch = params.nghost, params.N[0] + 2 * params.nghost
    coarsen = params.fn("coarsen")
    state = [grid.ptr(f) for f in STATE_VARS]
    t_coarsen, t_copy = [], []
    for k in range(a.warmup + a.launches):
        dev.event_record(20)
        check(coarsen(dev.ctx, pitch, g, a.n, a.n, fx, fy, *state, grid.ptr("p"), C.c_void_p(out.ptr)))
        dev.event_record(21)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(22)
        if k >= a.warmup:
            t_coarsen.append(dev.event_elapsed_ms(20, 21))
            t_copy.append(dev.event_elapsed_ms(21, 22))
    item = np.dtype(params.data_type).itemsize
    coarsen_ms, copy4_ms = median(t_coarsen), median(t_copy)
    read_bytes = 5 * a.n * a.n * item                       # real cells of rho, u, v, E, p
    res = {"tool": "insitu_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "factor": [fx, fy], "with_p": True,
           "launches": a.launches, "warmup": a.warmup,
           "coarsen_ms": round(coarsen_ms, 4), "coarsen_ms_min": round(min(t_coarsen), 4), "coarsen_ms_max": round(max(t_coarsen), 4),
           "copy4_ms": round(copy4_ms, 4), "copy4_ms_min": round(min(t_copy), 4), "copy4_ms_max": round(max(t_copy), 4),
           "coarsen_over_copy4": round(coarsen_ms / copy4_ms, 4),
           "coarsen_read_GBps": round(read_bytes / coarsen_ms / 1e6, 1), "copy4_GBps": round(8 * nb / copy4_ms / 1e6, 1),
           "coarse_bytes_to_host": 5 * cnx * cny * item, "accepted": bool(coarsen_ms <= copy4_ms)}
    if not a.no_d2h:
        dev.wait()
        t0 = time.perf_counter()
        host = grid.device_to_host(SAVED_VARS)
        res["d2h_six_fields_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["d2h_bytes"] = int(sum(v.nbytes for v in host.values()))
        del host
        t0 = time.perf_counter()
        planes = grid.coarsen((fx, fy))
        res["coarsen_to_host_ms"] = round((time.perf_counter() - t0) * 1e3, 2)       # kernel + copies of the coarse planes + x, y
        del planes
    out.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
