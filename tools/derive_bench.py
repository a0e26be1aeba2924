#!/usr/bin/env python3
"""What a derived-field frame costs on the device: armon_hip_derive for grad_rho alone (max) and for all eight quantities
(mean) against armon_hip_coarsen (4 vectors read, no p) and armon_hip_stream_copy4 (4 read + 4 written: the same-device
yardstick of DESIGN.md) on the same vectors in the same process, launches interleaved, event-timed, medians. The state is a
few cycles into the test case, so that the arithmetic sees values, not zeros. Prints ONE JSON line.

    python tools/derive_bench.py [--n 16384] [--factor 16 16] [--dtype float64] [--launches 30] [--test Sedov] [--cycles 2]

No bar is fixed in advance: the algorithmic traffic is 32 B per fp64 cell plus the two rows around each chunk of 64 rows,
what coarsen reads without p; the ratios to coarsen and to the copy are what DESIGN.md §4.9 reports."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import derived  # noqa: E402
from armon_amd._lib import check  # noqa: E402
from armon_amd.parameters import coarse_shape  # noqa: E402
from armon_amd.solver import STATE_VARS  # noqa: E402


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
    ap.add_argument("--test", default="Sedov")
    ap.add_argument("--cycles", type=int, default=2)
    a = ap.parse_args()
    assert a.launches >= 20
    params = armon_amd.ArmonParameters(test=a.test, N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0,
                                       maxcycle=a.cycles, return_data=True)
    grid = armon_amd.armon(params).data
    dev = params.device
    fx, fy = a.factor
    cnx, cny = coarse_shape(params.N, (fx, fy))
    out = dev.empty(8 * cnx * cny, params.data_type)
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    g, pitch = params.nghost, params.N[0] + 2 * params.nghost
    coarsen, derive = params.fn("coarsen"), params.fn("derive")
    state = [grid.ptr(f) for f in STATE_VARS]
    one = derived._c_spec(params, ("grad_rho",), ("max",), 0)
    every = derived._c_spec(params, derived.QUANTITIES, ("mean",) * 8, 0)
    times = {"grad_rho": [], "all8": [], "coarsen": [], "copy4": []}
    for k in range(a.warmup + a.launches):
        dev.event_record(20)
        check(derive(dev.ctx, pitch, g, a.n, a.n, fx, fy, *state, C.byref(one), C.c_void_p(out.ptr)))
        dev.event_record(21)
        check(derive(dev.ctx, pitch, g, a.n, a.n, fx, fy, *state, C.byref(every), C.c_void_p(out.ptr)))
        dev.event_record(22)
        check(coarsen(dev.ctx, pitch, g, a.n, a.n, fx, fy, *state, None, C.c_void_p(out.ptr)))
        dev.event_record(23)
        dev.stream_copy4(src, dst, nb)
        dev.event_record(24)
        if k >= a.warmup:
            for slot, name in enumerate(("grad_rho", "all8", "coarsen", "copy4")):
                times[name].append(dev.event_elapsed_ms(20 + slot, 21 + slot))
    item = np.dtype(params.data_type).itemsize
    ms = {name: median(v) for name, v in times.items()}
    read_bytes = 4 * a.n * a.n * item                       # real cells of rho, u, v, E (grad_rho alone reads no E: 3/4 of it)
    res = {"tool": "derive_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "factor": [fx, fy], "test": a.test,
           "cycles": a.cycles, "launches": a.launches, "warmup": a.warmup}
    for name, v in times.items():
        res[name + "_ms"], res[name + "_ms_min"], res[name + "_ms_max"] = round(ms[name], 4), round(min(v), 4), round(max(v), 4)
    res.update({"grad_rho_over_coarsen": round(ms["grad_rho"] / ms["coarsen"], 4), "all8_over_coarsen": round(ms["all8"] / ms["coarsen"], 4),
                "grad_rho_over_copy4": round(ms["grad_rho"] / ms["copy4"], 4), "all8_over_copy4": round(ms["all8"] / ms["copy4"], 4),
                "grad_rho_read_GBps": round(0.75 * read_bytes / ms["grad_rho"] / 1e6, 1), "all8_read_GBps": round(read_bytes / ms["all8"] / 1e6, 1),
                "coarsen_read_GBps": round(read_bytes / ms["coarsen"] / 1e6, 1), "copy4_GBps": round(8 * nb / ms["copy4"] / 1e6, 1),
                "bytes_per_cell": 4 * item, "plane_bytes_to_host": cnx * cny * item})
    out.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
