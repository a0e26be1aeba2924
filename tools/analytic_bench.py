#!/usr/bin/env python3
"""What the error norms cost on the device: armon_hip_exact_norms over a Sedov state a few cycles in, for a Riemann problem
along x (1 sample), the point-blast table along r (1 sample, and 2 x 2 samples per cell) and armon_hip_exact_fill of the table,
next to the profile's X pass (width 16) as the comparison point, against armon_hip_stream_copy4 on the same four vectors in
the same process — launches interleaved, event-timed, medians. The pass reads 32 B per fp64 cell where the copy moves 64.
Prints ONE JSON line.

    python tools/analytic_bench.py [--n 16384] [--dtype float64] [--launches 30] [--cycles 3]

Yardstick: the copy and its own spread, (max - min) / median over its repeats in this process."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import analytic as an  # noqa: E402
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
    ap.add_argument("--time", type=float, default=0.5, help="the time of the exact solutions: the blast then covers 40 % of the cells")
    a = ap.parse_args()
    params = armon_amd.ArmonParameters(test="Sedov", N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0, maxcycle=a.cycles,
                                       return_data=True)
    grid = armon_amd.armon(params).data
    dev = params.device
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    item = np.dtype(params.data_type).itemsize
    res = {"tool": "analytic_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "cycles": a.cycles, "launches": a.launches,
           "warmup": a.warmup, "time": a.time}
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

    blast = an.reference_for(params, a.time)
    sod = an.ExactSolution(an.RIEMANN, "x", (0.0, 0.0), 1.4, time=0.5, riemann=an.riemann_exact((1.0, 0.0, 1.0), (0.125, 0.0, 0.1), 1.4))
    table = dev.from_host(np.ascontiguousarray(blast.values).ravel())
    out = dev.empty(4 * an.WORDS, np.uint64)
    geometry = [dev.ctx, grid.size.size[0], grid.size.ghosts, a.n, a.n, *[C.c_void_p(grid.data[f].ptr) for f in ("rho", "u", "v", "E")],
                0, 0, a.n, a.n, 0, 0]
    cases = {"riemann_x_s1": (sod, 1), "table_r_s1": (blast, 1), "table_r_s2": (blast, 2)}
    for name, (solution, samples) in cases.items():
        c_spec = an._c_spec(an.spec_of(params, solution, samples), table.ptr)
        check(dev._L.armon_hip_exact_norms_reset(dev.ctx, C.c_void_p(out.ptr)))
        report(name, timed(lambda: check(params.fn("exact_norms")(*geometry, C.byref(c_spec), C.c_void_p(out.ptr)))))
        dev.wait()
        raw = out.to_host().reshape(4, an.WORDS)
        runs = a.warmup + a.launches                       # every launch merged the same cells into the same records
        # (the few cells that still hold the blast's energy are past the p quanta of a solution at a later time: they count as bad)
        assert int(raw[0, an.W_N]) + int(raw[0, an.W_BAD]) == runs * a.n * a.n and int(raw[0, an.W_BAD]) <= runs * 64, name
        res[name + "_n_bad"] = int(raw[0, an.W_BAD]) // runs
    # the profile's X pass of the same session: the comparison point
    spec = prof.make_spec(params, "x", width=16)
    p_spec = prof._c_spec(spec, prof.default_scale(prof.state_bounds([(params, grid)], spec)))
    bins = dev.empty(spec[2] * prof.WORDS, np.uint64)
    check(dev._L.armon_hip_profile_reset(dev.ctx, spec[2], C.c_void_p(bins.ptr)))
    report("profile_x_w16", timed(lambda: prof._call("profile", params, grid, (0, 0, a.n, a.n), p_spec, bins)))
    bins.free()
    # the fill last: it overwrites the state
    c_spec = an._c_spec(an.spec_of(params, blast, 1), table.ptr)
    report("fill_table_r_s1", timed(lambda: check(params.fn("exact_fill")(*geometry, C.byref(c_spec)))))
    check(dev._L.armon_hip_exact_norms_reset(dev.ctx, C.c_void_p(out.ptr)))
    check(params.fn("exact_norms")(*geometry, C.byref(c_spec), C.c_void_p(out.ptr)))
    dev.wait()
    assert not out.to_host().reshape(4, an.WORDS)[:, 2:12].any()      # the filled state is at distance 0
    out.free()
    table.free()
    copy4_ms = median(t_copy_all)
    spread = (max(t_copy_all) - min(t_copy_all)) / copy4_ms
    res.update({"copy4_ms": round(copy4_ms, 4), "copy4_ms_min": round(min(t_copy_all), 4), "copy4_ms_max": round(max(t_copy_all), 4),
                "copy4_spread": round(spread, 4), "copy4_GBps": round(8 * nb / copy4_ms / 1e6, 1)})
    for name in list(cases) + ["profile_x_w16", "fill_table_r_s1"]:
        res[name + "_over_copy4"] = round(res[name + "_ms"] / copy4_ms, 4)
        res[name + "_over_profile_x"] = round(res[name + "_ms"] / res["profile_x_w16_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
