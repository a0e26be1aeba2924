#!/usr/bin/env python3
"""What a sample of the run history costs on the device: armon_hip_history_sample (the pass and its fold) over a Sedov state
a few cycles in, against armon_hip_stream_copy4 on the same four vectors and against the X profile of width N (one bin: the
nearest thing the profiles offer) in the same process — launches interleaved, event-timed, medians. The sample reads 32 B
per fp64 cell where the copy moves 64. Then, unless ``--run-n 0``: a Sod run of ``--run-cycles`` cycles at ``--run-n`` squared
with ``history_step=1`` and with the history off, several times each in turn; the difference per cycle should be the sample
and no more (a larger one means a hidden synchronisation). Prints ONE JSON line.

    python tools/history_bench.py [--n 16384] [--dtype float64] [--launches 30] [--cycles 3] [--run-n 4096] [--run-cycles 100]

Yardstick: the copy and its own spread, (max - min) / median over its repeats in this process."""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import history as hist  # noqa: E402
from armon_amd import profile as prof  # noqa: E402
from armon_amd._lib import check  # noqa: E402
from armon_amd.solver import STATE_VARS  # noqa: E402

import ctypes as C  # noqa: E402


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
    ap.add_argument("--gauges", type=int, default=8)
    ap.add_argument("--run-n", type=int, default=4096)
    ap.add_argument("--run-cycles", type=int, default=100)
    ap.add_argument("--run-repeats", type=int, default=3)
    a = ap.parse_args()
    params = armon_amd.ArmonParameters(test="Sedov", N=(a.n, a.n), data_type=a.dtype, silent=5, placement_tries=0, maxcycle=a.cycles,
                                       return_data=True)
    grid = armon_amd.armon(params).data
    dev = params.device
    tile, window = (params, grid), (0, 0, a.n, a.n)
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    item = np.dtype(params.data_type).itemsize
    res = {"tool": "history_bench", "device": dev.name, "N": [a.n, a.n], "dtype": a.dtype, "cycles": a.cycles, "launches": a.launches,
           "warmup": a.warmup, "gauges": a.gauges}
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

    # the sample, with the default scale of this state and a few gauges along the diagonal
    rng = np.random.default_rng(1)
    points = [(float(params.origin[0] + f * params.domain_size[0]), float(params.origin[1] + f * params.domain_size[1]))
              for f in rng.uniform(0, 1, a.gauges)]
    first, _ = hist.sample_state([tile], gauges=points)
    sampler = hist.Sampler([tile], capacity=4, gauges=points, scale_exp=first.scale_exp)
    slot = [0]

    def sample():
        sampler.enqueue(slot[0] % 4)
        slot[0] += 1
    report("sample", timed(sample))
    raw, _ = sampler.read(0, 4)
    assert all(np.array_equal(raw[k], first.raw) for k in range(4)), "the timed samples are not the first one"
    sampler.close()
    res["sample_n_bad"] = first.n_bad
    # the parent's nearest: one bin of five sums along x
    spec = prof.make_spec(params, "x", width=a.n)
    scale = prof.default_scale(prof.state_bounds([tile], spec))
    c_spec = prof._c_spec(spec, scale)
    bins = dev.empty(spec[2] * prof.WORDS, np.uint64)
    check(dev._L.armon_hip_profile_reset(dev.ctx, spec[2], C.c_void_p(bins.ptr)))
    report("profile_x_one_bin", timed(lambda: prof._call("profile", params, grid, window, c_spec, bins)))
    bins.free()
    copy4_ms = median(t_copy_all)
    spread = (max(t_copy_all) - min(t_copy_all)) / copy4_ms
    res.update({"copy4_ms": round(copy4_ms, 4), "copy4_ms_min": round(min(t_copy_all), 4), "copy4_ms_max": round(max(t_copy_all), 4),
                "copy4_spread": round(spread, 4), "copy4_GBps": round(8 * nb / copy4_ms / 1e6, 1)})
    for name in ("sample", "profile_x_one_bin"):
        res[name + "_over_copy4"] = round(res[name + "_ms"] / copy4_ms, 4)
    del grid, src, dst
    # a whole run with a row per cycle against the same run with none: what the missing wait buys
    if a.run_n > 0:
        times = {"off": [], "on": []}
        with tempfile.TemporaryDirectory() as tmp:
            for _ in range(a.run_repeats + 1):                  # (the first pair warms up and is dropped)
                for mode in ("off", "on"):
                    opts = dict(history_step=1, history_capacity=256, output_dir=tmp) if mode == "on" else {}
                    p = armon_amd.ArmonParameters(test="Sod", N=(a.run_n, a.run_n), data_type=a.dtype, silent=5, maxcycle=a.run_cycles,
                                                  placement_tries=0, **opts)
                    stats = armon_amd.armon(p)
                    times[mode].append(stats.solve_time / stats.cycles * 1e3)
                    rows = None if stats.history is None else len(stats.history)
            assert rows == a.run_cycles + 1
        off, on = median(times["off"][1:]), median(times["on"][1:])
        res.update({"run_N": [a.run_n, a.run_n], "run_cycles": a.run_cycles, "run_repeats": a.run_repeats,
                    "sample_ms_scaled_to_run": round(res["sample_ms"] * (a.run_n / a.n) ** 2, 4),
                    "cycle_ms_history_off": round(off, 4), "cycle_ms_history_on": round(on, 4), "cycle_ms_difference": round(on - off, 4),
                    "cycle_ms_off_all": [round(t, 4) for t in times["off"][1:]], "cycle_ms_on_all": [round(t, 4) for t in times["on"][1:]]})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
