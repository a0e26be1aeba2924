#!/usr/bin/env python3
"""What the mixing measures cost on the device: armon_hip_mixing (Y, width 1), its bounds pass, armon_hip_scalar_pdf (64 bins),
armon_hip_profile (Y, width 1) and armon_hip_stream_copy4 on the same vectors of a Sedov state a few cycles in that carries four
tagged scalars — fp64 and fp32, ns = 1 and ns = 4, launches interleaved in one process, event-timed, medians of ``--launches``
after ``--warmup``. The mixing pass launches once per plane and reads rho and the plane: 16 ns B per fp64 cell; the PDF 16 B,
the profile 32 B, the copy moves 64 B. Prints ONE JSON line.

    python tools/mixing_bench.py [--n 16384] [--launches 30] [--warmup 3] [--cycles 3]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import armon_amd  # noqa: E402
from armon_amd import mixing as mix  # noqa: E402
from armon_amd import profile as prof  # noqa: E402
from armon_amd._lib import PdfSpec, check  # noqa: E402
from armon_amd.problem import SCALAR_PREFIX  # noqa: E402
from armon_amd.solver import STATE_VARS  # noqa: E402

NAMES = ("a", "b", "c", "d")


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def one_type(a, dtype):
    Box, Scalar = armon_amd.Box, armon_amd.Scalar
    tags = [Scalar("a", regions=[(Box(y=(0., 9.)), 1.)]), Scalar("b", regions=[(Box(x=(0., 9.)), 1.)]),
            Scalar("c", regions=[(Box(x=(-0.5, 0.5), y=(-0.5, 0.5)), 1.)]), Scalar("d", background=0.5)]
    params = armon_amd.ArmonParameters(test="Sedov", N=(a.n, a.n), data_type=dtype, silent=5, placement_tries=0, maxcycle=a.cycles,
                                       return_data=True, scalars=tags)
    grid = armon_amd.armon(params).data
    dev = params.device
    tile, window = (params, grid), (0, 0, a.n, a.n)
    src, dst = [grid.data[f] for f in STATE_VARS], [grid.alt[f] for f in STATE_VARS]
    nb = src[0].nbytes & ~15
    item = np.dtype(params.data_type).itemsize
    res = {"N": [a.n, a.n]}
    # the profile's Y pass, for comparison
    p_spec = prof.make_spec(params, "y", width=1)
    p_c = prof._c_spec(p_spec, prof.default_scale(prof.state_bounds([tile], p_spec)))
    p_bins = dev.empty(p_spec[2] * prof.WORDS, np.uint64)
    check(dev._L.armon_hip_profile_reset(dev.ctx, p_spec[2], C.c_void_p(p_bins.ptr)))
    spec = mix.make_spec(params, "y", 1)
    head, win = mix._geometry(params, grid, window)
    rho = C.c_void_p(grid.data["rho"].ptr)
    runs = a.warmup + a.launches
    copies = []
    for ns in (1, 4):
        names = NAMES[:ns]
        bounds = mix.state_bounds([tile], spec, names)
        c_spec = mix._c_spec(spec, [mix.default_scale(b) for b in bounds])
        bins, top = dev.empty(ns * spec[1] * mix.WORDS, np.uint64), dev.zeros(5 * ns, np.uint64)
        check(dev._L.armon_hip_mixing_reset(dev.ctx, ns, spec[1], C.c_void_p(bins.ptr)))
        pdf = PdfSpec()
        pdf.lo, pdf.inv_w, pdf.nbins, pdf.rho_scale_exp = 0.0, 64.0, 64, mix.default_scale(bounds[0])[0]
        hist = dev.empty(mix.pdf_words(64), np.uint64)
        check(dev._L.armon_hip_scalar_pdf_reset(dev.ctx, 64, C.c_void_p(hist.ptr)))
        phi0 = C.c_void_p(grid.data[SCALAR_PREFIX + "a"].ptr)
        t = {k: [] for k in ("mixing", "bounds", "pdf", "profile", "copy4")}
        for k in range(runs):
            dev.event_record(20)
            mix._call_mixing("mixing", params, grid, names, window, c_spec, bins)
            dev.event_record(21)
            mix._call_mixing("mixing_bounds", params, grid, names, window, c_spec, top)
            dev.event_record(22)
            check(params.fn("scalar_pdf")(*head, rho, phi0, *win, C.byref(pdf), C.c_void_p(hist.ptr)))
            dev.event_record(23)
            prof._call("profile", params, grid, window, p_c, p_bins)
            dev.event_record(24)
            dev.stream_copy4(src, dst, nb)
            dev.event_record(25)
            dev.wait()
            if k >= a.warmup:
                for i, name in enumerate(t):
                    t[name].append(dev.event_elapsed_ms(20 + i, 21 + i))
        raw = bins.to_host().reshape(ns, spec[1], mix.WORDS)            # every launch merged the same cells into the same bins
        assert int(raw[:, :, mix.W_N].sum()) == runs * ns * a.n * a.n and not raw[:, :, mix.W_BAD].any()
        words = hist.to_host()
        assert int(words[:-1].reshape(-1, 4)[:, 0].sum()) == runs * a.n * a.n and words[-1] == 0
        for buf in (bins, top, hist):
            buf.free()
        copies.extend(t["copy4"])
        cells = a.n * a.n * item
        for name, bytes_per_cell in (("mixing", 2 * ns), ("bounds", 2 * ns), ("pdf", 2), ("profile", 4)):
            ms = median(t[name])
            res[f"{name}_ns{ns}_ms"], res[f"{name}_ns{ns}_GBps"] = round(ms, 4), round(bytes_per_cell * cells / ms / 1e6, 1)
            res[f"{name}_ns{ns}_ms_min"], res[f"{name}_ns{ns}_ms_max"] = round(min(t[name]), 4), round(max(t[name]), 4)
        res[f"copy4_ns{ns}_ms"] = round(median(t["copy4"]), 4)
        res[f"copy4_ns{ns}_ms_min"], res[f"copy4_ns{ns}_ms_max"] = round(min(t["copy4"]), 4), round(max(t["copy4"]), 4)
        res[f"mixing_ns{ns}_per_plane_over_profile"] = round(median(t["mixing"]) / ns / median(t["profile"]), 4)
    p_bins.free()
    copy4 = median(copies)
    res.update({"copy4_ms": round(copy4, 4), "copy4_GBps": round(8 * nb / copy4 / 1e6, 1),
                "copy4_spread": round((max(copies) - min(copies)) / copy4, 4)})
    for ns in (1, 4):
        res[f"mixing_ns{ns}_over_copy4"] = round(res[f"mixing_ns{ns}_ms"] / copy4, 4)
    res["pdf_over_copy4"] = round(res["pdf_ns1_ms"] / copy4, 4)
    return dev.name, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cycles", type=int, default=3)
    a = ap.parse_args()
    res = {"tool": "mixing_bench", "launches": a.launches, "warmup": a.warmup, "cycles": a.cycles}
    for dtype in ("float64", "float32"):
        res["device"], res[dtype] = one_type(a, dtype)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
