"""What the tests of armon_hip_sweep_scalars share (test infrastructure: a plain helper module, no tests): the planes of a
harness block on the device, the descriptor and the launch through the C ABI, random planes, the cell-by-cell check of one
exact launch against the restatement (tests/scalars_restated.py), and the yardstick of the tuned arithmetic. Used by
tests/test_gpu_scalars.py, test_gpu_scalars_long_blocks.py, test_gpu_scalars_shapes.py and test_gpu_scalars_special.py."""
import ctypes as C
import functools

import numpy as np

from scalars_restated import restated_sweep
from sweep_harness import F_HIGH, F_LOW, MARKER, TAGS, bits
from sweep_reference import STATE, rand_dt, rand_state, real_mask, uv_factors

WALLS = dict(f_low=(-1., 1.), f_high=(1., 1.))          # mirrors whose transverse factor is +1: the one a plane is mirrored with


def lag_of(scheme, projection):
    return 2 + (scheme == "GAD") + (projection == "euler_2nd")


class Planes:
    """``ns`` input planes and ``ns`` output planes on the device of a harness block."""

    def __init__(self, blk, ns):
        self.blk, self.ns = blk, ns
        self.inp = [blk.dev.empty(blk.n, blk.dtype) for _ in range(ns)]
        self.out = [blk.dev.empty(blk.n, blk.dtype) for _ in range(ns)]

    def upload(self, planes):
        for a, h in zip(self.inp, planes):
            a.copy_from_host(h)
        for a in self.out:
            a.copy_from_host(self.blk.marker)

    def fetch(self):
        self.blk.dev.wait()
        return [a.to_host() for a in self.inp], [a.to_host() for a in self.out]

    def free(self):
        self.blk.dev.wait()
        for a in self.inp + self.out:
            a.free()


def descriptor(blk, axis, scheme, limiter, projection, eos, exact, dt, bc=(1, 1), f_low=F_LOW, f_high=F_HIGH):
    from armon_amd.blocking import Axis
    from armon_amd.solver import sweep_desc
    d = sweep_desc(blk.params, blk.grid, Axis.X if axis == 0 else Axis.Y, dt, blk.cell_size(axis), emit_p=True, emit_c=True, emit_dt=True)
    d.scheme, d.limiter = TAGS["scheme"][scheme], TAGS["limiter"][limiter]
    d.projection, d.eos, d.exact = TAGS["projection"][projection], TAGS["eos"][eos], int(exact)
    d.bc_low, d.bc_high = bc
    d.u_factor_low, d.v_factor_low = uv_factors(axis, f_low)
    d.u_factor_high, d.v_factor_high = uv_factors(axis, f_high)
    return d


def launch(blk, d, inp, out, ns=None, expect=0, entry="sweep_scalars"):
    ns = len(inp) if ns is None else ns
    a = (C.c_void_p * max(len(inp), 1))(*[x.ptr if x is not None else None for x in inp])
    b = (C.c_void_p * max(len(out), 1))(*[x.ptr if x is not None else None for x in out])
    rc = blk.params.fn(entry)(blk.dev.ctx, C.byref(d), ns, a, b)
    msg = blk.dev._L.armon_hip_last_error().decode()
    assert (rc == 0) == (expect == 0) and (expect == 0 or rc == expect), (rc, msg)
    return msg


def bounded_launch(blk, d, inp, out, ns=None, expect=0):
    """``launch`` through armon_hip_sweep_scalars_bounded[_f32]."""
    return launch(blk, d, inp, out, ns, expect, entry="sweep_scalars_bounded")


def rand_planes(nx, ny, g, ns, dtype, seed):
    rng = np.random.default_rng(seed)
    return [rng.uniform(-1., 2., (nx + 2 * g) * (ny + 2 * g)).astype(dtype) for _ in range(ns)]


def case_numbers(nx, ny, axis, eos, dtype):
    T = np.dtype(dtype).type
    cs = [float(T(1.) / T(nx)), float(T(1.) / T(ny))]            # ArmonParameters.cell_size of the unit square
    return float(np.float32(rand_dt(eos, cs[axis]))), cs[axis]


def assert_untouched(blk, f, what):
    """The eight state arrays of the descriptor, p, c and the dt scalar after a scalar sweep: the input as uploaded, the marker."""
    mark = MARKER[blk.dtype.name]
    host = blk.grid.device_to_host(STATE)
    for k in STATE:
        assert np.array_equal(bits(host[k]), bits(f[k])), f"{what}: the state's {k} was modified"
    out = blk.fetch()
    for k, a in out.items():
        assert (bits(a) == mark).all(), f"{what}: {k} of the descriptor's outputs was written"


def assert_planes_are(blk, got_in, got, planes, want, axis, what=""):
    """After one exact launch: phi_in as uploaded; phi_out the marker outside the real cells and the bits of ``want`` (finite)
    on every real cell, signs of zero included."""
    nx, ny, g = blk.nx, blk.ny, blk.g
    inside = real_mask(nx, ny, g, axis)
    mark = MARKER[blk.dtype.name]
    for k in range(len(planes)):
        assert np.isfinite(want[k][inside]).all(), f"{what}the restatement of plane {k} is not finite"
        assert np.array_equal(bits(got_in[k]), bits(planes[k])), f"{what}phi_in[{k}] was modified"
        stray = np.flatnonzero((bits(got[k]) != mark) & ~inside)
        assert stray.size == 0, f"{what}phi_out[{k}]: {stray.size} cells written outside the real cells, first at {stray[0]}"
        bad = np.flatnonzero((bits(got[k]) != bits(want[k])) & inside)
        assert bad.size == 0, (f"{what}phi_out[{k}]: {bad.size} cells differ from the restatement, first at flat index {bad[0]} "
                               f"(pitch {nx + 2 * g}): {got[k][bad[0]]!r} != {want[k][bad[0]]!r}")


def exact_launch_is_the_restatement(blk, f, planes, want, axis, scheme, limiter, projection, eos, dt, bc=(1, 1), each_alone=True,
                                    what="", launch=launch):
    """Upload the state ``f`` and ``planes``, run one exact launch of all of them and check it (assert_planes_are,
    assert_untouched); with ``each_alone``, plane k of the ns-launch is the ns = 1 launch on it. ``launch`` is the entry point's:
    ``launch`` above, or ``bounded_launch``. Returns phi_out."""
    ns = len(planes)
    P = Planes(blk, ns)
    try:
        blk.upload(f)
        blk.mark_outputs()
        P.upload(planes)
        d = descriptor(blk, axis, scheme, limiter, projection, eos, True, dt, bc=bc)
        launch(blk, d, P.inp, P.out)
        got_in, got = P.fetch()
        assert_planes_are(blk, got_in, got, planes, want, axis, what)
        assert_untouched(blk, f, what + "exact scalar sweep")
        if each_alone and ns > 1:
            for k in range(ns):
                P.out[0].copy_from_host(blk.marker)
                launch(blk, d, [P.inp[k]], [P.out[0]])
                blk.dev.wait()
                assert np.array_equal(bits(P.out[0].to_host()), bits(got[k])), f"{what}plane {k}: ns = 1 and ns = {ns} differ"
        return got
    finally:
        P.free()


def plane_kappa(f32, planes32, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, f_low=F_LOW, f_high=F_HIGH):
    """Per plane max|restated32 - restated64| / (eps32 max|restated64|) over the real cells, both restatements on the SAME
    numbers — state, planes, cell size and step in fp32; 0 where the fp64 plane is 0 everywhere. Returns (kappas, the fp64
    restatement of those fp32 inputs)."""
    opts = (nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, 1, 1, f_low, f_high)
    o32, _ = restated_sweep(f32, planes32, *opts, "float32")
    o64, _ = restated_sweep({k: a.astype(np.float64) for k, a in f32.items()}, [p.astype(np.float64) for p in planes32], *opts, "float64")
    inside = real_mask(nx, ny, g, axis)
    eps32 = float(np.finfo(np.float32).eps)
    kappa = []
    for a32, a64 in zip(o32, o64):
        top = np.abs(a64[inside]).max()
        kappa.append(float(np.abs(a32[inside].astype(np.float64) - a64[inside]).max() / (eps32 * top)) if top > 0 else 0.)
    return kappa, o64


@functools.lru_cache(maxsize=None)
def kappa_of_plane(nx, ny, g, axis, scheme, limiter, projection, eos, seed):
    """As kappa_of of tests/test_gpu_sweep_random_state.py, for the planes: max|restated32 - restated64| / (eps32 max|restated64|)
    over the real cells, both restatements on the SAME numbers — state, planes, cell size and step rounded to fp32. Returns
    kappa per plane."""
    f32 = rand_state(nx, ny, g, eos, "float32", seed)
    planes32 = rand_planes(nx, ny, g, 2, "float32", seed + 1)
    dt, dx = case_numbers(nx, ny, axis, eos, "float32")
    kappa, _ = plane_kappa(f32, planes32, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx)
    assert all(k > 0.5 for k in kappa), kappa              # a yardstick, not an accident of one cell
    return kappa
