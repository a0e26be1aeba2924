"""What the fused-sweep tests share (test infrastructure: a plain helper module, no tests): a block on the device whose sweep
options are set launch by launch, the marker every output array starts from, the cell-by-cell check of what a sweep wrote, and
the launch forms of the tuned kernels. Used by tests/test_gpu_sweep_random_state.py, tests/test_gpu_special_states.py and the
scalar-sweep tests (tests/scalars_harness.py)."""
import ctypes as C

import numpy as np

from sweep_reference import STATE, real_mask, uv_factors

# (factor of the velocity along the axis, of the transverse one): differ in both components and between the sides, so a swap
# of the two components or of the two sides changes bits on a state whose velocities are not symmetric
F_LOW, F_HIGH = (-1., 1.), (1., -1.)
MARKER = {"float64": np.uint64(0x7ff8dead0000beef), "float32": np.uint32(0x7fc0beef)}
OUT_NAMES = STATE + ("p", "c")
TAGS = dict(scheme={"Godunov": 0, "GAD": 1}, limiter={"no_limiter": 0, "minmod": 1, "superbee": 2},
            projection={"euler": 0, "euler_2nd": 1}, eos={"perfect_gas": 0, "bizarrium": 1})
TUNED_FORMS = {0: [dict(ARMON_X_ROWS=0), dict(ARMON_X_ROWS=1), dict(ARMON_X_ROWS=2)],
               1: [dict(ARMON_Y_SX=0, ARMON_Y_COLS1=0), dict(ARMON_Y_SX=1, ARMON_Y_COLS1=0), dict(ARMON_Y_SX=2, ARMON_Y_COLS1=0),
                   dict(ARMON_Y_SX=1, ARMON_Y_COLS1=1), dict(ARMON_Y_SX=2, ARMON_Y_COLS1=1)]}
TUNED_DEFAULTS = dict(ARMON_X_ROWS=0, ARMON_Y_SX=0, ARMON_Y_COLS1=0)


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- the block on the device ---------------------------------------------------------------------------------------------

class Block:
    """A BlockGrid of one shape, ghost width and precision; the sweep's options are set on the descriptor, launch by launch."""

    def __init__(self, dev, nx, ny, g, dtype, **params):
        import armon_amd
        from armon_amd.solver import BlockGrid
        self.nx, self.ny, self.g, self.dtype = nx, ny, g, np.dtype(dtype)
        self.params = armon_amd.ArmonParameters(test="Sod", N=(nx, ny), nghost=g, data_type=dtype, silent=5, ctx=dev.ctx, **params)
        self.dev = self.params.device
        self.grid = BlockGrid(self.params)
        self.n = (nx + 2 * g) * (ny + 2 * g)
        self.marker = np.full(self.n, MARKER[self.dtype.name]).view(self.dtype)
        self.outs = {**{k: self.grid.alt[k] for k in STATE}, "p": self.grid.data["p"], "c": self.grid.data["c"]}

    def cell_size(self, axis):
        return float(self.params.cell_size(axis))

    def upload(self, f):
        for k in STATE:
            self.grid.data[k].copy_from_host(f[k])

    def mark_outputs(self):
        for a in self.outs.values():
            a.copy_from_host(self.marker)
        self.grid.dt_scalar.copy_from_host(self.marker[:2])

    def sweep(self, axis, scheme, limiter, projection, eos, exact, dt, bc=(1, 1), f_low=F_LOW, f_high=F_HIGH, emit=(0, 0),
              emit_dt=True, out_range=None, accumulate=False, cfl_sizes=None, expect=0):
        from armon_amd.blocking import Axis
        from armon_amd.solver import sweep_desc
        d = sweep_desc(self.params, self.grid, Axis.X if axis == 0 else Axis.Y, dt, self.cell_size(axis), emit_p=bool(emit[0]),
                       emit_c=bool(emit[1]), emit_dt=emit_dt, out_range=out_range, dt_accumulate=accumulate)
        d.scheme, d.limiter = TAGS["scheme"][scheme], TAGS["limiter"][limiter]
        d.projection, d.eos, d.exact = TAGS["projection"][projection], TAGS["eos"][eos], int(exact)
        d.bc_low, d.bc_high = bc
        if cfl_sizes is not None:
            d.cfl_dx, d.cfl_dy = cfl_sizes
        d.u_factor_low, d.v_factor_low = uv_factors(axis, f_low)
        d.u_factor_high, d.v_factor_high = uv_factors(axis, f_high)
        rc = self.params.fn("sweep")(self.dev.ctx, C.byref(d))
        assert rc == expect, (rc, self.dev._L.armon_hip_last_error())

    def fetch(self):
        self.dev.wait()
        out = {k: a.to_host() for k, a in self.outs.items()}
        out["dt"] = self.grid.dt_scalar.to_host()
        return out

    def set_tuning(self, **knobs):
        for k, v in knobs.items():
            assert self.dev._L.armon_hip_set_tuning(self.dev.ctx, k.encode(), int(v)) == 0, k

    def written_mask(self, axis, lo, hi):
        """The cells a sweep of the piece [lo, hi) may write: real cells, lo <= i < hi along the axis."""
        return real_mask(self.nx, self.ny, self.g, axis, lo, hi)


def block_cache():
    """Generator behind a module-scoped fixture: yields get(nx, ny, g, dtype) -> Block, one context for all of them. Keywords
    go to the block's ArmonParameters (a ghost width below 4 needs the scheme and projection that allow it)."""
    import armon_amd
    from armon_amd.device import HIPDevice
    dev = HIPDevice(0)
    cache = {}

    def get(nx, ny, g, dtype, **params):
        key = (nx, ny, g, np.dtype(dtype).name) + tuple(sorted(params.items()))
        if key not in cache:
            cache[key] = Block(dev, nx, ny, g, dtype, **params)
        return cache[key]

    yield get
    dev.wait()
    cache.clear()
    dev.close()


def check_outputs(blk, out, ref, axis, lo=0, hi=None, emit=(0, 0), emit_dt=True, exact=True, what=""):
    """Inside the written set: the reference's bits (``exact``) or at least no marker; outside it, and in every array the
    sweep was not asked for: the marker, untouched."""
    n = (blk.nx, blk.ny)[axis]
    hi = n if hi is None else hi
    inside = blk.written_mask(axis, lo, hi)
    mark = MARKER[blk.dtype.name]
    for k in OUT_NAMES:
        got = bits(out[k])
        wanted = k in STATE or (k == "p" and emit[0]) or (k == "c" and emit[1])
        if not wanted:
            assert (got == mark).all(), f"{what}{k}: written though not asked for ({(got != mark).sum()} cells)"
            continue
        stray = np.flatnonzero((got != mark) & ~inside)
        assert stray.size == 0, f"{what}{k}: {stray.size} cells written outside the piece [{lo}, {hi}), first at flat index {stray[0]}"
        missed = np.flatnonzero((got == mark) & inside)
        assert missed.size == 0, f"{what}{k}: {missed.size} cells of the piece [{lo}, {hi}) not written, first at flat index {missed[0]}"
        if exact:
            want = bits(getattr(ref, k))
            bad = np.flatnonzero((got != want) & inside)
            assert bad.size == 0, (f"{what}{k}: {bad.size} cells differ from the oracle, first at flat index {bad[0]} "
                                   f"(row pitch {blk.nx + 2 * blk.g}): {out[k][bad[0]]!r} != {getattr(ref, k)[bad[0]]!r}")
    dt = bits(out["dt"])
    assert dt[1] == mark, f"{what}dt_cfl_out: second element written"
    if not emit_dt:
        assert dt[0] == mark, f"{what}dt_cfl_out written though not asked for"
    elif exact:
        want = ref.cfl(lo, hi)
        assert out["dt"][0] == want and np.isfinite(want), f"{what}dt_cfl_out {out['dt'][0]!r} != {want!r}"


def run_tuned_forms(blk, opts, dt, bc, what):
    """One tuned sweep of the uploaded state in every launch form of the axis (TUNED_FORMS): each writes exactly the real
    cells, and all give the same bits. Returns the outputs."""
    axis = opts[0]
    results = []
    try:
        for knobs in TUNED_FORMS[axis]:
            blk.set_tuning(**knobs)
            blk.mark_outputs()
            blk.sweep(*opts, False, dt, bc=bc, emit=(1, 1))
            out = blk.fetch()
            check_outputs(blk, out, None, axis, emit=(1, 1), exact=False, what=f"{what}{knobs}: ")
            results.append(out)
    finally:
        blk.set_tuning(**TUNED_DEFAULTS)
    for knobs, out in zip(TUNED_FORMS[axis][1:], results[1:]):
        for k in OUT_NAMES + ("dt",):
            assert np.array_equal(bits(out[k]), bits(results[0][k])), f"{what}{k}: {knobs} and {TUNED_FORMS[axis][0]} differ"
    return results[0]
