"""Run history (csrc/history.hip): the global integrals, the extrema with their cells and a few point gauges of the state,
sampled EXACTLY where it lives, over time. No reference counterpart: the reference prints mass and energy per cycle behind a
fence (ref src/solver.jl:356-371).

PER CELL at the global 0-based position ``(gx, gy)``, all arithmetic in fp64 (fp32 values converted first):

    q2      = u u + v v,   e = E - 0.5 q2
    p, c    the EOS of the cell in the data type, converted
    terms   rho, rho u, rho v, rho E, (0.5 rho) q2, p
    Q_k     = round-half-even(t_k / 2^s_k), an exact integer; limbs as in profile.py
    m       = 0 where q2 == 0, q2 / (c c) otherwise (the square of the Mach number)
    ext     (order key, g = gy NX + gx) pairs: rho, p, e a minimum and a maximum, q2 and m a maximum; equal keys: the smaller g
    bad     one of rho, u, v, E, e, c, t_k not finite or a |Q_k| >= 2^95: the cell adds 1 to n_bad and nothing else

Every addend is rounded once, on its own; everything after is integer addition, a pair minimum or a pair maximum. So the
record (40 words, ``armon_history_record``) is a function of the state and the scale only, and the records of the tiles of a
group merge to the single block's WORD FOR WORD. Internal energy is not summed: with ``s_3 == s_4`` it is ``S3 - S4``, exactly.

A sample is ENQUEUED on the stream behind the cycle and written into a ring on the device; the host reads the ring in
batches (``Sampler.read``), so a run sampled every cycle never waits for its history. ``cell_terms`` / ``reference_record`` /
``merge_raw`` below restate the rule in Python; the tests hold the kernel against them.
"""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

from ._lib import HistorySpec, check, solver_error
from .profile import MASK, SCALE_LIMIT, from_key, from_limbs, limbs, order_key, quantise, quantise_limbs  # noqa: F401  (the rule's parts)

WORDS = 40
W_N, W_BAD, W_SUM, W_EXT = 0, 1, 2, 20
TERMS = ("rho", "rho_u", "rho_v", "rho_E", "kinetic", "p")
EXTREMA = ("rho_min", "rho_max", "p_min", "p_max", "e_min", "e_max", "q2_max", "mach2_max")
MIN_EXTREMA = (0, 2, 4)
GAUGE_VARS = ("rho", "u", "v", "E", "p")
MAX_GAUGES = 64
HEADROOM = 16               # bits every term may grow by before a cell goes BAD under the default scale
FIRST_SCALE = (1024,) * 6   # the scale of the sample the default scale is taken from: no finite term reaches 2^95 quanta of 2^1024
SUMS = ("mass", "momentum_x", "momentum_y", "energy", "kinetic", "pressure")
COLUMNS = ("cycle", "time", "dt", "n", "n_bad", "mass", "momentum_x", "momentum_y", "energy", "kinetic", "internal", "pressure",
           "rho_min", "rho_max", "p_min", "p_max", "e_min", "e_max", "speed_max", "mach_max") \
    + tuple(f"{name}_{ax}" for name in ("rho_min", "rho_max", "p_min", "p_max", "e_min", "e_max", "speed_max", "mach_max") for ax in ("gx", "gy"))
FORMAT_VERSION = 1


# ---- the rule, in Python (the tests' oracle) -------------------------------------------------------------------------------
def cell_terms(rho, u, v, E, p, c):
    """Cells holding ``rho, u, v, E`` with the EOS values ``p, c`` of the data type (scalars or arrays of one shape; fp32 inputs
    are converted first) → ``(t, x)``: the six terms and the eight values that enter the extrema, fp64. One numpy operation
    per operation of the rule."""
    rho, u, v, E, p, c = (np.asarray(a).astype(np.float64) for a in (rho, u, v, E, p, c))
    with np.errstate(all="ignore"):
        q2 = u * u + v * v
        e = E - 0.5 * q2
        t = [rho, rho * u, rho * v, rho * E, (0.5 * rho) * q2, p]
        m = np.where(q2 == 0., 0., q2 / (c * c))
    return t, [rho, rho, p, p, e, e, q2, m]


def neutral():
    raw = np.zeros(WORDS, dtype=np.uint64)
    for k in range(8):
        raw[W_EXT + 2 * k] = MASK if k in MIN_EXTREMA else 0
        raw[W_EXT + 2 * k + 1] = MASK
    return raw


def reference_record(rho, u, v, E, p, c, origin=(0, 0), global_nx=None, scale_exp=(0,) * 6):
    """The record of the 2-D arrays ``rho, u, v, E`` (+ the EOS values ``p, c`` of the data type) whose first cell sits at global
    ``origin = (gx, gy)`` of a grid ``global_nx`` wide (default: the arrays' own width) → ``(40,)`` uint64."""
    ny, nx = np.shape(rho)
    global_nx = int(origin[0]) + nx if global_nx is None else int(global_nx)
    g = ((np.arange(ny, dtype=np.int64)[:, None] + int(origin[1])) * np.int64(global_nx)
         + (np.arange(nx, dtype=np.int64)[None, :] + int(origin[0])))
    t, x = cell_terms(rho, u, v, E, p, c)
    ok = np.ones((ny, nx), dtype=bool)
    for a in [np.asarray(a).astype(np.float64) for a in (rho, u, v, E, c)] + [x[4]]:
        ok &= np.isfinite(a)
    quanta = []
    for k in range(6):
        l0, l1, l2, good = quantise_limbs(t[k], scale_exp[k])
        ok &= good
        quanta.append((l0, l1, l2))
    w = [int(v) for v in neutral()]
    w[W_N], w[W_BAD] = int(ok.sum()), int((~ok).sum())
    for k in range(6):
        sign = np.where(np.signbit(t[k][ok]), -1, 1).astype(np.int64)
        for j in range(3):
            w[W_SUM + 3 * k + j] = int((quanta[k][j][ok].astype(np.int64) * sign).sum(dtype=np.int64))
    if w[W_N]:
        at = g[ok]
        for k in range(8):
            bits = np.ascontiguousarray(x[k][ok]).view(np.uint64)
            keys = np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ np.uint64(1 << 63))
            top = keys.min() if k in MIN_EXTREMA else keys.max()
            w[W_EXT + 2 * k], w[W_EXT + 2 * k + 1] = int(top), int(at[keys == top].min())
    return np.array([v & MASK for v in w], dtype=np.uint64)


def merge_raw(x, y):
    """The merge of two ``(40,)`` records: sums add (mod 2^64, limb by limb); a pair takes the smaller (minimum) or the larger
    (maximum) key and on equal keys the smaller position."""
    out = x + y                                 # (unsigned: wraps like the device's integer adds)
    for k in range(8):
        i = W_EXT + 2 * k
        a, b = (int(x[i]), int(x[i + 1])), (int(y[i]), int(y[i + 1]))
        better = b[0] < a[0] if k in MIN_EXTREMA else b[0] > a[0]
        out[i], out[i + 1] = b if (better or (b[0] == a[0] and b[1] < a[1])) else a
    out[W_EXT + 16:] = 0
    return out


def _exponent(bound):
    """e with ``bound < 2^e`` (the frexp exponent); 0 for a bound of 0 or one that is not finite."""
    return math.frexp(bound)[1] if (bound != 0 and math.isfinite(bound)) else 0


def default_scale(raw):
    """The six exponents from the EXTREMA of a first sample (they do not depend on the scale it was taken with while that scale
    refuses no cell: ``FIRST_SCALE`` refuses none whose terms are finite): with
    ``B_rho = max |rho|``, ``B_E = max |e| + q2_max / 2``, ``B_p = max |p|`` and ``e(B)`` the exponent with ``B < 2^e``:
    ``s_rho = e(B_rho) + 16 - 94``, ``s_rhoE = s_ke = e(B_rho B_E) + 16 - 94``, ``s_mom = e(B_rho sqrt(2 B_E)) + 16 - 94``,
    ``s_p = e(B_p) + 16 - 94``. Every term may grow 65 536-fold before a cell goes BAD; the momentum and kinetic scales come
    from the energy bound, not from the initial velocities (0 in Sod); the energy and kinetic scales agree, so that the
    internal energy is their exact difference."""
    if int(raw[W_N]) == 0:
        return (HEADROOM - 94,) * 6
    val = [from_key(int(raw[W_EXT + 2 * k])) for k in range(8)]
    B_rho, B_p = max(abs(val[0]), abs(val[1])), max(abs(val[2]), abs(val[3]))
    B_E = max(abs(val[4]), abs(val[5])) + 0.5 * val[6]
    s_rho, s_p = _exponent(B_rho) + HEADROOM - 94, _exponent(B_p) + HEADROOM - 94
    s_E = _exponent(B_rho * B_E) + HEADROOM - 94
    s_mom = _exponent(B_rho * math.sqrt(2. * B_E)) + HEADROOM - 94
    return (s_rho, s_mom, s_mom, s_E, s_E, s_p)


def check_scale(scale_exp):
    try:
        scale_exp = tuple(int(s) for s in scale_exp)
        good = len(scale_exp) == 6 and all(abs(s) <= SCALE_LIMIT for s in scale_exp)
    except (TypeError, ValueError):
        good = False
    if not good:
        solver_error("config", f"history_scale_exp takes six integer exponents within ±{SCALE_LIMIT}, got {scale_exp!r}")
    return scale_exp


# ---- the result ------------------------------------------------------------------------------------------------------------
class HistoryRecord:
    """One sample. ``raw``: the 40 words; ``scale_exp``; ``ds``: the area of a cell; ``global_nx``. Decoded: ``n``, ``n_bad``;
    ``sums[k]`` (exact Python ints, in quanta ``2^scale_exp[k]``); ``mass``, ``momentum_x``, ``momentum_y``, ``energy``,
    ``kinetic``, ``pressure`` = sum x ds and ``internal`` = (S3 - S4) x ds (needs ``scale_exp[3] == scale_exp[4]``, NaN
    otherwise), each fp64 rounded once from the exact rational; the extrema ``rho_min`` … ``e_max``, ``speed_max`` and
    ``mach_max`` (the square roots of the q2 and m maxima) and ``at[name]`` = the global ``(gx, gy)`` of the first cell that
    attains each (None while no cell was added)."""

    def __init__(self, raw, scale_exp, ds, global_nx):
        self.raw = np.ascontiguousarray(raw, dtype=np.uint64).reshape(WORDS)
        self.scale_exp, self.ds, self.global_nx = tuple(int(s) for s in scale_exp), float(ds), int(global_nx)
        self.n, self.n_bad = int(self.raw[W_N]), int(self.raw[W_BAD])
        signed = self.raw[W_SUM:W_EXT].view(np.int64).reshape(6, 3).tolist()
        self.sums = tuple(from_limbs(row) for row in signed)
        ds_q = Fraction(self.ds)

        def value(S, s):
            try:
                return float(S * Fraction(2) ** s * ds_q)
            except OverflowError:
                return math.copysign(math.inf, S)
        for k, name in enumerate(SUMS):
            setattr(self, name, value(self.sums[k], self.scale_exp[k]))
        same = self.scale_exp[3] == self.scale_exp[4]
        self.internal = value(self.sums[3] - self.sums[4], self.scale_exp[3]) if same else math.nan
        self.at = {}
        for k, name in enumerate(EXTREMA):
            key, g = int(self.raw[W_EXT + 2 * k]), int(self.raw[W_EXT + 2 * k + 1])
            val = from_key(key) if self.n else math.nan
            name = {"q2_max": "speed_max", "mach2_max": "mach_max"}.get(name, name)
            setattr(self, name, math.sqrt(val) if name in ("speed_max", "mach_max") and self.n else val)
            self.at[name] = (g % self.global_nx, g // self.global_nx) if (self.n and g != MASK) else None

    def row(self):
        """The record's columns of a history file, in the order of ``COLUMNS[3:]``."""
        out = [float(self.n), float(self.n_bad)] + [getattr(self, c) for c in COLUMNS[5:20]]
        for name in COLUMNS[12:20]:
            out += [float(v) for v in (self.at[name] or (-1, -1))]
        return out

    def merge(self, other):
        if (self.scale_exp, self.ds, self.global_nx) != (other.scale_exp, other.ds, other.global_nx):
            solver_error("config", f"history records of another scale or grid do not merge: {self.scale_exp} against {other.scale_exp}")
        return HistoryRecord(merge_raw(self.raw, other.raw), self.scale_exp, self.ds, self.global_nx)

    def __eq__(self, other):
        return isinstance(other, HistoryRecord) and (self.scale_exp, self.ds, self.global_nx) == (other.scale_exp, other.ds, other.global_nx) \
            and np.array_equal(self.raw, other.raw)

    def __repr__(self):
        return f"HistoryRecord(n = {self.n}, n_bad = {self.n_bad}, mass = {self.mass!r}, energy = {self.energy!r})"


class History:
    """The rows of a run: ``cycle``, ``time``, ``dt`` (the step the completed cycle advanced by, 0 for the first row) per row,
    ``raw`` = the ``(rows, 40)`` words, ``gauge_values`` = ``(rows, gauges, 5)`` fp64 (rho, u, v, E, p); ``scale_exp``, ``ds``,
    ``global_nx``, ``gauges`` = the points and ``gauge_cells`` = their global ``(gx, gy)``. ``records[i]``: row i decoded;
    ``history.mass`` …: one array per column of ``COLUMNS``; ``gauges_of(i)``: dict name → array over the rows."""

    def __init__(self, scale_exp, ds, global_nx, gauges=(), gauge_cells=()):
        self.scale_exp, self.ds, self.global_nx = tuple(int(s) for s in scale_exp), float(ds), int(global_nx)
        self.gauges = tuple((float(x), float(y)) for x, y in gauges)
        self.gauge_cells = tuple((int(x), int(y)) for x, y in gauge_cells)
        self.cycle, self.time, self.dt = [], [], []
        self.raw = np.zeros((0, WORDS), dtype=np.uint64)
        self.gauge_values = np.zeros((0, len(self.gauges), 5), dtype=np.float64)
        self._records = []

    def append(self, cycle, time, dt, raw, gauge_values):
        raw = np.asarray(raw, dtype=np.uint64).reshape(-1, WORDS)
        self.cycle += [int(c) for c in np.atleast_1d(cycle)]
        self.time += [float(t) for t in np.atleast_1d(time)]
        self.dt += [float(t) for t in np.atleast_1d(dt)]
        self.raw = np.concatenate([self.raw, raw])
        self.gauge_values = np.concatenate([self.gauge_values, np.asarray(gauge_values, dtype=np.float64).reshape(len(raw), len(self.gauges), 5)])
        assert len(self.cycle) == len(self.time) == len(self.dt) == len(self.raw)

    def __len__(self):
        return len(self.cycle)

    @property
    def records(self):
        while len(self._records) < len(self.raw):
            self._records.append(HistoryRecord(self.raw[len(self._records)], self.scale_exp, self.ds, self.global_nx))
        return self._records

    def rows(self, start=0):
        """Rows ``start`` … as lists of floats: ``COLUMNS``, then the five values of every gauge."""
        return [[float(self.cycle[i]), self.time[i], self.dt[i]] + self.records[i].row() + [float(v) for v in self.gauge_values[i].ravel()]
                for i in range(start, len(self))]

    def table(self):
        """Everything a history file holds → dict (``io.read_history_file`` returns the same)."""
        rows = np.array(self.rows(), dtype=np.float64).reshape(len(self), len(COLUMNS) + 5 * len(self.gauges))
        t = {"version": FORMAT_VERSION, "scale_exp": self.scale_exp, "ds": self.ds, "global_nx": self.global_nx,
             "gauges": self.gauges, "gauge_cells": self.gauge_cells}
        for k, c in enumerate(COLUMNS):
            t[c] = rows[:, k].copy()
        for i in range(len(self.gauges)):
            for j, name in enumerate(GAUGE_VARS):
                t[f"g{i}_{name}"] = rows[:, len(COLUMNS) + 5 * i + j].copy()
        return t

    def gauges_of(self, i):
        return {name: self.gauge_values[:, i, j].copy() for j, name in enumerate(GAUGE_VARS)}

    def __getattr__(self, name):
        if name in COLUMNS[3:]:
            k = COLUMNS.index(name) - 3
            return np.array([r.row()[k] for r in self.records], dtype=np.float64)
        raise AttributeError(name)

    def _meta(self):
        return (self.scale_exp, self.ds, self.global_nx, self.gauges, self.gauge_cells)

    def concat(self, other):
        if self._meta() != other._meta():
            solver_error("config", "histories of another scale, grid or set of gauges do not join")
        out = History(*self._meta())
        for h in (self, other):
            if len(h):
                out.append(h.cycle, h.time, h.dt, h.raw, h.gauge_values)
        return out

    def __eq__(self, other):
        return isinstance(other, History) and self._meta() == other._meta() and self.cycle == other.cycle \
            and np.array_equal(np.array(self.time).view(np.uint64), np.array(other.time).view(np.uint64)) \
            and np.array_equal(np.array(self.dt).view(np.uint64), np.array(other.dt).view(np.uint64)) \
            and np.array_equal(self.raw, other.raw) \
            and np.array_equal(self.gauge_values.view(np.uint64), other.gauge_values.view(np.uint64))

    def __repr__(self):
        return f"History({len(self)} rows, {len(self.gauges)} gauges, scale_exp={self.scale_exp})"


# ---- device side -----------------------------------------------------------------------------------------------------------
def gauge_cells(p0, gauges):
    """The global 0-based cell ``(gx, gy)`` that contains each point (the domain is closed: a point on its upper edge belongs
    to the last cell). A point outside the domain is a configuration error."""
    NX, NY = p0.global_grid
    cells = []
    for pt in gauges:
        try:
            x, y = (float(c) for c in pt)
        except (TypeError, ValueError):
            solver_error("config", f"history_gauges takes (x, y) points, got {pt!r}")
        pos = []
        for c, o, L, n, h in ((x, p0.origin[0], p0.domain_size[0], NX, p0.cell_size(0)), (y, p0.origin[1], p0.domain_size[1], NY, p0.cell_size(1))):
            if not (math.isfinite(c) and float(o) <= c <= float(o) + float(L)):
                solver_error("config", f"the history gauge {pt!r} lies outside the domain [{o}, {float(o) + float(L)}] of its axis")
            pos.append(min(int(math.floor((c - float(o)) / float(h))), n - 1))
        cells.append(tuple(pos))
    return cells


class Sampler:
    """The device side of a history of the state held by ``tiles`` = ``[(params, grid), ...]``: one ring of ``capacity`` slots per
    tile (armon_hip_history_create), the gauges resolved once. ``enqueue(slot)`` puts one sample of every tile on its stream
    and returns; ``read(first, count)`` waits for them and merges the tiles' slots → ``(raw (count, 40), gauge values (count,
    gauges, 5))``. ``close()`` releases the rings (before the contexts go)."""

    def __init__(self, tiles, capacity=1, gauges=(), scale_exp=(0,) * 6):
        self.tiles, self.capacity = list(tiles), int(capacity)
        p0 = self.tiles[0][0]
        self.gauges = tuple((float(x), float(y)) for x, y in gauges)
        if len(self.gauges) > MAX_GAUGES:
            solver_error("config", f"history_gauges: {len(self.gauges)} points, at most {MAX_GAUGES}")
        self.gauge_cells = tuple(gauge_cells(p0, self.gauges))
        self.global_nx = int(p0.global_grid[0])
        self.ds = float(p0.cell_size(0)) * float(p0.cell_size(1))
        self.eos, self.gamma = (1 if p0.test.eos == "bizarrium" else 0), float(p0.test.gamma)
        self.set_scale(scale_exp)
        self.handles, self.owner = [], []           # owner[i]: the tile that holds gauge i
        try:
            for params, _ in self.tiles:
                h = C.c_void_p()
                check(params.device._L.armon_hip_history_create(params.device.ctx, self.capacity, len(self.gauges), C.byref(h)))
                self.handles.append(h)
            for t, (params, _) in enumerate(self.tiles):
                ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
                local = []
                for gx, gy in self.gauge_cells:
                    inside = ox <= gx < ox + params.N[0] and oy <= gy < oy + params.N[1]
                    local.append((gy - oy) * params.N[0] + (gx - ox) if inside else -1)
                if local:
                    check(params.device._L.armon_hip_history_set_gauges(params.device.ctx, self.handles[t], (C.c_int64 * len(local))(*local), len(local)))
                self.owner.append(local)
            self.owner = [next(t for t, local in enumerate(self.owner) if local[i] >= 0) for i in range(len(self.gauges))]
        except BaseException:
            self.close()
            raise

    def set_scale(self, scale_exp):
        self.scale_exp = check_scale(scale_exp)
        self.spec = HistorySpec()
        self.spec.eos, self.spec.gamma, self.spec.global_nx = self.eos, self.gamma, self.global_nx
        self.spec.scale_exp[:] = list(self.scale_exp)

    def enqueue(self, slot):
        for (params, grid), h in zip(self.tiles, self.handles):
            check(params.fn("history_sample")(params.device.ctx, h, int(slot), C.byref(self.spec), grid.size.size[0], grid.size.ghosts,
                                               params.N[0], params.N[1], *[C.c_void_p(grid.data[f].ptr) for f in ("rho", "u", "v", "E")],
                                               0, 0, params.N[0], params.N[1], params.N_origin[0] - 1, params.N_origin[1] - 1))

    def read(self, first, count):
        ng = len(self.gauges)
        raw = np.tile(neutral(), (count, 1))
        values = np.zeros((count, ng, 5), dtype=np.float64)
        for t, ((params, _), h) in enumerate(zip(self.tiles, self.handles)):
            rec = np.empty((count, WORDS), dtype=np.uint64)
            gv = np.empty((count, ng, 5), dtype=np.float64)
            check(params.device._L.armon_hip_history_read(params.device.ctx, h, int(first), int(count), rec.ctypes.data_as(C.c_void_p),
                                                           gv.ctypes.data_as(C.c_void_p) if ng else None))
            for i in range(count):
                raw[i] = merge_raw(raw[i], rec[i])
            for g in range(ng):
                if self.owner[g] == t:
                    values[:, g, :] = gv[:, g, :]
        return raw, values

    def close(self):
        for (params, _), h in zip(self.tiles, self.handles):
            if h and params.device.ctx:
                params.device._L.armon_hip_history_destroy(params.device.ctx, h)
        self.handles = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_state(tiles, gauges=(), scale_exp=None):
    """One synchronous sample of the state held by ``tiles`` (at rest) → ``(HistoryRecord, gauge values (gauges, 5))``.
    ``scale_exp=None``: the default scale — a first sample gives the extrema, ``default_scale`` the exponents, and the sample
    is retaken with them."""
    s = Sampler(tiles, 1, gauges, FIRST_SCALE if scale_exp is None else scale_exp)
    try:
        s.enqueue(0)
        raw, values = s.read(0, 1)
        if scale_exp is None:
            s.set_scale(default_scale(raw[0]))
            s.enqueue(0)
            raw, values = s.read(0, 1)
        return HistoryRecord(raw[0], s.scale_exp, s.ds, s.global_nx), values[0]
    finally:
        s.close()


# ---- the run options (history_step, history_file, history_gauges, history_capacity, history_scale_exp) ---------------------
def history_path(params):
    return os.path.join(params.output_dir, f"{params.history_file}.txt")


class HistoryRun:
    """The history of the run ``owner`` (a ``BlockGrid`` or a ``TileGroup``): ``start`` after the initial state (or the restart)
    is in place, ``sample(gdt, dt)`` after a completed cycle — ENQUEUED on a single block's stream with no wait; a group is
    sampled at rest, its boundary strips being written on other streams — ``flush`` when the ring is full, before a
    checkpoint and at the end: the slots are read, the rows appended to ``history`` and to the file. ``io_ns``: what the reads
    and the file cost, to be taken out of the solve time."""

    def __init__(self, owner, params):
        self.owner, self.params = owner, params
        self.group = hasattr(owner, "_tiles_at_rest")
        self.sampler = self.history = None
        self.pending = []                       # (cycle, time, dt) of the slots written since the last flush
        self.last_cycle, self.io_ns = -1, 0

    def _tiles(self):
        from .compare import _tiles_of
        return _tiles_of(self.owner)

    def start(self, gdt):
        try:
            self._start(gdt)
        except BaseException:
            self.close()                        # the rings do not outlive a refused start
            raise

    def _start(self, gdt):
        import time as _time
        from . import io
        p = self.params
        tiles = self._tiles()
        t0 = _time.perf_counter_ns()
        restarted = p.restart_from is not None
        path = history_path(p)
        scale = p.history_scale_exp
        self.sampler = Sampler(tiles, p.history_capacity, p.history_gauges, FIRST_SCALE if scale is None else scale)
        s = self.sampler
        kept = None
        if restarted and os.path.exists(path):
            kept = io.read_history_header(path)
            if scale is None:
                scale = tuple(kept["scale_exp"])
        if scale is None:
            s.enqueue(0)
            scale = default_scale(s.read(0, 1)[0][0])
        s.set_scale(scale)
        self.history = History(s.scale_exp, s.ds, s.global_nx, s.gauges, s.gauge_cells)
        os.makedirs(p.output_dir, exist_ok=True)
        if kept is not None:
            io.check_history_header(path, kept, self.history, p.global_grid)
            io.truncate_history_file(path, int(gdt.cycle))
        else:
            io.write_history_file(path, self.history, p.global_grid)
        self.io_ns += _time.perf_counter_ns() - t0
        if restarted:
            self.last_cycle = int(gdt.cycle)    # the run it continues wrote this row
        else:
            self.sample(gdt, 0.0)

    def sample(self, gdt, dt):
        if len(self.pending) == self.sampler.capacity:
            self.flush()
        if self.group:
            self.owner._tiles_at_rest()
        self.sampler.enqueue(len(self.pending))
        self.pending.append((int(gdt.cycle), float(gdt.time), float(dt)))
        self.last_cycle = int(gdt.cycle)

    def flush(self):
        import time as _time
        from . import io
        if not self.pending:
            return
        for params, _ in self.sampler.tiles:
            params.wait()                       # the cycles still queued are the run's own time, not the history's
        t0 = _time.perf_counter_ns()
        raw, values = self.sampler.read(0, len(self.pending))
        first = len(self.history)
        cycle, time, dt = zip(*self.pending)
        self.history.append(cycle, time, dt, raw, values)
        io.append_history_rows(history_path(self.params), self.history, first)
        self.pending = []
        self.io_ns += _time.perf_counter_ns() - t0

    def finish(self, gdt, dt):
        """The row of the cycle the run stopped at, unless it was sampled; the last flush; the rings are released."""
        try:
            if self.last_cycle != int(gdt.cycle):
                self.sample(gdt, dt)
            self.flush()
        finally:
            self.close()
        self.owner.history = self.history
        return self.history

    def close(self):
        if self.sampler is not None:
            self.sampler.close()
