"""Mixing measures of the passive scalars (csrc/mixing.hip): per scalar the exact profile of rho, φ, φ², ρφ, ρφ²
along x or y, and the histogram of φ with the exact mass of every bin, computed where the state lives. No reference
counterpart: the reference carries no scalars.

PER CELL at the global 0-based position ``(gx, gy)`` and per scalar plane k, all arithmetic in fp64 (fp32 values converted
first):

    bin     x: gx // width      y: gy // width      a cell with b >= nbins is skipped and counted nowhere
    terms   t0 = rho, t1 = phi, t2 = phi phi, t3 = rho phi, t4 = t3 phi
    Q_j     = round-half-even(t_j / 2^s_kj), an exact integer; a cell is BAD for plane k when rho, phi or a t_j is not finite or a
            |Q_j| >= 2^95: it adds 1 to that plane's n_bad and nothing else; the other planes are not affected
    limbs   as in profile.py; phi enters phi_min / phi_max through its order key

    PDF     bad when rho or phi is not finite or |Q(rho)| >= 2^95; else "below" when phi < lo; else
            fb = floor((phi - lo) inv_w), "above" when not fb < nbins, else bin int(fb); the row takes 1 and the limbs of Q(rho)

Every word of a record (20 words per (plane, bin), ``armon_mixing_bin``; 4 words per row of a histogram) merges by integer
addition, minimum or maximum, so a record is a function of the planes, the binning and the scale only, WORD FOR WORD.
``reference_record`` / ``reference_bounds`` / ``reference_pdf`` below restate the rules with numpy and Python ints; the tests hold
the kernels against them.

The integral width W and the mixedness Θ take φ as it is: they ASSUME a mixture fraction in [0, 1]. The second-order remap
overshoots slightly, so a sharp front gives bins whose φ̄(1 − φ̄) is a little below zero; ``minimum`` and
``maximum`` say by how much.
"""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

from ._lib import MixingSpec, PdfSpec, check, solver_error
from .profile import MASK, SCALE_LIMIT, default_scale, from_key, from_limbs, order_key, order_keys, quantise_limbs  # noqa: F401

AXES = {"x": 0, "y": 1}
TERMS = ("rho", "phi", "phi2", "rho_phi", "rho_phi2")
WORDS = 20
W_N, W_BAD, W_SUM, W_PHI_MIN, W_PHI_MAX = 0, 1, 2, 17, 18
MAX_SCALARS = 4
PDF_MAX_BINS = 1024
PDF_ROW = 4                 # words of a histogram row: count, three limbs


# ---- the rules, restated (the tests' oracle) -------------------------------------------------------------------------------
def cell_terms(rho, phi):
    """The five terms of cells (arrays of one shape; fp32 converted first) → list of fp64 arrays, one numpy operation per
    operation of the rule."""
    rho, phi = np.asarray(rho).astype(np.float64), np.asarray(phi).astype(np.float64)
    with np.errstate(all="ignore"):
        t3 = rho * phi
        return [rho, phi, phi * phi, t3, t3 * phi]


def _signed_limbs(t, s):
    """→ the three signed limbs of every Q as int64 arrays, and ok."""
    l0, l1, l2, ok = quantise_limbs(t, s)
    neg = np.signbit(t)
    return [np.where(neg, -l.astype(np.int64), l.astype(np.int64)) for l in (l0, l1, l2)], ok


def neutral(nbins):
    raw = np.zeros((int(nbins), WORDS), dtype=np.uint64)
    raw[:, W_PHI_MIN] = MASK
    return raw


def reference_record(axis, nbins, width, scale_exp, rho, phi, origin=(0, 0)):
    """The record of ONE plane: the 2-D arrays ``rho, phi`` whose first cell sits at global ``origin = (gx, gy)``, binned along
    ``axis`` → ``(nbins, 20)`` uint64. Integer arithmetic after the quantisation: numpy int64 sums of limbs below 2^32 (exact
    while a bin holds fewer than 2^31 cells), reduced bin by bin."""
    axis = AXES[axis] if isinstance(axis, str) else int(axis)
    rho, phi = np.asarray(rho), np.asarray(phi)
    ny, nx = rho.shape
    t = cell_terms(rho, phi)
    good = np.ones(rho.shape, dtype=bool)
    for a in t:
        good &= np.isfinite(a)
    limbs = []
    for j in range(5):
        l, ok = _signed_limbs(t[j], scale_exp[j])
        limbs.append(l)
        good &= ok
    along = (np.arange(nx, dtype=np.int64) + int(origin[0])) if axis == 0 else (np.arange(ny, dtype=np.int64) + int(origin[1]))
    b = along // int(width)                     # the bin of every column (x) or row (y)
    line = 0 if axis == 0 else 1                # the array axis that is summed first: whole columns or whole rows share a bin
    keys = order_keys(t[1])
    raw = neutral(nbins)
    cols = np.zeros((len(along), WORDS), dtype=np.int64)
    cols[:, W_N] = good.sum(axis=line)
    cols[:, W_BAD] = (~good).sum(axis=line)
    for j in range(5):
        for i in range(3):
            cols[:, W_SUM + 3 * j + i] = np.where(good, limbs[j][i], 0).sum(axis=line, dtype=np.int64)
    kmin = np.where(good, keys, np.uint64(MASK)).min(axis=line)
    kmax = np.where(good, keys, np.uint64(0)).max(axis=line)
    sel = b < nbins
    np.add.at(raw, (b[sel], slice(0, W_PHI_MIN)), cols[sel, :W_PHI_MIN].view(np.uint64))     # (unsigned: wraps like the device's integer adds)
    np.minimum.at(raw[:, W_PHI_MIN], b[sel], kmin[sel])
    np.maximum.at(raw[:, W_PHI_MAX], b[sel], kmax[sel])
    return raw


def reference_bounds(rho, phi):
    """The bounds pass of one plane: the bit patterns of the largest finite |t_j| → five ints."""
    out = []
    for a in cell_terms(rho, phi):
        a = np.abs(a[np.isfinite(a)])
        out.append(int(a.view(np.uint64).max()) if a.size else 0)
    return tuple(out)


def pdf_words(nbins):
    return (int(nbins) + 2) * PDF_ROW + 1


def reference_pdf(rho, phi, lo, inv_w, nbins, rho_scale_exp):
    """The histogram of one plane → ``4 (nbins + 2) + 1`` uint64 words: rows 0 .. nbins - 1 the bins, row nbins "below", row
    nbins + 1 "above", then the bad count."""
    rho, phi = np.asarray(rho).astype(np.float64).ravel(), np.asarray(phi).astype(np.float64).ravel()
    l, ok = _signed_limbs(rho, rho_scale_exp)
    good = ok & np.isfinite(phi)
    lo, inv_w = np.float64(lo), np.float64(inv_w)
    with np.errstate(all="ignore"):
        fb = np.floor((phi - lo) * inv_w)
    inside = good & ~(phi < lo) & (fb < nbins)
    row = np.where(phi < lo, nbins, np.where(inside, np.where(inside, fb, 0.).astype(np.int64), nbins + 1))
    out = np.zeros(pdf_words(nbins), dtype=np.uint64)
    table = np.zeros((nbins + 2, PDF_ROW), dtype=np.int64)
    np.add.at(table[:, 0], row[good], 1)
    for i in range(3):
        np.add.at(table[:, 1 + i], row[good], l[i][good])
    out[:-1] = table.view(np.uint64).ravel()
    out[-1] = int((~good).sum())
    return out


def merge_raw(x, y):
    """The merge of two ``(..., 20)`` records: sums add (mod 2^64, limb by limb), minimum and maximum of the keys."""
    out = x + y
    out[..., W_PHI_MIN] = np.minimum(x[..., W_PHI_MIN], y[..., W_PHI_MIN])
    out[..., W_PHI_MAX] = np.maximum(x[..., W_PHI_MAX], y[..., W_PHI_MAX])
    return out


def _once_rounded(q):
    """A Fraction (or None = undefined) → fp64, rounded once."""
    if q is None:
        return math.nan
    try:
        return float(q)
    except OverflowError:
        return math.copysign(math.inf, q)


# ---- the results -----------------------------------------------------------------------------------------------------------
class MixingProfile:
    """One scalar's record. ``raw``: the ``(nbins, 20)`` words; ``spec = (axis, nbins, width, dx, dy, N)`` with N the global
    cells along the axis; ``scale_exp``: the five exponents; decoded: ``n``, ``n_bad``, ``sums[j][b]`` (exact Python ints in
    quanta ``2^scale_exp[j]``), ``coord`` (bin centres), and per bin — fp64, each rounded once from the exact rational, NaN where
    the bin is empty — ``phi = S1/n``, ``phi_favre = S3/S0``, ``variance = S2/n − (S1/n)²``,
    ``favre_variance = S4/S0 − (S3/S0)²``, ``rho = S0/n``, ``phi_min``, ``phi_max``. Whole-record measures, each from exact
    rationals and rounded once, with ℓ_b = (cell rows of bin b) × (cell size along the axis): ``content = Σ S3_b dx dy``,
    ``integral_width W = Σ φ̄_b (1 − φ̄_b) ℓ_b``, ``mixedness Θ = Σ ((S1_b − S2_b)/n_b) ℓ_b / W`` (Youngs' molecular-mix
    parameter; NaN when W = 0), ``extent(lo, hi)``, ``minimum``, ``maximum``. W and Θ assume a mixture fraction in [0, 1]."""

    COLUMNS = ("coord", "n", "rho", "phi", "phi_favre", "variance", "favre_variance", "phi_min", "phi_max")

    def __init__(self, raw, spec, scale_exp, name="", origin=(0., 0.), cycle=0, time=0.0):
        self.raw = np.ascontiguousarray(raw, dtype=np.uint64).reshape(-1, WORDS)
        self.spec, self.scale_exp = tuple(spec), tuple(int(s) for s in scale_exp)
        self.name, self.origin, self.cycle, self.time = str(name), tuple(float(o) for o in origin), int(cycle), float(time)
        assert self.raw.shape[0] == self.nbins and len(self.scale_exp) == 5
        self._decoded = {}

    axis = property(lambda self: "xy"[self.spec[0]])
    nbins = property(lambda self: self.spec[1])
    width = property(lambda self: self.spec[2])
    n = property(lambda self: self.raw[:, W_N].copy())
    n_bad = property(lambda self: self.raw[:, W_BAD].copy())

    def _once(self, name, make):
        if name not in self._decoded:
            self._decoded[name] = make()
        return self._decoded[name]

    sums = property(lambda self: self._once("sums", self._sums))

    def _sums(self):
        signed = self.raw[:, W_SUM:W_SUM + 15].view(np.int64).reshape(-1, 5, 3).tolist()
        return [[from_limbs(row[j]) for row in signed] for j in range(5)]

    def _exact(self):
        """Per bin the exact rationals S0 .. S4 (values, not quanta) and n."""
        scale = [Fraction(2) ** s for s in self.scale_exp]
        S = self.sums
        return [[S[j][b] * scale[j] for j in range(5)] for b in range(self.nbins)], self.raw[:, W_N].tolist()

    @property
    def cell(self):
        """The cell size along the axis."""
        return self.spec[3 + self.spec[0]]

    def lengths(self):
        """ℓ_b as exact rationals: the cell rows of bin b (the last bin may be cut by the domain) times the cell size."""
        N, w, d = self.spec[5], self.width, Fraction(self.cell)
        return [max(0, min(w, N - b * w)) * d for b in range(self.nbins)]

    def _means(self):
        S, n = self._once("exact", self._exact)
        out = {k: [] for k in ("rho", "phi", "phi_favre", "variance", "favre_variance")}
        for b in range(self.nbins):
            s, m = S[b], n[b]
            out["rho"].append(_once_rounded(s[0] / m if m else None))
            out["phi"].append(_once_rounded(s[1] / m if m else None))
            out["variance"].append(_once_rounded(s[2] / m - (s[1] / m) ** 2 if m else None))
            fav = m and s[0] != 0
            out["phi_favre"].append(_once_rounded(s[3] / s[0] if fav else None))
            out["favre_variance"].append(_once_rounded(s[4] / s[0] - (s[3] / s[0]) ** 2 if fav else None))
        has = self.raw[:, W_N] != 0
        for name, w in (("phi_min", W_PHI_MIN), ("phi_max", W_PHI_MAX)):
            out[name] = [from_key(int(k)) if o else math.nan for k, o in zip(self.raw[:, w], has)]
        return {k: np.array(v, dtype=np.float64) for k, v in out.items()}

    def __getattr__(self, name):
        if name in ("rho", "phi", "phi_favre", "variance", "favre_variance", "phi_min", "phi_max"):
            return self._once("means", self._means)[name]
        raise AttributeError(name)

    @property
    def coord(self):
        ax = self.spec[0]
        return self.origin[ax] + (np.arange(self.nbins, dtype=np.float64) + 0.5) * self.width * self.cell

    def _edge(self, cells):
        return float(Fraction(self.origin[self.spec[0]]) + cells * Fraction(self.cell))

    # the whole-record measures
    def _content(self):
        S, _ = self._once("exact", self._exact)
        return sum((s[3] for s in S), Fraction(0)) * Fraction(self.spec[3]) * Fraction(self.spec[4])

    def _width_exact(self):
        S, n = self._once("exact", self._exact)
        W = Fraction(0)
        for b, l in enumerate(self.lengths()):
            if n[b]:
                m = S[b][1] / n[b]
                W += m * (1 - m) * l
        return W

    content = property(lambda self: _once_rounded(self._content()))
    integral_width = property(lambda self: _once_rounded(self._width_exact()))

    @property
    def mixedness(self):
        S, n = self._once("exact", self._exact)
        W = self._width_exact()
        if W == 0:
            return math.nan
        top = sum(((S[b][1] - S[b][2]) / n[b] * l for b, l in enumerate(self.lengths()) if n[b]), Fraction(0))
        return _once_rounded(top / W)

    def extent(self, lo=0.01, hi=0.99):
        """The lower edge of the first bin and the upper edge of the last bin with ``lo <= φ̄_b <= hi`` (exact comparisons), or
        None when no bin qualifies."""
        S, n = self._once("exact", self._exact)
        lo, hi = Fraction(lo), Fraction(hi)
        inside = [b for b in range(self.nbins) if n[b] and lo <= S[b][1] / n[b] <= hi]
        if not inside:
            return None
        return self._edge(inside[0] * self.width), self._edge(min((inside[-1] + 1) * self.width, self.spec[5]))

    @property
    def minimum(self):
        keys = self.raw[self.raw[:, W_N] != 0, W_PHI_MIN]
        return from_key(int(keys.min())) if keys.size else math.nan

    @property
    def maximum(self):
        keys = self.raw[self.raw[:, W_N] != 0, W_PHI_MAX]
        return from_key(int(keys.max())) if keys.size else math.nan

    def measures(self):
        """What one line of the time series holds for this scalar → dict."""
        ext = self.extent()
        return {"content": self.content, "min": self.minimum, "max": self.maximum, "width": self.integral_width,
                "mixedness": self.mixedness, "extent_lo": math.nan if ext is None else ext[0],
                "extent_hi": math.nan if ext is None else ext[1]}

    def table(self):
        """Everything this scalar's block of a mixing file holds → dict (``io.read_mixing_file`` returns the same)."""
        t = {"name": self.name, "axis": self.axis, "width": self.width, "cycle": self.cycle, "time": self.time,
             "coord": self.coord, "n": self.n}
        t.update(self._once("means", self._means))
        return t

    def _same(self, other):
        return (self.spec, self.scale_exp, self.origin, self.name) == (other.spec, other.scale_exp, other.origin, other.name)

    def merge(self, other):
        if not self._same(other):
            solver_error("config", f"mixing profiles of another scalar, binning or scale do not merge: {self.name!r}, {self.spec}, "
                                   f"{self.scale_exp} against {other.name!r}, {other.spec}, {other.scale_exp}")
        return MixingProfile(merge_raw(self.raw, other.raw), self.spec, self.scale_exp, self.name, self.origin, self.cycle, self.time)

    def __eq__(self, other):
        return isinstance(other, MixingProfile) and self._same(other) and np.array_equal(self.raw, other.raw)

    def report(self):
        t, m = self.table(), self.measures()
        lines = [f"Mixing of {self.name!r} along {self.axis} (width {self.width}), {self.nbins} bins, {int(self.raw[:, W_N].sum())} cells, "
                 f"{int(self.raw[:, W_BAD].sum())} bad, quanta 2^{list(self.scale_exp)}",
                 f"  content = {m['content']:.12g}  min = {m['min']:.6g}  max = {m['max']:.6g}  W = {m['width']:.6g}  "
                 f"Theta = {m['mixedness']:.6g}  extent = {self.extent()}"]
        for b in range(self.nbins):
            lines.append(f"  {t['coord'][b]:12.5g}  n = {int(t['n'][b]):9d}  phi = {t['phi'][b]:12.5g}  favre = {t['phi_favre'][b]:12.5g}  "
                         f"var = {t['variance'][b]:12.5g}  min = {t['phi_min'][b]:12.5g}  max = {t['phi_max'][b]:12.5g}")
        return "\n".join(lines)

    def __repr__(self):
        return f"MixingProfile({self.name!r}, {self.axis}, nbins={self.nbins}, scale_exp={self.scale_exp}, cycle={self.cycle})"


class ScalarPDF:
    """The histogram of one scalar. ``raw``: the ``4 (nbins + 2) + 1`` words; ``lo, hi``: the range; ``counts`` (uint64 per bin),
    ``mass_sums`` (exact Python ints in quanta ``2^rho_scale_exp``), ``mass`` (fp64: Σ rho of the bin, rounded once; times
    dx dy it is the mass), ``below`` / ``above``: ``(count, mass)`` of the cells outside the range, ``bad``, ``edges``
    (``nbins + 1`` values ``lo + i (hi − lo) / nbins``; the bin a cell falls into is decided by the rule, with
    ``inv_w = nbins / (hi − lo)``) and ``density()``."""

    def __init__(self, raw, lo, hi, nbins, rho_scale_exp, name="", cycle=0, time=0.0):
        self.raw = np.ascontiguousarray(raw, dtype=np.uint64).ravel()
        self.lo, self.hi, self.nbins, self.rho_scale_exp = float(lo), float(hi), int(nbins), int(rho_scale_exp)
        self.name, self.cycle, self.time = str(name), int(cycle), float(time)
        assert self.raw.size == pdf_words(self.nbins)

    inv_w = property(lambda self: inv_width(self.lo, self.hi, self.nbins))
    rows = property(lambda self: self.raw[:-1].reshape(self.nbins + 2, PDF_ROW))
    counts = property(lambda self: self.rows[:self.nbins, 0].copy())
    bad = property(lambda self: int(self.raw[-1]))

    def _mass_sum(self, row):
        return from_limbs(self.rows[row, 1:].view(np.int64).tolist())

    @property
    def mass_sums(self):
        return [self._mass_sum(b) for b in range(self.nbins)]

    def _mass(self, row):
        return _once_rounded(self._mass_sum(row) * Fraction(2) ** self.rho_scale_exp)

    @property
    def mass(self):
        return np.array([self._mass(b) for b in range(self.nbins)], dtype=np.float64)

    below = property(lambda self: (int(self.rows[self.nbins, 0]), self._mass(self.nbins)))
    above = property(lambda self: (int(self.rows[self.nbins + 1, 0]), self._mass(self.nbins + 1)))

    @property
    def edges(self):
        return self.lo + np.arange(self.nbins + 1, dtype=np.float64) * (self.hi - self.lo) / self.nbins

    def density(self, weight="count"):
        """The bins as a probability density over the range: ``weight`` = ``"count"`` or ``"mass"``, normalised by the cells
        (or mass) INSIDE the range so that ``Σ density · (hi − lo) / nbins = 1``; NaN when the range holds nothing."""
        v = self.counts.astype(np.float64) if weight == "count" else self.mass
        total = v.sum()
        return v / (total * (self.hi - self.lo) / self.nbins) if total != 0 else np.full(self.nbins, math.nan)

    def _same(self, other):
        return (self.lo, self.hi, self.nbins, self.rho_scale_exp, self.name) == (other.lo, other.hi, other.nbins, other.rho_scale_exp, other.name)

    def merge(self, other):
        if not self._same(other):
            solver_error("config", f"histograms of another scalar, range or scale do not merge: {self!r} against {other!r}")
        return ScalarPDF(self.raw + other.raw, self.lo, self.hi, self.nbins, self.rho_scale_exp, self.name, self.cycle, self.time)

    def __eq__(self, other):
        return isinstance(other, ScalarPDF) and self._same(other) and np.array_equal(self.raw, other.raw)

    def table(self):
        return {"name": self.name, "lo": self.lo, "hi": self.hi, "nbins": self.nbins, "bad": self.bad, "below": self.below,
                "above": self.above, "edges": self.edges, "counts": self.counts, "mass": self.mass}

    def __repr__(self):
        return f"ScalarPDF({self.name!r}, [{self.lo}, {self.hi}), nbins={self.nbins}, rho_scale_exp={self.rho_scale_exp})"


# ---- device side -----------------------------------------------------------------------------------------------------------
def inv_width(lo, hi, nbins):
    """``inv_w`` of the rule: ``nbins / (hi − lo)``, one fp64 division."""
    return float(np.float64(nbins) / (np.float64(hi) - np.float64(lo)))


def make_spec(p0, axis, width=1, bins=None):
    """The binning of the global domain of ``p0`` → the tuple ``MixingProfile.spec`` holds. ``bins``: how many (default: all of
    the axis); fewer cut the far cells off."""
    if axis not in AXES:
        solver_error("config", f"unknown mixing axis {axis!r}: 'x' or 'y'")
    if isinstance(width, bool) or int(width) != width or width < 1:
        solver_error("config", f"mixing width must be an integer >= 1, got {width!r}")
    N = int(p0.global_grid[AXES[axis]])
    if bins is None:
        bins = -(-N // int(width))
    if isinstance(bins, bool) or int(bins) != bins or bins < 1:
        solver_error("config", f"mixing bins must be an integer >= 1, got {bins!r}")
    return (AXES[axis], int(bins), int(width), float(p0.cell_size(0)), float(p0.cell_size(1)), N)


def _names(p0, scalars):
    names = tuple(p0.scalar_names) if scalars is None else ((scalars,) if isinstance(scalars, str) else tuple(scalars))
    if not p0.scalar_names:
        solver_error("config", "mixing measures need passive scalars: this run carries none")
    for s in names:
        if s not in p0.scalar_names:
            solver_error("config", f"no scalar {s!r}: this run carries {p0.scalar_names}")
    if not 1 <= len(names) <= MAX_SCALARS or len(set(names)) != len(names):
        solver_error("config", f"mixing takes 1 to {MAX_SCALARS} distinct scalars, got {names!r}")
    return names


def _window(params, windows, i):
    return windows[i] if windows else (0, 0, params.N[0], params.N[1])


def _geometry(params, grid, window):
    col0, row0, wnx, wny = window
    return (params.device.ctx, grid.size.size[0], grid.size.ghosts, params.N[0], params.N[1]), (col0, row0, wnx, wny)


def _call_mixing(name, params, grid, names, window, c_spec, out):
    from .problem import SCALAR_PREFIX
    head, win = _geometry(params, grid, window)
    phi = (C.c_void_p * len(names))(*[grid.data[SCALAR_PREFIX + s].ptr for s in names])
    check(params.fn(name)(*head, C.c_void_p(grid.data["rho"].ptr), len(names), phi, *win,
                          params.N_origin[0] - 1 + win[0], params.N_origin[1] - 1 + win[1], C.byref(c_spec), C.c_void_p(out.ptr)))


def _c_spec(spec, scales):
    s = MixingSpec()
    s.axis, s.nbins, s.width = spec[0], spec[1], spec[2]
    for k, sc in enumerate(scales):
        s.scale_exp[k][:] = list(sc)
    return s


def state_bounds(tiles, spec, names, windows=None):
    """The bounds pass over every tile → per scalar the five bit patterns, merged by maximum."""
    c_spec, outs, ns = _c_spec(spec, ()), [], len(names)
    try:
        for i, (params, grid) in enumerate(tiles):
            outs.append(params.device.zeros(5 * ns, np.uint64))
            _call_mixing("mixing_bounds", params, grid, names, _window(params, windows, i), c_spec, outs[-1])
        top = np.zeros(5 * ns, dtype=np.uint64)
        for (params, _), out in zip(tiles, outs):
            params.wait()
            top = np.maximum(top, out.to_host())
    finally:
        for out in outs:
            out.free()
    return [tuple(int(v) for v in top[5 * k:5 * k + 5]) for k in range(ns)]


def _check_scales(scale_exp, names):
    if isinstance(scale_exp, dict):
        scale_exp = [scale_exp.get(s) for s in names]
    try:
        scales = [tuple(int(v) for v in sc) for sc in scale_exp]
        good = len(scales) == len(names) and all(len(sc) == 5 and all(abs(v) <= SCALE_LIMIT for v in sc) for sc in scales)
    except (TypeError, ValueError):
        good = False
    if not good:
        solver_error("config", f"scale_exp takes five exponents within ±{SCALE_LIMIT} per scalar (a list in the order of the scalars, "
                               f"or a dict name -> five), got {scale_exp!r}")
    return scales


def mixing_state(tiles, axis="y", width=1, scalars=None, scale_exp=None, windows=None, bins=None):
    """The mixing profiles of the scalars held by the ``(params, grid)`` of ``tiles`` (idle) → dict name → ``MixingProfile``.
    ``axis``: ``"x" | "y"``; ``width``: cells per bin; ``scalars``: the names (default all); ``scale_exp``: per scalar five
    exponents instead of the default scale ``s = e − 94`` (then no bounds pass runs); ``windows``: per tile the
    ``(col0, row0, wnx, wny)`` of its real cells to take instead of all; ``bins``: fewer bins than the axis holds. Each tile runs the bounds pass, the bounds merge by
    maximum BEFORE any main pass so that every tile uses the same quanta, then each tile's records are read back and merged."""
    p0 = tiles[0][0]
    names = _names(p0, scalars)
    spec = make_spec(p0, axis, width, bins)
    scales = [default_scale(b) for b in state_bounds(tiles, spec, names, windows)] if scale_exp is None else _check_scales(scale_exp, names)
    c_spec, nbins, ns, outs = _c_spec(spec, scales), spec[1], len(names), []
    try:
        for i, (params, grid) in enumerate(tiles):
            outs.append(params.device.empty(ns * nbins * WORDS, np.uint64))
            check(params.device._L.armon_hip_mixing_reset(params.device.ctx, ns, nbins, C.c_void_p(outs[-1].ptr)))
            _call_mixing("mixing", params, grid, names, _window(params, windows, i), c_spec, outs[-1])
        raw = np.stack([neutral(nbins)] * ns)
        for (params, _), out in zip(tiles, outs):
            params.wait()
            raw = merge_raw(raw, out.to_host().reshape(ns, nbins, WORDS))
    finally:
        for out in outs:
            out.free()
    return {s: MixingProfile(raw[k], spec, scales[k], s, p0.origin) for k, s in enumerate(names)}


def pdf_state(tiles, name, bins=64, range=(0., 1.), rho_scale_exp=None, windows=None):
    """The histogram of the scalar ``name`` over the tiles → ``ScalarPDF``. ``bins``: 1 .. 1024 equal bins of
    ``range = (lo, hi)``; ``rho_scale_exp``: the quantum of the mass sums instead of the default (``s = e − 94`` from the
    bounds pass of rho)."""
    from .problem import SCALAR_PREFIX
    p0 = tiles[0][0]
    (name,) = _names(p0, (name,))
    if isinstance(bins, bool) or int(bins) != bins or not 1 <= bins <= PDF_MAX_BINS:
        solver_error("config", f"pdf bins must be an integer in [1, {PDF_MAX_BINS}], got {bins!r}")
    try:
        lo, hi = float(range[0]), float(range[1])
        good = len(range) == 2 and math.isfinite(lo) and math.isfinite(hi) and lo < hi and math.isfinite(inv_width(lo, hi, bins))
    except (TypeError, ValueError, IndexError):
        good = False
    if not good:
        solver_error("config", f"pdf range takes two finite values lo < hi, got {range!r}")
    bins = int(bins)
    if rho_scale_exp is None:
        rho_scale_exp = default_scale(state_bounds(tiles, make_spec(p0, "y"), (name,), windows)[0])[0]
    if isinstance(rho_scale_exp, bool) or int(rho_scale_exp) != rho_scale_exp or abs(rho_scale_exp) > SCALE_LIMIT:
        solver_error("config", f"rho_scale_exp takes an exponent within ±{SCALE_LIMIT}, got {rho_scale_exp!r}")
    s = PdfSpec()
    s.lo, s.inv_w, s.nbins, s.rho_scale_exp = lo, inv_width(lo, hi, bins), bins, int(rho_scale_exp)
    outs = []
    try:
        for i, (params, grid) in enumerate(tiles):
            outs.append(params.device.empty(pdf_words(bins), np.uint64))
            check(params.device._L.armon_hip_scalar_pdf_reset(params.device.ctx, bins, C.c_void_p(outs[-1].ptr)))
            head, win = _geometry(params, grid, _window(params, windows, i))
            check(params.fn("scalar_pdf")(*head, C.c_void_p(grid.data["rho"].ptr), C.c_void_p(grid.data[SCALAR_PREFIX + name].ptr), *win,
                                          C.byref(s), C.c_void_p(outs[-1].ptr)))
        raw = np.zeros(pdf_words(bins), dtype=np.uint64)
        for (params, _), out in zip(tiles, outs):
            params.wait()
            raw = raw + out.to_host()
    finally:
        for out in outs:
            out.free()
    return ScalarPDF(raw, lo, hi, bins, rho_scale_exp, name)


# ---- the run options (mixing_step, mixing_axis, ..., mixing_at_end) --------------------------------------------------------
def mixing_path(params, cycle=None):
    """The file of one sample, or (``cycle`` None) of the time series."""
    tail = "" if cycle is None else f"_{cycle:06d}"
    return os.path.join(params.output_dir, f"{params.mixing_file}{tail}.txt")


def mixing_run(grid, params, gdt):
    """The mixing sample of the lone block ``grid`` after ``gdt.cycle`` completed cycles: appended to ``grid.mixing_samples``,
    written to ``mixing_path(params, cycle)``, and the time series ``mixing_path(params)`` rewritten with one line per
    sample. Synchronous."""
    from .io import write_mixing_file, write_mixing_series
    tiles = [(params, grid)]
    names = params.mixing_scalars
    profiles = mixing_state(tiles, params.mixing_axis, width=params.mixing_bin_width, scalars=names)
    pdfs = None
    if params.mixing_pdf_bins:
        pdfs = {s: pdf_state(tiles, s, bins=params.mixing_pdf_bins, range=params.mixing_pdf_range) for s in profiles}
    for r in list(profiles.values()) + list((pdfs or {}).values()):
        r.cycle, r.time = int(gdt.cycle), float(gdt.time)
    sample = (int(gdt.cycle), float(gdt.time), profiles, pdfs)
    grid.mixing_samples.append(sample)
    os.makedirs(params.output_dir, exist_ok=True)
    write_mixing_file(mixing_path(params, gdt.cycle), profiles, pdfs, params.output_precision)
    write_mixing_series(mixing_path(params), grid.mixing_samples, params.output_precision)
    return sample
