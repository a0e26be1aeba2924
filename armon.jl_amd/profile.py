"""In-situ profiles (csrc/profile.hip): the state binned along x, along y or by the distance from a centre, and summed EXACTLY
where it lives. No reference counterpart: the reference writes whole fields (ref src/io.jl:37-81).

PER CELL at the global 0-based position ``(gx, gy)``, all arithmetic in fp64 (fp32 values converted first):

    bin     x: gx // width      y: gy // width
            r: rx = ((gx + 0.5) - cx) dx, ry likewise, rr = sqrt(rx rx + ry ry), b = floor(rr inv_dr)
            a cell with b >= nbins is skipped and counted nowhere
    un, ut  x: u, v     y: v, u     r: (u rx + v ry) / rr, (v rx - u ry) / rr, both 0 where rr == 0
    terms   rho, rho un, rho ut, rho E, p   (p = the EOS of the cell in the data type, converted)
    Q_k     = round-half-even(t_k / 2^s_k), an exact integer; a cell is BAD when one of rho, u, v, E, t_k is not finite or a
            |Q_k| >= 2^95: it adds 1 to n_bad and nothing else
    limbs   a = |Q_k| → a & 0xffffffff, (a >> 32) & 0xffffffff, a >> 64, negated when Q_k < 0, each added to its own int64

Every addend is rounded once, on its own, to a fixed-point integer; everything after that is integer addition, a minimum or
a maximum. So the record of a bin (24 words, ``armon_profile_bin``) is a function of the state, the binning and the scale
only, and the records of the tiles of a group merge to the single block's WORD FOR WORD — which floating-point sums cannot
give for a radius, whose bins cut across rows, tiles and waves. The default scale ``s_k = e_k - 94``, ``max |t_k| < 2^e_k``
over the whole domain, keeps every |Q_k| below 2^94 and the quantum 2^-41 of the largest term's last bit or finer. No limb
overflows while fewer than 2^31 cells are merged into one bin. ``quantise`` / ``limbs`` / ``cell_terms`` /
``reference_record`` below restate the rule in Python; the tests hold the kernel against them.
"""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

from ._lib import ProfileSpec, check, solver_error

KINDS = {"x": 0, "y": 1, "r": 2}
TERMS = ("rho", "rho_un", "rho_ut", "rho_E", "p")
WORDS = 24
W_N, W_BAD, W_SUM, W_RHO_MIN, W_RHO_MAX, W_P_MIN, W_P_MAX = 0, 1, 2, 17, 18, 19, 20
MASK = (1 << 64) - 1
EDGE = 1 << 95
SCALE_LIMIT = 4096          # |s_k| the library accepts


# ---- the rule, in Python (the tests' oracle) -------------------------------------------------------------------------------
def quantise(t, s):
    """round-half-even(t / 2^s) as a Python int, or None when ``t`` is not finite or the result reaches 2^95 in magnitude."""
    t = float(t)
    if not math.isfinite(t):
        return None
    m, e = math.frexp(t)
    M = int(m * 9007199254740992.0)             # exact: t = M 2^(e - 53), |M| < 2^53
    sh = e - 53 - int(s)
    if M == 0:
        return 0
    if sh >= 0:
        if sh > 160:
            return None
        Q = M << sh
    else:
        a, r = abs(M), -sh
        if r > 64:
            return 0
        q, rem = a >> r, a & ((1 << r) - 1)
        half = 1 << (r - 1)
        if rem > half or (rem == half and q & 1):
            q += 1
        Q = -q if M < 0 else q
    return None if abs(Q) >= EDGE else Q


def limbs(Q):
    """The three signed limbs of ``Q``: their value ``l0 + l1 2^32 + l2 2^64`` is ``Q``."""
    a = abs(Q)
    l = (a & 0xffffffff, (a >> 32) & 0xffffffff, a >> 64)
    return tuple(-v for v in l) if Q < 0 else l


def quantise_limbs(t, s):
    """``quantise`` and ``limbs`` on a whole fp64 array → ``(l0, l1, l2, ok)``: the three limbs of |Q| as uint64
    arrays, ok = False where the value is not finite or |Q| >= 2^95."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    b = t.view(np.uint64)
    one, m32 = np.uint64(1), np.uint64(0xffffffff)
    ef = ((b >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    frac = b & np.uint64((1 << 52) - 1)
    m = np.where(ef > 0, frac | np.uint64(1 << 52), frac)
    sh = np.where(ef > 0, ef, 1) - 1075 - int(s)
    ok = ef != 0x7ff
    live = ok & (m != 0)
    words = np.zeros((5,) + t.shape, dtype=np.uint64)
    down = live & (sh < 0)
    r = np.minimum(np.where(down, -sh, 1), 63).astype(np.uint64)      # (a shift by 64 or more rounds to 0, as a shift by 63 does)
    q, rem, half = m >> r, m & ((one << r) - one), one << (r - one)
    q = q + ((rem > half) | ((rem == half) & ((q & one) != 0))).astype(np.uint64)
    words[0] = np.where(down, q & m32, 0)
    words[1] = np.where(down, q >> np.uint64(32), 0)
    up = live & (sh >= 0)
    far = up & (sh >= 95)
    w, bit = np.where(up & ~far, sh // 32, -1), (np.where(up, sh, 0) % 32).astype(np.uint64)
    lo, hi = (m & m32) << bit, (m >> np.uint64(32)) << bit               # both below 2^64; their bits do not overlap once placed
    for k in range(3):
        sel = w == k
        words[k] += np.where(sel, lo & m32, 0)
        words[k + 1] += np.where(sel, (lo >> np.uint64(32)) + (hi & m32), 0)
        words[k + 2] += np.where(sel, hi >> np.uint64(32), 0)
    ok = ok & ~far & (words[3] == 0) & (words[4] == 0) & (words[2] < np.uint64(1 << 31))
    return words[0], words[1], words[2], ok


def from_limbs(l):
    return l[0] + (l[1] << 32) + (l[2] << 64)


def order_key(x):
    """The order key of an fp64 value: unsigned order = numerical order, -0.0 below +0.0."""
    b = int(np.array([x], dtype=np.float64).view(np.uint64)[0])
    return (b ^ MASK) if b >> 63 else (b ^ (1 << 63))


def order_keys(a):
    """``order_key`` for a whole array (converted to fp64 first) → uint64 array of the same shape."""
    bits = np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ np.uint64(1 << 63))


def from_key(k):
    b = (k ^ (1 << 63)) if k >> 63 else (k ^ MASK)
    return float(np.array([b], dtype=np.uint64).view(np.float64)[0])


def cell_terms(kind, rho, u, v, E, p, gx, gy, width=1, cx=0.0, cy=0.0, dx=1.0, dy=1.0, inv_dr=1.0):
    """The bin and the five terms of cells (scalars or numpy arrays of one shape; fp32 inputs are converted first, ``p`` may be
    None) at the global positions ``gx, gy`` → ``(b, [t0 .. t4])`` as int64 / fp64 arrays. One numpy operation per operation of
    the rule: numpy's fp64 +, -, *, / and sqrt are the IEEE ones."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    rho, u, v, E = (np.asarray(a).astype(np.float64) for a in (rho, u, v, E))
    gx, gy, _ = np.broadcast_arrays(np.asarray(gx, dtype=np.int64), np.asarray(gy, dtype=np.int64), rho)
    with np.errstate(all="ignore"):
        if kind == 0:
            b, un, ut = gx // width, u, v
        elif kind == 1:
            b, un, ut = gy // width, v, u
        else:
            rx = ((gx.astype(np.float64) + 0.5) - np.float64(cx)) * np.float64(dx)
            ry = ((gy.astype(np.float64) + 0.5) - np.float64(cy)) * np.float64(dy)
            rr = np.sqrt(rx * rx + ry * ry)
            fb = np.floor(rr * np.float64(inv_dr))
            b = np.where(fb < 2.0 ** 62, fb, 2.0 ** 62).astype(np.int64)
            safe = np.where(rr == 0., 1., rr)
            un = np.where(rr == 0., 0., (u * rx + v * ry) / safe)
            ut = np.where(rr == 0., 0., (v * rx - u * ry) / safe)
        t = [rho, rho * un, rho * ut, rho * E, np.zeros_like(rho) if p is None else np.asarray(p).astype(np.float64)]
    return np.asarray(b, dtype=np.int64), t


def neutral(nbins):
    raw = np.zeros((int(nbins), WORDS), dtype=np.uint64)
    raw[:, (W_RHO_MIN, W_P_MIN)] = MASK
    return raw


def reference_record(kind, nbins, scale_exp, rho, u, v, E, p, origin=(0, 0), skip=None, **geometry):
    """The record of the 2-D arrays ``rho, u, v, E`` (+ ``p``, or None) whose first cell sits at global ``origin = (gx, gy)``,
    built cell by cell with ``cell_terms`` / ``quantise`` / ``limbs`` → ``(nbins, 24)`` uint64. ``skip``: a boolean array of
    cells to leave out altogether."""
    ny, nx = np.shape(rho)
    gx = np.arange(nx, dtype=np.int64)[None, :] + int(origin[0])
    gy = np.arange(ny, dtype=np.int64)[:, None] + int(origin[1])
    b, t = cell_terms(kind, rho, u, v, E, p, gx, gy, **geometry)
    nterms = 4 if p is None else 5
    fields = [np.asarray(a).astype(np.float64).ravel() for a in (rho, u, v, E)]
    finite = np.ones(nx * ny, dtype=bool)
    for a in fields + [a.ravel() for a in t]:
        finite &= np.isfinite(a)
    key_of = {W_RHO_MIN: order_keys(t[0]).ravel().tolist(), W_P_MIN: order_keys(t[4]).ravel().tolist()}
    b, t = b.ravel(), [a.ravel().tolist() for a in t]
    words = [[0] * WORDS for _ in range(nbins)]
    for w in words:
        w[W_RHO_MIN] = w[W_P_MIN] = MASK
    keep = np.ones(nx * ny, dtype=bool) if skip is None else ~np.asarray(skip).ravel()
    for i in np.flatnonzero((b < nbins) & keep):
        w = words[b[i]]
        Q = [quantise(t[k][i], scale_exp[k]) for k in range(nterms)] if finite[i] else [None]
        if any(q is None for q in Q):
            w[W_BAD] += 1
            continue
        w[W_N] += 1
        for k in range(nterms):
            for j, l in enumerate(limbs(Q[k])):
                w[W_SUM + 3 * k + j] += l
        for lo, hi in ((W_RHO_MIN, W_RHO_MAX),) + (((W_P_MIN, W_P_MAX),) if nterms == 5 else ()):
            key = key_of[lo][i]
            w[lo], w[hi] = min(w[lo], key), max(w[hi], key)
    return np.array([[x & MASK for x in w] for w in words], dtype=np.uint64).reshape(nbins, WORDS)


def merge_raw(x, y):
    """The merge of two ``(nbins, 24)`` records: sums add (mod 2^64, limb by limb), minima and maxima of the keys."""
    out = x + y                                 # (unsigned: wraps like the device's integer adds)
    for w in (W_RHO_MIN, W_P_MIN):
        out[:, w] = np.minimum(x[:, w], y[:, w])
    for w in (W_RHO_MAX, W_P_MAX):
        out[:, w] = np.maximum(x[:, w], y[:, w])
    return out


def default_scale(bounds):
    """``s_k = e_k - 94`` with ``max |t_k| < 2^e_k`` (the frexp exponent), ``e_k = 0`` when the maximum is 0; ``bounds`` = the
    five bit patterns of the bounds pass."""
    top = np.array([int(v) for v in bounds], dtype=np.uint64).view(np.float64)
    return tuple((math.frexp(float(v))[1] if v != 0 else 0) - 94 for v in top)


# ---- the result ------------------------------------------------------------------------------------------------------------
class Profile:
    """``raw``: the ``(nbins, 24)`` words; ``spec``: what the bins are (kind, eos, nbins, width, cx, cy, dx, dy, inv_dr, gamma) and
    ``scale_exp``; decoded: ``n``, ``n_bad``, ``sums[k][b]`` (exact Python ints, in quanta ``2^scale_exp[k]``), the means
    ``rho = S0/n, un = S1/S0, ut = S2/S0, E = S3/S0, p = S4/n`` (the conventions of ``coarsen``; fp64, each rounded once from
    the exact rational; NaN where the bin is empty), the extrema ``rho_min .. p_max``, ``coord`` (the bin centres: physical x,
    y or radius) and ``cycle``, ``time`` when the profile was taken by a run."""

    def __init__(self, raw, spec, scale_exp, origin=(0., 0.), cycle=0, time=0.0):
        self.raw = np.ascontiguousarray(raw, dtype=np.uint64).reshape(-1, WORDS)
        self.spec, self.scale_exp = tuple(spec), tuple(int(s) for s in scale_exp)
        self.origin, self.cycle, self.time = tuple(float(o) for o in origin), int(cycle), float(time)
        assert self.raw.shape[0] == self.nbins
        self._decoded = {}                          # the sums, means and extrema, decoded on first use (``raw`` is not to be written to)

    kind = property(lambda self: "xyr"[self.spec[0]])
    with_p = property(lambda self: self.spec[1] >= 0)
    nbins = property(lambda self: self.spec[2])
    width = property(lambda self: self.spec[3])
    n = property(lambda self: self.raw[:, W_N].copy())
    n_bad = property(lambda self: self.raw[:, W_BAD].copy())

    @property
    def dr(self):
        return 1.0 / self.spec[8]

    @property
    def centre(self):
        """R: the centre in physical coordinates."""
        return (self.origin[0] + self.spec[4] * self.spec[6], self.origin[1] + self.spec[5] * self.spec[7])

    def _once(self, name, make):
        if name not in self._decoded:
            self._decoded[name] = make()
        return self._decoded[name]

    sums = property(lambda self: self._once("sums", self._sums))

    def _sums(self):
        signed = self.raw[:, W_SUM:W_SUM + 15].view(np.int64).reshape(-1, 5, 3).tolist()
        return [[from_limbs(row[k]) for row in signed] for k in range(5)]

    def _means(self):
        S, n = self.sums, self.raw[:, W_N].tolist()
        scale = [Fraction(2) ** s for s in self.scale_exp]

        def ratio(num, den):
            if den == 0:
                return math.nan
            try:
                return float(Fraction(num) / Fraction(den))
            except OverflowError:
                return math.copysign(math.inf, num * den)
        out = {"rho": [ratio(S[0][b] * scale[0], n[b]) for b in range(self.nbins)]}
        for name, k in (("un", 1), ("ut", 2), ("E", 3)):
            out[name] = [ratio(S[k][b] * scale[k], S[0][b] * scale[0]) if n[b] else math.nan for b in range(self.nbins)]
        out["p"] = [ratio(S[4][b] * scale[4], n[b]) if self.with_p else math.nan for b in range(self.nbins)]
        return {k: np.array(v, dtype=np.float64) for k, v in out.items()}

    def _extrema(self):
        has = self.raw[:, W_N] != 0
        out = {}
        for name, w in (("rho_min", W_RHO_MIN), ("rho_max", W_RHO_MAX), ("p_min", W_P_MIN), ("p_max", W_P_MAX)):
            ok = has & (self.with_p or name.startswith("rho"))
            out[name] = np.array([from_key(int(k)) if o else math.nan for k, o in zip(self.raw[:, w], np.broadcast_to(ok, has.shape))])
        return out

    @property
    def coord(self):
        b = np.arange(self.nbins, dtype=np.float64) + 0.5
        if self.kind == "r":
            return b * self.dr
        ax = 0 if self.kind == "x" else 1
        return self.origin[ax] + b * self.width * self.spec[6 + ax]

    def table(self):
        """Everything a profile file holds → dict (``io.read_profile_file`` returns the same)."""
        t = {"kind": self.kind, "cycle": self.cycle, "time": self.time, "coord": self.coord, "n": self.n}
        if self.kind == "r":
            t["centre"], t["dr"] = self.centre, self.dr
        else:
            t["width"] = self.width
        t.update(self._once("means", self._means))
        t.update(self._once("extrema", self._extrema))
        return t

    def __getattr__(self, name):
        if name in ("rho", "un", "ut", "E", "p"):
            return self._once("means", self._means)[name]
        if name in ("rho_min", "rho_max", "p_min", "p_max"):
            return self._once("extrema", self._extrema)[name]
        raise AttributeError(name)

    def merge(self, other):
        if (self.spec, self.scale_exp, self.origin) != (other.spec, other.scale_exp, other.origin):
            solver_error("config", f"profiles of another kind, binning or scale do not merge: {self.spec}, {self.scale_exp} "
                                   f"against {other.spec}, {other.scale_exp}")
        return Profile(merge_raw(self.raw, other.raw), self.spec, self.scale_exp, self.origin, self.cycle, self.time)

    def __eq__(self, other):
        return isinstance(other, Profile) and (self.spec, self.scale_exp, self.origin) == (other.spec, other.scale_exp, other.origin) \
            and np.array_equal(self.raw, other.raw)

    def report(self):
        t = self.table()
        what = f"centre {t['centre']}, dr = {t['dr']:.6g}" if self.kind == "r" else f"width {self.width}"
        lines = [f"Profile along {self.kind} ({what}), {self.nbins} bins, {int(self.raw[:, W_N].sum())} cells, "
                 f"{int(self.raw[:, W_BAD].sum())} bad, quanta 2^{list(self.scale_exp)}"]
        for b in range(self.nbins):
            lines.append(f"  {t['coord'][b]:12.5g}  n = {int(t['n'][b]):9d}  rho = {t['rho'][b]:12.5g}  un = {t['un'][b]:12.5g}  "
                         f"ut = {t['ut'][b]:12.5g}  E = {t['E'][b]:12.5g}  p = {t['p'][b]:12.5g}")
        return "\n".join(lines)

    def __repr__(self):
        return f"Profile({self.kind}, nbins={self.nbins}, scale_exp={self.scale_exp}, cycle={self.cycle})"


# ---- device side -----------------------------------------------------------------------------------------------------------
def make_spec(p0, kind, bins=None, width=1, centre=None, dr=None, with_p=True):
    """The binning of a profile of the global domain of ``p0`` → the tuple ``Profile.spec`` holds."""
    if kind not in KINDS:
        solver_error("config", f"unknown profile kind {kind!r}: 'x', 'y' or 'r'")
    NX, NY = p0.global_grid
    dx, dy = float(p0.cell_size(0)), float(p0.cell_size(1))
    if isinstance(width, bool) or int(width) != width or width < 1:
        solver_error("config", f"profile width must be an integer >= 1, got {width!r}")
    width = int(width)
    cx = cy = 0.0
    inv_dr = 1.0
    if kind == "r":
        if centre is None:
            centre = (p0.origin[0] + p0.domain_size[0] / 2, p0.origin[1] + p0.domain_size[1] / 2)
        dr = min(dx, dy) if dr is None else float(dr)
        if not (math.isfinite(dr) and dr > 0):
            solver_error("config", f"profile dr must be a finite number > 0, got {dr!r}")
        cx, cy = (float(centre[0]) - p0.origin[0]) / dx, (float(centre[1]) - p0.origin[1]) / dy
        inv_dr = 1.0 / dr
        if bins is None:
            far = max(math.hypot((X - cx) * dx, (Y - cy) * dy) for X in (0, NX) for Y in (0, NY))
            bins = int(math.floor(far * inv_dr)) + 1
    elif bins is None:
        bins = -(-(NX if kind == "x" else NY) // width)
    if isinstance(bins, bool) or int(bins) != bins or bins < 1:
        solver_error("config", f"profile bins must be an integer >= 1, got {bins!r}")
    eos = -1 if not with_p else (1 if p0.test.eos == "bizarrium" else 0)
    return (KINDS[kind], eos, int(bins), width, cx, cy, dx, dy, inv_dr, float(p0.test.gamma))


def _c_spec(spec, scale_exp):
    s = ProfileSpec()
    s.kind, s.eos, s.nbins, s.width, s.cx, s.cy, s.dx, s.dy, s.inv_dr, s.gamma = spec
    s.scale_exp[:] = list(scale_exp)
    return s


def _call(name, params, grid, window, spec, out):
    col0, row0, wnx, wny = window
    check(params.fn(name)(params.device.ctx, grid.size.size[0], grid.size.ghosts, params.N[0], params.N[1],
                          *[C.c_void_p(grid.data[f].ptr) for f in ("rho", "u", "v", "E")], col0, row0, wnx, wny,
                          params.N_origin[0] - 1 + col0, params.N_origin[1] - 1 + row0, C.byref(spec), C.c_void_p(out.ptr)))


def state_bounds(tiles, spec, windows=None):
    """The bounds pass over every tile (its whole window, or ``windows[i]``) → the five bit patterns, merged by maximum."""
    c_spec, outs = _c_spec(spec, (0,) * 5), []
    try:
        for i, (params, grid) in enumerate(tiles):
            outs.append(params.device.zeros(5, np.uint64))
            _call("profile_bounds", params, grid, windows[i] if windows else (0, 0, params.N[0], params.N[1]), c_spec, outs[-1])
        top = np.zeros(5, dtype=np.uint64)
        for (params, _), out in zip(tiles, outs):
            params.wait()
            top = np.maximum(top, out.to_host())
    finally:
        for out in outs:
            out.free()
    return tuple(int(v) for v in top)


def profile_state(tiles, kind, bins=None, width=1, centre=None, dr=None, with_p=True, scale_exp=None, windows=None):
    """The profile of the state held by the ``(params, grid)`` of ``tiles`` (idle) → ``Profile``. ``kind``: ``"x" | "y" | "r"``;
    ``bins``: how many (default: all of the axis, or out to the farthest corner); ``width``: cells per bin (x, y); ``centre``:
    physical coordinates (r; default: the domain's centre); ``dr``: the ring width (r; default ``min(dx, dy)``); ``with_p``:
    also the pressure — the EOS of each cell's state, no ``p`` vector is read; ``scale_exp``: five exponents instead of the
    default scale (then no bounds pass runs); ``windows``: per tile the ``(col0, row0, wnx, wny)`` of its real cells to take
    instead of all of them. Each tile runs the bounds pass, the bounds merge by maximum BEFORE any main pass so that every
    tile uses the same quanta, then each tile's ``nbins x 192`` bytes are read back and merged on the host."""
    p0 = tiles[0][0]
    spec = make_spec(p0, kind, bins, width, centre, dr, with_p)
    if scale_exp is None:
        scale_exp = default_scale(state_bounds(tiles, spec, windows))
    scale_exp = tuple(int(s) for s in scale_exp)
    if len(scale_exp) != 5 or any(abs(s) > SCALE_LIMIT for s in scale_exp):
        solver_error("config", f"scale_exp takes five exponents within ±{SCALE_LIMIT}, got {scale_exp!r}")
    c_spec, nbins, outs = _c_spec(spec, scale_exp), spec[2], []
    try:
        for i, (params, grid) in enumerate(tiles):
            outs.append(params.device.empty(nbins * WORDS, np.uint64))
            check(params.device._L.armon_hip_profile_reset(params.device.ctx, nbins, C.c_void_p(outs[-1].ptr)))
            _call("profile", params, grid, windows[i] if windows else (0, 0, params.N[0], params.N[1]), c_spec, outs[-1])
        raw = neutral(nbins)
        for (params, _), out in zip(tiles, outs):
            params.wait()
            raw = merge_raw(raw, out.to_host().reshape(nbins, WORDS))
    finally:
        for out in outs:
            out.free()
    return Profile(raw, spec, scale_exp, p0.origin)


# ---- the run options (profile_step, profile_kind, ..., profile_at_end) -----------------------------------------------------
def profile_path(params, cycle):
    return os.path.join(params.output_dir, f"{params.profile_file}_{cycle:06d}.txt")


def profile_run(owner, params, gdt):
    """The profile of the run ``owner`` (a ``BlockGrid`` or a ``TileGroup``) after ``gdt.cycle`` completed cycles, written to
    ``profile_path`` and appended to ``owner.profiles``."""
    from .compare import _tiles_of
    from .io import write_profile_file
    prof = profile_state(_tiles_of(owner), params.profile_kind, bins=params.profile_bins, width=params.profile_width,
                         centre=params.profile_centre, dr=params.profile_dr)
    prof.cycle, prof.time = int(gdt.cycle), float(gdt.time)
    os.makedirs(params.output_dir, exist_ok=True)
    write_profile_file(profile_path(params, gdt.cycle), prof, params.output_precision)
    owner.profiles.append((gdt.cycle, prof))
    return prof
