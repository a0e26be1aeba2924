"""Exact solutions of the test cases that have one, and the state's distance from them (csrc/analytic.hip). No reference
counterpart: the reference holds its runs to golden files only.

Host side, pure numpy: ``riemann_exact`` (Toro ch. 4), ``sedov_similarity`` (the self-similar point blast, integrated inward
from the shock), ``reference_for`` (the solution of a run's test case at a time) and ``ExactSolution.table`` (a caller's own
1-D reference along x, y or r). ``evaluate`` / ``stored_reference`` / ``cell_vars`` / ``reference_record`` restate the
device rule of include/armon_hip.h (armon_hip_exact_norms) operation for operation; the tests hold the kernels against them.

THE RULE. The solution (rho, un, p) at ``samples`` points per cell and axis, their mean, then the mean AS THE DATA TYPE STORES
IT: u, v from un, E = p / ((gamma - 1) rho) + (u u + v v) / 2, the four converted to the data type — exactly what
``fill_exact`` writes. The state and this stored reference both go through ``cell_vars`` (rho, un, ut, p; p = the EOS
evaluated in the data type), d = state - reference, and d, |d|, d d enter exact fixed-point sums (profile.py's quantise /
limbs), |d| a (value, position) maximum. A state written by ``fill_exact`` is therefore at distance 0 exactly, and the record
is a function of the state and the spec only: tiles merge to the single block's record word for word.
"""
import ctypes as C
import math
import os
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from ._lib import ExactSpec, check, solver_error
from .profile import EDGE, KINDS, MASK, SCALE_LIMIT, from_limbs, quantise_limbs

RIEMANN, TABLE = 0, 1
VARS = ("rho", "un", "ut", "p")
WORDS = 16
W_N, W_BAD, W_D, W_ABS, W_SQ, W_MAX, W_AT = 0, 1, 2, 5, 8, 11, 12
NO_CLOSED_FORM = ("Sod_circ", "Bizarrium", "DebugIndexes")


def has_closed_form(test, periodic=None):
    """Whether ``reference_for`` knows the exact solution of ``test``: a built-in case by its name; a user-defined problem
    (problem.py) when it is a one-dimensional perfect-gas Riemann problem at gamma = 7/5 (``BoundProblem.riemann_setup``).
    Never under a body force: the solutions known here are those of the unforced equations. Never when the
    axis a Riemann problem varies along is periodic: the jump then has a mirror image one period away and
    the solution of the unbounded problem is not the flow's. ``periodic``: the run's periodic axes (None: those of the
    test's own boundaries)."""
    if tuple(getattr(test, "gravity", (0., 0.))) != (0., 0.):
        return False
    if periodic is None:
        from .boundaries import periodic_axes
        periodic = periodic_axes(test.boundaries)
    if getattr(test, "is_problem", False):
        setup = test.riemann_setup()
        return setup is not None and not periodic["xy".index(setup[0])]
    if test.name in ("Sod", "Sod_y") and periodic[0 if test.name == "Sod" else 1]:
        return False
    return test.name not in NO_CLOSED_FORM


# ---- the Riemann problem ---------------------------------------------------------------------------------------------------
def riemann_exact(left, right, gamma=7 / 5, tol=1e-15, max_iter=100):
    """The exact solution of the perfect-gas Riemann problem between ``left`` and ``right`` = (rho, u, p): Newton iteration on
    p* (Toro, ch. 4) → a namespace with ``p_star, u_star, rho_star_l, rho_star_r, c_star_l, c_star_r``, the outer sound speeds
    ``c_l, c_r`` and ``speeds`` = (left head, left tail, contact, right tail, right head); a shock has head == tail."""
    g = float(gamma)
    (rl, ul, pl), (rr, ur, pr) = (tuple(float(x) for x in left), tuple(float(x) for x in right))
    if not (rl > 0 and rr > 0 and pl > 0 and pr > 0 and g > 1):
        solver_error("analytic", f"the Riemann problem needs rho > 0, p > 0 and gamma > 1, got {left}, {right}, {gamma}")
    cl, cr = math.sqrt(g * pl / rl), math.sqrt(g * pr / rr)
    if 2 / (g - 1) * (cl + cr) <= ur - ul:
        solver_error("analytic", "the Riemann problem generates vacuum: no star state")

    def f(p, rk, pk, ck):
        if p > pk:                              # shock
            A, B = 2 / ((g + 1) * rk), (g - 1) / (g + 1) * pk
            s = math.sqrt(A / (p + B))
            return (p - pk) * s, s * (1 - (p - pk) / (2 * (B + p)))
        pr_ = p / pk                            # rarefaction
        return 2 * ck / (g - 1) * (pr_ ** ((g - 1) / (2 * g)) - 1), pr_ ** (-(g + 1) / (2 * g)) / (rk * ck)

    z = (g - 1) / (2 * g)                       # start: the two-rarefaction value (positive)
    p = ((cl + cr - (g - 1) / 2 * (ur - ul)) / (cl / pl ** z + cr / pr ** z)) ** (1 / z)
    for _ in range(max_iter):
        fl, dl = f(p, rl, pl, cl)
        fr, dr = f(p, rr, pr, cr)
        new = p - (fl + fr + ur - ul) / (dl + dr)
        if new <= 0:
            new = 1e-6 * p
        done = 2 * abs(new - p) / (new + p) < tol
        p = new
        if done:
            break
    fl, fr = f(p, rl, pl, cl)[0], f(p, rr, pr, cr)[0]
    u = 0.5 * (ul + ur) + 0.5 * (fr - fl)
    mu = (g - 1) / (g + 1)

    def star(rk, pk):
        q = p / pk
        return rk * ((q + mu) / (mu * q + 1)) if p > pk else rk * q ** (1 / g)
    rsl, rsr = star(rl, pl), star(rr, pr)
    csl, csr = math.sqrt(g * p / rsl), math.sqrt(g * p / rsr)
    if p > pl:
        head_l = tail_l = ul - cl * math.sqrt((g + 1) / (2 * g) * p / pl + (g - 1) / (2 * g))
    else:
        head_l, tail_l = ul - cl, u - csl
    if p > pr:
        head_r = tail_r = ur + cr * math.sqrt((g + 1) / (2 * g) * p / pr + (g - 1) / (2 * g))
    else:
        head_r, tail_r = ur + cr, u + csr
    return SimpleNamespace(gamma=g, left=(rl, ul, pl), right=(rr, ur, pr), c_l=cl, c_r=cr, p_star=p, u_star=u, rho_star_l=rsl,
                           rho_star_r=rsr, c_star_l=csl, c_star_r=csr, speeds=(head_l, tail_l, u, tail_r, head_r))


# ---- the point blast -------------------------------------------------------------------------------------------------------
def sedov_similarity(gamma=1.4, nu=2, nodes=4000, stop=0.02):
    """The self-similar point blast in ``nu`` dimensions: with lam = r / R, rho = rho0 g(lam), u = R' v(lam), p = rho0 R'^2 pi(lam),
    delta = 2 / (nu + 2), k = (delta - 1) / delta,
        (v - lam) g' + g v' = -(nu - 1) g v / lam,   (v - lam) v' + pi' / g = -k v,   (v - lam)(pi' / pi - gamma g' / g) = -2 k
    integrated inward by RK4 from g = (gamma+1)/(gamma-1), v = pi = 2/(gamma+1) at lam = 1 on ``nodes`` uniform steps down to
    lam = ``stop``; below, g follows its power law lam^(nu/(gamma-1)), v is linear and pi constant. → a namespace with
    ``alpha`` (R(t) = (E0 t^2 / (alpha rho0))^(1/(nu+2)); Simpson's rule on the nodes), ``lam, g, v, pi`` on nodes + 1 points."""
    gamma, nu, M = float(gamma), int(nu), int(nodes)
    if M < 8 or M % 2:
        solver_error("analytic", f"sedov_similarity needs an even number of nodes >= 8, got {nodes!r}")
    delta = 2.0 / (nu + 2)
    k = (delta - 1) / delta

    def rhs(lam, y):
        g, v, pi = y
        w = v - lam
        a = pi / (g * w)
        dv = (-k * v + a * (2 * k + gamma * (nu - 1) * v / lam)) / (w - gamma * a)
        dg = g * (-(nu - 1) * v / lam - dv) / w
        dpi = pi * (-2 * k / w + gamma * dg / g)
        return np.array([dg, dv, dpi])

    lam = np.arange(M + 1, dtype=np.float64) / M
    out = np.zeros((3, M + 1))
    y = np.array([(gamma + 1) / (gamma - 1), 2 / (gamma + 1), 2 / (gamma + 1)])
    out[:, M] = y
    h, j = -1.0 / M, M
    while j > 0 and lam[j - 1] >= stop:
        x = lam[j]
        k1 = rhs(x, y)
        k2 = rhs(x + h / 2, y + h / 2 * k1)
        k3 = rhs(x + h / 2, y + h / 2 * k2)
        k4 = rhs(x + h, y + h * k3)
        y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        j -= 1
        out[:, j] = y
    if j > 0:                                   # the centre: g -> 0
        s = lam[:j] / lam[j]
        out[0, :j] = out[0, j] * s ** (nu / (gamma - 1))
        out[1, :j] = out[1, j] * s
        out[2, :j] = out[2, j]
    g, v, pi = out
    S = {1: 2.0, 2: 2 * math.pi, 3: 4 * math.pi}[nu]
    alpha = delta ** 2 * S * _simpson((0.5 * g * v * v + pi / (gamma - 1)) * lam ** (nu - 1), 1.0 / M)
    return SimpleNamespace(gamma=gamma, nu=nu, alpha=float(alpha), lam=lam, g=g, v=v, pi=pi, delta=delta)


def _simpson(f, h):
    return h / 3 * (f[0] + f[-1] + 4 * f[1:-1:2].sum() + 2 * f[2:-1:2].sum())


# ---- a solution on a grid --------------------------------------------------------------------------------------------------
def _exponent_above(x):
    """e with |x| < 2^e (the frexp exponent), 0 for 0."""
    x = abs(float(x))
    return math.frexp(x)[1] if x != 0 else 0


class ExactSolution:
    """An exact solution along ``coord`` = ``"x" | "y" | "r"`` measured from ``centre`` (physical coordinates): a Riemann
    problem at ``time`` (``riemann`` = the result of ``riemann_exact``) or a table (``scale``: where lam = 1; ``values`` =
    (3, M + 1) rho, un, p on uniform nodes of lam in [0, 1]; ``outer`` = (rho, un, p) beyond). ``magnitude``: the largest
    |rho|, |un|, |p| of the solution, from which the default quanta come."""

    def __init__(self, form, coord, centre, gamma, time=0.0, riemann=None, scale=1.0, values=None, outer=(0., 0., 0.), info=None):
        if coord not in KINDS:
            solver_error("analytic", f"unknown coordinate {coord!r}: 'x', 'y' or 'r'")
        self.form, self.coord, self.centre, self.gamma, self.time = form, coord, tuple(float(c) for c in centre), float(gamma), float(time)
        self.riemann, self.scale, self.outer = riemann, float(scale), tuple(float(o) for o in outer)
        self.values = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
        self.info = info or {}
        if form == TABLE:
            if self.values.ndim != 2 or self.values.shape[0] != 3 or self.values.shape[1] < 2:
                solver_error("analytic", f"a table holds rho, un, p on at least two nodes: (3, M + 1) values, got {self.values.shape}")
            if not (math.isfinite(self.scale) and self.scale > 0):
                solver_error("analytic", f"the scale of a table must be a finite number > 0, got {scale!r}")
            top = np.maximum(np.abs(self.values).max(axis=1), np.abs(self.outer))
        else:
            r = riemann
            top = (max(r.left[0], r.right[0], r.rho_star_l, r.rho_star_r), max(abs(r.left[1]), abs(r.right[1]), abs(r.u_star)),
                   max(r.left[2], r.right[2], r.p_star))
        self.magnitude = tuple(float(t) for t in top)

    @classmethod
    def table(cls, coord, scale, rho, un, p, outer, centre=(0., 0.), gamma=7 / 5):
        """A caller's own 1-D reference: ``rho, un, p`` on M + 1 uniform nodes of ``coord`` / ``scale`` in [0, 1], ``outer`` =
        (rho, un, p) where the coordinate reaches ``scale``; ``centre``: where the coordinate is 0."""
        return cls(TABLE, coord, centre, gamma, scale=scale, values=np.stack([np.asarray(a, dtype=np.float64) for a in (rho, un, p)]),
                   outer=outer)

    def default_scale(self):
        """``(e_k - 62, 2 e_k - 62)`` per variable, 2^e_k the power of two above the solution's largest |rho|, |un|, |p|; the
        transverse velocity takes un's."""
        e = [_exponent_above(m) for m in self.magnitude]
        e = (e[0], e[1], e[1], e[2])
        return tuple((ek - 62, 2 * ek - 62) for ek in e)

    def spec(self, origin, cell, global_nx, samples=1, coord_range=None, scale_exp=None):
        """The spec of this solution on a grid of cells ``cell = (dx, dy)`` whose first cell starts at ``origin`` (what
        ``armon_exact_spec`` holds, as a namespace)."""
        if samples not in (1, 2, 4) or isinstance(samples, bool):
            solver_error("analytic", f"samples must be 1, 2 or 4, got {samples!r}")
        lo, hi = (-math.inf, math.inf) if coord_range is None else (float(coord_range[0]), float(coord_range[1]))
        if math.isnan(lo) or math.isnan(hi):
            solver_error("analytic", f"coord_range is (min, max), got {coord_range!r}")
        scale_exp = self.default_scale() if scale_exp is None else tuple((int(a), int(b)) for a, b in scale_exp)
        if len(scale_exp) != 4 or any(abs(s) > SCALE_LIMIT for pair in scale_exp for s in pair):
            solver_error("analytic", f"scale_exp takes four pairs of exponents within ±{SCALE_LIMIT}, got {scale_exp!r}")
        dx, dy = float(cell[0]), float(cell[1])
        s = SimpleNamespace(form=self.form, coord=KINDS[self.coord], samples=int(samples), eos=0, global_nx=int(global_nx),
                            cx=(self.centre[0] - float(origin[0])) / dx, cy=(self.centre[1] - float(origin[1])) / dy, dx=dx, dy=dy,
                            gamma=self.gamma, coord_min=lo, coord_max=hi, scale_exp=scale_exp)
        if self.form == RIEMANN:
            r, g = self.riemann, self.gamma
            if g != 7 / 5:
                solver_error("analytic", f"the fans of the Riemann solution are written for gamma = 7/5, got {g!r}")
            s.time = self.time
            s.side = ((r.left[0], r.left[1], r.left[2], r.c_l), (r.right[0], r.right[1], r.right[2], r.c_r))
            s.star = (r.p_star, r.u_star, r.rho_star_l, r.rho_star_r)
            s.speed = tuple(r.speeds)
            s.g1, s.g2, s.g3 = 2 / (g + 1), ((g - 1) / ((g + 1) * r.c_l), (g - 1) / ((g + 1) * r.c_r)), (g - 1) / 2
        else:
            s.inv_scale, s.M, s.outer, s.values = 1.0 / self.scale, self.values.shape[1] - 1, self.outer, self.values
        return s

    def __repr__(self):
        what = f"Riemann at t = {self.time:.6g}" if self.form == RIEMANN else f"table of {self.values.shape[1]} nodes, scale {self.scale:.6g}"
        return f"ExactSolution({what}, along {self.coord} from {self.centre})"


def sedov_energy(params):
    """E0 of the Sedov case as the grid holds it: the cells whose centre lies within ``test.r`` of the origin (init_test's own
    arithmetic for the centres), times the cell area, times rho (E_high - E_low)."""
    T = params.T
    dx, dy = params.cell_size(0), params.cell_size(1)
    r = T(params.test.r)
    e_high = T(float((1 / 1.033) ** 5 / float(T(math.pi) * (r * r))))
    e_low = T(2.5e-14)
    NX, NY = params.global_grid
    ix = np.arange(NX, dtype=np.int64).astype(params.data_type) * dx + T(params.origin[0]) + dx / T(2)
    iy = np.arange(NY, dtype=np.int64).astype(params.data_type) * dy + T(params.origin[1]) + dy / T(2)
    near_x, near_y = ix[np.abs(ix) <= r], iy[np.abs(iy) <= r]
    count = int(np.count_nonzero(near_x[None, :] * near_x[None, :] + near_y[:, None] * near_y[:, None] <= r * r))
    return count * float(dx) * float(dy) * 1.0 * (float(e_high) - float(e_low)), count


def reference_for(params, time, nodes=4000):
    """The exact solution of the run's test case at ``time`` → ``ExactSolution``. Refused (``SolverException("analytic", …)``):
    a case without a closed form, a time <= 0, and a time at which a wave has reached a wall."""
    name = params.test.name
    if not has_closed_form(params.test, getattr(params, "periodic", None)):
        solver_error("analytic", f"the test case {name} has no closed-form solution (give error_norms a table: ExactSolution.table)")
    time = float(time)
    if not (math.isfinite(time) and time > 0):
        solver_error("analytic", f"the exact solution needs a time > 0, got {time!r}")
    gamma = float(params.test.gamma)
    ox, oy = (float(o) for o in params.origin)
    lx, ly = (float(d) for d in params.domain_size)
    setup = None
    if getattr(params.test, "is_problem", False):
        setup = params.test.riemann_setup()         # a user-defined problem: decided by what it holds, never by its name
    elif name in ("Sod", "Sod_y"):
        setup = ("x" if name == "Sod" else "y", 0.5, (1.0, 0.0, (gamma - 1) * 1.0 * 2.5), (0.125, 0.0, (gamma - 1) * 0.125 * 2.0))
    if setup is not None:
        axis, x0, left, right = setup
        r = riemann_exact(left, right, gamma)
        lo, length = (ox, lx) if axis == "x" else (oy, ly)
        if x0 + r.speeds[0] * time <= lo or x0 + r.speeds[4] * time >= lo + length:
            solver_error("analytic", f"at t = {time:.6g} a wave of the {name} problem has reached a wall (speeds {r.speeds[0]:.5f}, "
                                     f"{r.speeds[4]:.5f} from {x0}): the solution of the unbounded problem no longer applies")
        return ExactSolution(RIEMANN, axis, (x0, 0.0) if axis == "x" else (0.0, x0), gamma, time=time, riemann=r)
    if name == "Sedov":
        E0, count = sedov_energy(params)
        rho0, p0 = 1.0, (gamma - 1) * 1.0 * 2.5e-14
        sim = sedov_similarity(gamma, 2, nodes)
        R = (E0 * time * time / (sim.alpha * rho0)) ** (1 / 4)
        wall = min(-ox, ox + lx, -oy, oy + ly)
        if R >= wall:
            solver_error("analytic", f"at t = {time:.6g} the blast wave (R = {R:.5f}) has reached a side of the domain ({wall:.5f} away)")
        Rdot = sim.delta * R / time
        values = np.stack([rho0 * sim.g, Rdot * sim.v, rho0 * Rdot * Rdot * sim.pi])
        return ExactSolution(TABLE, "r", (0.0, 0.0), gamma, time=time, scale=R, values=values, outer=(rho0, 0.0, p0),
                             info=dict(E0=E0, cells=count, alpha=sim.alpha, R=R, Rdot=Rdot))
    solver_error("analytic", f"no exact solution is known for the test case {name}")


# ---- the rule, in Python (the tests' oracle) -------------------------------------------------------------------------------
def _point(s, q):
    """ref_point of csrc/analytic.hip on an array of coordinates → rho, un, p."""
    with np.errstate(all="ignore"):
        if s.form == RIEMANN:
            xi = q / np.float64(s.time)
            sp = [np.float64(v) for v in s.speed]
            region = np.select([xi < sp[0], xi < sp[1], xi < sp[2], xi < sp[3], xi < sp[4]], [0, 1, 2, 3, 4], 5)
            fans = []
            for K, sign in ((0, 1), (1, -1)):
                rhoK, uK, pK, cK = (np.float64(v) for v in s.side[K])
                t = np.float64(s.g2[K]) * (uK - xi)
                r = np.float64(s.g1) + t if K == 0 else np.float64(s.g1) - t
                r2 = r * r
                r4 = r2 * r2
                r5 = r4 * r
                r7 = r5 * r2
                w = np.float64(s.g3) * uK
                fans.append((rhoK * r5, np.float64(s.g1) * (((cK if K == 0 else -cK) + w) + xi), pK * r7))
            pst, ust, rsl, rsr = s.star
            one = np.ones_like(xi)
            pick = lambda k: np.choose(region, [one * s.side[0][k], fans[0][k], one * (rsl, ust, pst)[k], one * (rsr, ust, pst)[k],
                                                fans[1][k], one * s.side[1][k]])
            return pick(0), pick(1), pick(2)
        lam = q * np.float64(s.inv_scale)
        inner = lam < 1.0
        sc = lam * np.float64(s.M)
        fj = np.floor(sc)
        j = np.where(fj > 0, np.where(fj < s.M - 1, fj, s.M - 1), 0)
        j = np.where(inner, j, 0).astype(np.int64)
        f = sc - j.astype(np.float64)
        out = []
        for k in range(3):
            t = s.values[k]
            a, b = t[j], t[j + 1]
            out.append(np.where(inner, a + f * (b - a), np.float64(s.outer[k])))
        return tuple(out)


def _centre(s, gx, gy):
    gx, gy = np.broadcast_arrays(np.asarray(gx, dtype=np.int64), np.asarray(gy, dtype=np.int64))
    rx = ((gx.astype(np.float64) + 0.5) - np.float64(s.cx)) * np.float64(s.dx)
    ry = ((gy.astype(np.float64) + 0.5) - np.float64(s.cy)) * np.float64(s.dy)
    rr = np.sqrt(rx * rx + ry * ry) if s.coord == 2 else np.zeros_like(rx)
    q = (rx, ry, rr)[s.coord]
    return gx, gy, rx, ry, rr, (q >= s.coord_min) & (q < s.coord_max)


def evaluate(spec, gx, gy):
    """The cell means (rho, un, p) of the solution ``spec`` in the cells at the global positions ``gx, gy`` (broadcast) → three
    fp64 arrays: the mean of ``samples`` points per axis, summed in the device's order."""
    s = spec
    gx, gy, *_ = _centre(s, gx, gy)
    ns = s.samples
    off = [(i + 0.5) / ns for i in range(ns)]
    acc = [np.zeros(gx.shape), np.zeros(gx.shape), np.zeros(gx.shape)]
    fx, fy = gx.astype(np.float64), gy.astype(np.float64)
    if s.coord == 2:
        for oj in off:
            py = ((fy + oj) - np.float64(s.cy)) * np.float64(s.dy)
            for oi in off:
                px = ((fx + oi) - np.float64(s.cx)) * np.float64(s.dx)
                for a, v in zip(acc, _point(s, np.sqrt(px * px + py * py))):
                    a += v
        w = (1.0 / ns) * (1.0 / ns)
    else:
        g, c, h = (fx, s.cx, s.dx) if s.coord == 0 else (fy, s.cy, s.dy)
        for oi in off:
            for a, v in zip(acc, _point(s, ((g + oi) - np.float64(c)) * np.float64(h))):
                a += v
        w = 1.0 / ns
    return tuple(a * w for a in acc)


def stored_reference(spec, gx, gy, dtype=np.float64):
    """What ``fill_exact`` writes into the cells at ``gx, gy``: ``(rho, u, v, E)`` in ``dtype`` and the mask of the cells whose
    centre coordinate lies in [coord_min, coord_max) (the others are left alone)."""
    s = spec
    gx, gy, rx, ry, rr, keep = _centre(s, gx, gy)
    rho, un, p = evaluate(s, gx, gy)
    with np.errstate(all="ignore"):
        if s.coord == 0:
            u, v = un, np.zeros_like(un)
        elif s.coord == 1:
            u, v = np.zeros_like(un), un
        else:
            safe = np.where(rr == 0., 1., rr)
            u = np.where(rr == 0., 0., un * rx / safe)
            v = np.where(rr == 0., 0., un * ry / safe)
        gm1 = np.float64(s.gamma) - 1.0
        E = p / (gm1 * rho) + 0.5 * (u * u + v * v)
        return tuple(a.astype(dtype) for a in (rho, u, v, E)), keep


def cell_vars(spec, rho, u, v, E, gx, gy):
    """rho, un, ut, p of cells holding ``rho, u, v, E`` (arrays of the run's data type) at ``gx, gy`` → four fp64 arrays; p is
    the perfect-gas EOS evaluated in the data type, operation for operation as the EOS kernels do."""
    s = spec
    T = np.asarray(rho).dtype.type
    _, _, rx, ry, rr, _ = _centre(s, gx, gy)
    with np.errstate(all="ignore"):
        e = E - T(0.5) * (u * u + v * v)
        p = ((T(s.gamma) - T(1.)) * rho * e).astype(np.float64)
        r64, u64, v64 = (np.asarray(a).astype(np.float64) for a in (rho, u, v))
        if s.coord == 0:
            un, ut = u64, v64
        elif s.coord == 1:
            un, ut = v64, u64
        else:
            safe = np.where(rr == 0., 1., rr)
            un = np.where(rr == 0., 0., (u64 * rx + v64 * ry) / safe)
            ut = np.where(rr == 0., 0., (v64 * rx - u64 * ry) / safe)
    return r64, un, ut, p


def neutral():
    raw = np.zeros((4, WORDS), dtype=np.uint64)
    raw[:, W_AT] = MASK
    return raw


def reference_record(spec, rho, u, v, E, origin=(0, 0), skip=None):
    """The record of the 2-D arrays ``rho, u, v, E`` (the run's data type) whose first cell sits at global ``origin = (gx, gy)``
    → ``(4, 16)`` uint64, by the rule above with Python integers for the sums. ``skip``: cells to leave out altogether."""
    s = spec
    ny, nx = np.shape(rho)
    gx = np.arange(nx, dtype=np.int64)[None, :] + int(origin[0])
    gy = np.arange(ny, dtype=np.int64)[:, None] + int(origin[1])
    state = [np.asarray(a) for a in (rho, u, v, E)]
    ref, keep = stored_reference(s, gx, gy, state[0].dtype)
    if skip is not None:
        keep = keep & ~np.asarray(skip)
    A, B = cell_vars(s, *state, gx, gy), cell_vars(s, *ref, gx, gy)
    ok = np.ones((ny, nx), dtype=bool)
    for a in [x.astype(np.float64) for x in state] + [x.astype(np.float64) for x in ref] + list(A) + list(B):
        ok &= np.isfinite(a)
    quanta = []
    with np.errstate(all="ignore"):
        for k in range(4):
            d = A[k] - B[k]
            sq = d * d
            *q1, ok1 = quantise_limbs(d, s.scale_exp[k][0])
            *q2, ok2 = quantise_limbs(sq, s.scale_exp[k][1])
            ok &= ok1 & ok2
            quanta.append((d, q1, q2))
    use = keep & ok
    g = (gy * np.int64(s.global_nx) + gx)
    words = []
    for k in range(4):
        d, q1, q2 = quanta[k]
        w = [0] * WORDS
        w[W_N], w[W_BAD] = int(use.sum()), int((keep & ~ok).sum())
        sign = np.where(np.signbit(d[use]), -1, 1).astype(np.int64)
        for base, l, sg in ((W_D, q1, sign), (W_ABS, q1, np.int64(1)), (W_SQ, q2, np.int64(1))):
            for j in range(3):              # a limb of every cell at once, summed exactly (below 2^63)
                w[base + j] = int((l[j][use].astype(np.int64) * sg).sum(dtype=np.int64))
        bits = np.abs(d[use]).view(np.uint64)
        w[W_AT] = MASK
        if bits.size and int(bits.max()) != 0:
            top = int(bits.max())
            w[W_MAX], w[W_AT] = top, int(g[use][bits == top].min())
        words.append([x & MASK for x in w])
    return np.array(words, dtype=np.uint64)


def merge_raw(x, y):
    """The merge of two ``(4, 16)`` records: sums add (mod 2^64, limb by limb), the (value, position) pair takes the larger value
    and on equal values the smaller position."""
    out = x + y
    for k in range(4):
        a, b = (int(x[k, W_MAX]), int(x[k, W_AT])), (int(y[k, W_MAX]), int(y[k, W_AT]))
        out[k, W_MAX], out[k, W_AT] = b if (b[0] > a[0] or (b[0] == a[0] and b[1] < a[1])) else a
    out[:, 13:] = 0
    return out


# ---- the result ------------------------------------------------------------------------------------------------------------
class _Var:
    def __init__(self, row, scale, nx):
        n = int(row[W_N])
        signed = row[W_D:W_MAX].view(np.int64).tolist()
        S = [from_limbs(signed[3 * i:3 * i + 3]) for i in range(3)]
        q0, q1 = Fraction(2) ** scale[0], Fraction(2) ** scale[1]
        self.n, self.n_bad = n, int(row[W_BAD])
        self.sums = tuple(S)
        self.bias = float(S[0] * q0 / n) if n else math.nan
        self.l1 = float(S[1] * q0 / n) if n else math.nan
        self.l2 = math.sqrt(S[2] * q1 / n) if n else math.nan
        self.linf = float(np.array([row[W_MAX]], dtype=np.uint64).view(np.float64)[0]) if n else math.nan
        at = int(row[W_AT])
        self.linf_at = None if at == MASK else (at % nx, at // nx)


class ErrorNorms:
    """``raw``: the ``(4, 16)`` words, one record for each of rho, un, ut, p. Decoded per variable (``norms.rho`` …): ``l1`` =
    S|d| / n, ``l2`` = sqrt(S d^2 / n), ``linf`` with ``linf_at`` = the global (gx, gy) of the first cell that attains it,
    ``bias`` = S d / n (each rounded once from the exact rational), ``n``, ``n_bad``.

    d is taken against the solution AS THE RUN'S DATA TYPE STORES IT (what ``fill_exact`` writes: rho, u, v, E rounded to the data
    type, p through the EOS in that type), not against the fp64 solution: in fp32 the reference itself is rounded at 2^-24
    relative, and along r its transverse velocity is within an ulp of 0 instead of exactly 0. A filled state is at distance 0."""

    def __init__(self, raw, scale_exp, global_nx, samples=1, cycle=0, time=0.0):
        self.raw = np.ascontiguousarray(raw, dtype=np.uint64).reshape(4, WORDS)
        self.scale_exp = tuple((int(a), int(b)) for a, b in scale_exp)
        self.global_nx, self.samples, self.cycle, self.time = int(global_nx), int(samples), int(cycle), float(time)
        for k, name in enumerate(VARS):
            setattr(self, name, _Var(self.raw[k], self.scale_exp[k], self.global_nx))

    n = property(lambda self: int(self.raw[0, W_N]))
    n_bad = property(lambda self: int(self.raw[0, W_BAD]))

    def merge(self, other):
        if (self.scale_exp, self.global_nx, self.samples) != (other.scale_exp, other.global_nx, other.samples):
            solver_error("config", f"error norms of another scale, grid or sampling do not merge: {self.scale_exp} against {other.scale_exp}")
        return ErrorNorms(merge_raw(self.raw, other.raw), self.scale_exp, self.global_nx, self.samples, self.cycle, self.time)

    def __eq__(self, other):
        return isinstance(other, ErrorNorms) and (self.scale_exp, self.global_nx, self.samples) == \
            (other.scale_exp, other.global_nx, other.samples) and np.array_equal(self.raw, other.raw)

    def table(self):
        """Everything an error-norms file holds → dict (``io.read_error_norms_file`` returns the same)."""
        t = {"cycle": self.cycle, "time": self.time, "samples": self.samples, "n": self.n, "n_bad": self.n_bad}
        for name in VARS:
            v = getattr(self, name)
            t[name] = {"l1": v.l1, "l2": v.l2, "linf": v.linf, "bias": v.bias, "linf_at": v.linf_at}
        return t

    def report(self):
        lines = [f"Error norms at cycle {self.cycle}, t = {self.time:.9g}: {self.n} cells, {self.n_bad} bad, {self.samples} sample(s) per axis"]
        for name in VARS:
            v = getattr(self, name)
            lines.append(f"  {name:>3}  L1 = {v.l1:12.5e}  L2 = {v.l2:12.5e}  Linf = {v.linf:12.5e} at {v.linf_at}  bias = {v.bias:+12.5e}")
        return "\n".join(lines)

    def __repr__(self):
        return f"ErrorNorms(L1(rho) = {self.rho.l1:.5e}, n = {self.n}, cycle = {self.cycle})"


# ---- device side -----------------------------------------------------------------------------------------------------------
def _c_spec(s, table_ptr):
    c = ExactSpec()
    c.form, c.coord, c.samples, c.eos, c.global_nx = s.form, s.coord, s.samples, s.eos, s.global_nx
    c.cx, c.cy, c.dx, c.dy, c.gamma, c.coord_min, c.coord_max = s.cx, s.cy, s.dx, s.dy, s.gamma, s.coord_min, s.coord_max
    for k in range(4):
        c.scale_exp[k][0], c.scale_exp[k][1] = s.scale_exp[k]
    if s.form == RIEMANN:
        c.time = s.time
        for K in range(2):
            c.side[K][:] = list(s.side[K])
        c.star[:], c.speed[:] = list(s.star), list(s.speed)
        c.g1, c.g3 = s.g1, s.g3
        c.g2[:] = list(s.g2)
    else:
        c.inv_scale, c.M = s.inv_scale, s.M
        c.outer[:] = list(s.outer)
        c.table = table_ptr
    return c


def _solution_for(p0, reference, time):
    if reference is None:
        if time is None:
            solver_error("analytic", "the exact solution of the test case needs a time")
        reference = reference_for(p0, time)
    if not isinstance(reference, ExactSolution):
        solver_error("analytic", f"reference must be an ExactSolution (reference_for, ExactSolution.table), got {type(reference).__name__}")
    if p0.test.eos != "perfect_gas":
        solver_error("analytic", "error norms and fill_exact need the perfect-gas EOS")
    return reference


def spec_of(p0, reference, samples=1, coord_range=None, scale_exp=None):
    return reference.spec(p0.origin, (float(p0.cell_size(0)), float(p0.cell_size(1))), p0.global_grid[0], samples, coord_range, scale_exp)


def tile_windows(tiles, window):
    """The part of the GLOBAL window ``(col0, row0, wnx, wny)`` (0-based real cells of the global grid) that each tile holds, as
    the tile's own ``(col0, row0, wnx, wny)``, or None for a tile the window misses."""
    NX, NY = tiles[0][0].global_grid
    c0, r0, wx, wy = (int(v) for v in window)
    if not (c0 >= 0 and r0 >= 0 and wx >= 1 and wy >= 1 and c0 + wx <= NX and r0 + wy <= NY):
        solver_error("analytic", f"the window {tuple(window)} leaves the global grid {NX} x {NY}")
    out = []
    for params, _ in tiles:
        ox, oy = params.N_origin[0] - 1, params.N_origin[1] - 1
        xa, xb = max(c0, ox), min(c0 + wx, ox + params.N[0])
        ya, yb = max(r0, oy), min(r0 + wy, oy + params.N[1])
        out.append((xa - ox, ya - oy, xb - xa, yb - ya) if xa < xb and ya < yb else None)
    return out


def _run(name, tiles, spec, windows, outs=None):
    """One launch per tile (a tile whose window is None is left out). A table is uploaded once per device, not per tile."""
    tables = {}
    try:
        for i, (params, grid) in enumerate(tiles):
            if windows and windows[i] is None:
                continue
            ptr = None
            if spec.form == TABLE:
                if params.device_id not in tables:
                    tables[params.device_id] = params.device.from_host(np.ascontiguousarray(spec.values).ravel())
                    params.wait()
                ptr = tables[params.device_id].ptr
            col0, row0, wnx, wny = windows[i] if windows else (0, 0, params.N[0], params.N[1])
            args = [params.device.ctx, grid.size.size[0], grid.size.ghosts, params.N[0], params.N[1],
                    *[C.c_void_p(grid.data[f].ptr) for f in ("rho", "u", "v", "E")], col0, row0, wnx, wny,
                    params.N_origin[0] - 1 + col0, params.N_origin[1] - 1 + row0, C.byref(_c_spec(spec, ptr))]
            if outs is not None:
                outs.append(params.device.empty(4 * WORDS, np.uint64))
                check(params.device._L.armon_hip_exact_norms_reset(params.device.ctx, C.c_void_p(outs[-1].ptr)))
                args.append(C.c_void_p(outs[-1].ptr))
            check(params.fn(name)(*args))
        for params, _ in tiles:
            params.wait()
    finally:
        for t in tables.values():
            t.free()


def error_norms_state(tiles, reference=None, time=None, samples=1, coord_range=None, windows=None, scale_exp=None):
    """The distance of the state held by the ``(params, grid)`` of ``tiles`` (idle) from ``reference`` (default: the test case's
    exact solution at ``time``) → ``ErrorNorms``. ``samples``: 1, 2 or 4 points per cell and axis; ``coord_range = (min, max)``:
    only the cells whose centre coordinate lies in it; ``windows``: per tile the ``(col0, row0, wnx, wny)`` of its real cells
    to take; ``scale_exp``: four pairs of exponents instead of the solution's default quanta. Each tile's 512 bytes are read
    back and merged on the host."""
    p0 = tiles[0][0]
    reference = _solution_for(p0, reference, time)
    spec = spec_of(p0, reference, samples, coord_range, scale_exp)
    outs = []
    try:
        _run("exact_norms", tiles, spec, windows, outs)
        raw = neutral()
        for out in outs:
            raw = merge_raw(raw, out.to_host().reshape(4, WORDS))
    finally:
        for out in outs:
            out.free()
    return ErrorNorms(raw, spec.scale_exp, spec.global_nx, spec.samples, time=reference.time if time is None else time)


def fill_state(tiles, reference=None, time=None, samples=1, coord_range=None, windows=None):
    """Write ``reference`` (default: the test case's exact solution at ``time``) into rho, u, v, E of the real cells of every
    tile; ghosts are left to the next sweep's boundary conditions."""
    p0 = tiles[0][0]
    reference = _solution_for(p0, reference, time)
    _run("exact_fill", tiles, spec_of(p0, reference, samples, coord_range), windows)
    return reference


# ---- the run options (error_norms_step, error_norms_at_end, error_norms_samples, error_norms_file) -------------------------
def error_norms_path(params, cycle):
    return os.path.join(params.output_dir, f"{params.error_norms_file}_{cycle:06d}.txt")


def error_norms_run(owner, params, gdt):
    """The error norms of the run ``owner`` (a ``BlockGrid`` or a ``TileGroup``) after ``gdt.cycle`` completed cycles, written to
    ``error_norms_path`` and appended to ``owner.error_norms_taken`` as ``(cycle, time, ErrorNorms)``. Where the test case has no
    solution at that time (a wave has reached a wall) the cycle is listed as ``(cycle, time, None)`` and the run goes on."""
    from .compare import _tiles_of
    from .io import write_error_norms_file
    from ._lib import SolverException
    try:
        reference = reference_for(params, float(gdt.time))
    except SolverException as e:
        # a wave has reached a wall (or the clock stands at 0): no solution to compare with at this cycle. The run goes on;
        # the cycle is listed without norms and no file is written.
        if params.is_root and params.silent < 3:
            print(f"error norms skipped at cycle {gdt.cycle}: {e.msg}")
        owner.error_norms_taken.append((int(gdt.cycle), float(gdt.time), None))
        return None
    norms = error_norms_state(_tiles_of(owner), reference, time=float(gdt.time), samples=params.error_norms_samples)
    norms.cycle, norms.time = int(gdt.cycle), float(gdt.time)
    os.makedirs(params.output_dir, exist_ok=True)
    write_error_norms_file(error_norms_path(params, gdt.cycle), norms, params.output_precision)
    owner.error_norms_taken.append((int(gdt.cycle), float(gdt.time), norms))
    return norms
