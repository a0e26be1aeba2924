"""The rule of ``armon_hip_init_regions`` restated for the tests in numpy, from its specification (DESIGN §4.11,
include/armon_hip.h) — never from csrc/init_regions.hip, which it is there to check. Everything is evaluated in the run's
dtype, one numpy operation per operation written.

    corner   x = T(gx) dXx + ox                    samples  xs_i = x + dXx T((2 i + 1) / (2 samples))
    HALF_PLANE  a0 xs + a1 ys <= a2                BOX      a0 <= xs <= a1 and a2 <= ys <= a3
    DISC        (xs-a0)(xs-a0) + (ys-a1)(ys-a1) <= a2
    ELLIPSE     (xs-a0)(xs-a0) a2 + (ys-a1)(ys-a1) a3 <= 1
    a point belongs to the LAST region that holds it, else to the background
    all samples in one region: its state verbatim; else m += rho, mu += rho u, mv += rho v, mE += rho E (y outer, x inner),
    rho = m / T(samples²), u = mu / m, v = mv / m, E = mE / m
"""
import numpy as np

HALF_PLANE, BOX, DISC, ELLIPSE = 0, 1, 2, 3


def holds(kind, a, xs, ys, T):
    a0, a1, a2, a3 = (T(v) for v in a)
    if kind == HALF_PLANE:
        return a0 * xs + a1 * ys <= a2
    if kind == BOX:
        return (a0 <= xs) & (xs <= a1) & (a2 <= ys) & (ys <= a3)
    if kind == DISC:
        return (xs - a0) * (xs - a0) + (ys - a1) * (ys - a1) <= a2
    if kind == ELLIPSE:
        return (xs - a0) * (xs - a0) * a2 + (ys - a1) * (ys - a1) * a3 <= T(1)
    raise ValueError(kind)


def owner(regions, xs, ys, T):
    """Index of the region each point belongs to, -1 for the background."""
    hit = np.full(np.broadcast(xs, ys).shape, -1, dtype=np.int64)
    for k in range(len(regions) - 1, -1, -1):           # from the back: the first hit is kept
        inside = holds(regions[k][0], regions[k][1], xs, ys, T)
        hit = np.where((hit < 0) & inside, k, hit)
    return hit


def restate(gx, gy, origin, dX, samples, background, regions, dtype):
    """``gx, gy``: 1-D integer arrays of global cell positions; ``regions`` = [(kind, (a0..a3), (rho, u, v, E))] →
    rho, u, v, E as ``(len(gy), len(gx))`` arrays of ``dtype`` and the mask of the mixed cells."""
    T = np.dtype(dtype).type
    dXx, dXy, ox, oy = T(dX[0]), T(dX[1]), T(origin[0]), T(origin[1])
    x = np.asarray(gx, dtype=np.int64).astype(T) * dXx + ox
    y = np.asarray(gy, dtype=np.int64).astype(T) * dXy + oy
    states = [tuple(T(v) for v in background)] + [tuple(T(v) for v in s) for _, _, s in regions]     # index hit + 1
    table = [np.array([s[q] for s in states], dtype=T) for q in range(4)]
    shape = (len(y), len(x))
    m, mu, mv, mE = (np.zeros(shape, dtype=T) for _ in range(4))
    first, mixed, last = None, np.zeros(shape, dtype=bool), None
    with np.errstate(all="ignore"):
        for sy in range(samples):
            ys = (y + dXy * T((2 * sy + 1) / (2 * samples)))[:, None]
            for sx in range(samples):
                xs = (x + dXx * T((2 * sx + 1) / (2 * samples)))[None, :]
                hit = owner(regions, xs, ys, T)
                rho, u, v, E = (t[hit + 1] for t in table)
                if first is None:
                    first = hit
                mixed |= hit != first
                m = m + rho
                mu = mu + rho * u
                mv = mv + rho * v
                mE = mE + rho * E
                last = (rho, u, v, E)
        mix = (m / T(samples * samples), mu / m, mv / m, mE / m)
    out = tuple(np.where(mixed, a, b).astype(T) for a, b in zip(mix, last))
    return out + (mixed,)


def block(N, nghost, global_pos=(0, 0)):
    """Global positions of the cells of a ghosted block of ``N = (nx, ny)`` real cells whose first real cell is
    ``global_pos`` → gx, gy."""
    return (np.arange(-nghost, N[0] + nghost, dtype=np.int64) + global_pos[0],
            np.arange(-nghost, N[1] + nghost, dtype=np.int64) + global_pos[1])
