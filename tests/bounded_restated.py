"""The bound-preserving scalar sweep restated (test infrastructure: a plain helper module, no tests).

Built like tests/scalars_restated.py. The STATE's part is the oracle's: ``bounded_sweep`` composes its per-step functions as
``sweep_reference.reference_sweep`` does — EOS, mirror, fluxes, ``cell_update``, ``advection_*``, ``euler_projection`` on the
true state — and takes from them the Lagrangian density, the interface velocities, the mass fluxes ``a_rho`` and the new
density. The PLANES' part is plain numpy in the run's data type, one IEEE operation per operation written, in the order
include/armon_hip.h states for ``armon_hip_sweep_scalars_bounded``; maxima, minima and the sign are taken by comparisons as
csrc/physics.hpp takes them. A wall mirrors the plane with factor +1; a side with ``bc = 0`` reads the ghosts given.
``run_cycles`` drives whole cycles as ``scalars_restated.run_cycles`` does and reports how far the value before the clamp
ever lay outside the clamp's bounds.
"""
import numpy as np

from oracle import oracle as O
from scalars_restated import mirror_plus, wrap_periodic
from sweep_reference import GAMMA, STATE, uv_factors


def state_stages(fields, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, bc_low, bc_high, f_low, f_high, dtype):
    """The oracle's stages of one sweep of the state ``fields`` (the arguments of ``reference_sweep``). Returns
    ``(rho_lag, us, a_rho, new state)``: flat ghosted arrays — the Lagrangian density (valid w cells past the real ones), the
    final interface velocities, the mass fluxes of the interfaces 0 … n of every line — and the new state as a dict."""
    dtype = np.dtype(dtype)
    L = O.lib(f32=dtype == np.float32)
    L.armon_oracle_set_threads(1)
    P = O.ptr
    X = axis == 0
    s = 1 if X else nx + 2 * g
    w = 2 if projection == "euler_2nd" else 1
    n = nx if X else ny
    d = O.alloc_fields(nx, ny, g, dtype=dtype.type)
    for k in STATE:
        assert fields[k].dtype == dtype and fields[k].size == d[k].size
        d[k][:] = fields[k]
    ua = d["u"] if X else d["v"]

    def along(lo, hi):
        return O.domain_range(nx, ny, g, (lo, 0), (hi - n, 0)) if X else O.domain_range(nx, ny, g, (0, lo), (0, hi - n))

    eos_r = along(0 if bc_low else -g, n if bc_high else n + g)
    if eos == "bizarrium":
        L.armon_oracle_bizarrium_EOS(eos_r, *(P(d[k]) for k in ("rho", "u", "v", "E", "p", "c", "g")))
    else:
        L.armon_oracle_perfect_gas_EOS(eos_r, GAMMA, *(P(d[k]) for k in ("rho", "E", "u", "v", "p", "c", "g")))
    for high, on, (fa, ft) in ((0, bc_low, f_low), (1, bc_high, f_high)):
        if not on:
            continue
        border = along(n - 1, n) if high else along(0, 1)
        uf, vf = uv_factors(axis, (fa, ft))
        L.armon_oracle_boundary_conditions(border, s if high else -s, g, uf, vf,
                                           *(P(d[k]) for k in ("rho", "u", "v", "p", "c", "g", "E")))
    fl, cu, ad, pr = along(-w, n + w + 1), along(-w, n + w), along(0, n + 1), along(0, n)
    if scheme == "GAD":
        L.armon_oracle_acoustic_GAD(fl, s, dt, dx, P(d["us"]), P(d["ps"]), P(d["rho"]), P(ua), P(d["p"]), P(d["c"]),
                                    O.LIMITERS[limiter])
    else:
        L.armon_oracle_acoustic(fl, s, P(d["us"]), P(d["ps"]), P(d["rho"]), P(ua), P(d["p"]), P(d["c"]))
    L.armon_oracle_cell_update(cu, s, dx, dt, P(d["us"]), P(d["ps"]), P(d["rho"]), P(ua), P(d["E"]))
    rho_lag = d["rho"].copy()
    adv = [P(d[k]) for k in ("us", "rho", "u", "v", "E", "work_1", "work_2", "work_3", "work_4")]
    if projection == "euler_2nd":
        L.armon_oracle_advection_second_order(ad, s, dx, dt, *adv)
    else:
        L.armon_oracle_advection_first_order(ad, s, dt, *adv)
    L.armon_oracle_euler_projection(pr, s, dx, dt, *adv)
    return rho_lag, d["us"].copy(), d["work_1"].copy(), {k: d[k].copy() for k in STATE}


def _mx(x, y):
    return np.where(y > x, y, x)          # phys::mx


def _mn(x, y):
    return np.where(y > x, x, y)          # phys::mn


def slope_minmod(um, u0, up):
    """phys::slope_minmod with both ratios 1: a plain minmod of the two differences."""
    Dp = up - u0
    Dm = u0 - um
    sg = np.where(Dp > 0, Dp.dtype.type(1), np.where(Dp < 0, Dp.dtype.type(-1), Dp))
    return sg * _mx(np.zeros_like(Dp), _mn(sg * Dp, sg * Dm))


def bounded_sweep(fields, planes, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, bc_low, bc_high, f_low, f_high, dtype):
    """One sweep along ``axis`` (0 = x, 1 = y) of the planes under the bounded rule; the arguments and the first and last
    result are those of ``scalars_restated.restated_sweep``. Returns ``(new planes, planes before the clamp, new state)``;
    only the real cells of the planes are meaningful."""
    dtype = np.dtype(dtype)
    T = dtype.type
    rho_lag, us, a_rho, state = state_stages(fields, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, bc_low, bc_high,
                                             f_low, f_high, dtype)
    shape = (ny + 2 * g, nx + 2 * g)
    ax = 1 if axis == 0 else 0

    def at(a, k):                          # a[i + k] at i (what wraps around lands in the outermost ghosts only)
        return np.roll(a, -k, axis=ax)

    rho_lag, us, a_rho, rho_new = (a.reshape(shape) for a in (rho_lag, us, a_rho, state["rho"]))
    dt, dx = T(dt), T(dx)
    out, raw = [], []
    with np.errstate(all="ignore"):        # (cells the stages never reach hold zeros: 0 / 0 outside the real cells)
        m = (dx + dt * (at(us, 1) - us)) * rho_lag
        up = dt * us > 0
        m_d = np.where(up, at(m, -1), m)
        h = T(0.5) * (T(1) - np.abs(a_rho) / m_d)
        for plane in planes:
            assert plane.dtype == dtype and plane.size == rho_lag.size
            f = mirror_plus(plane, nx, ny, g, axis, bc_low, bc_high).reshape(shape)
            fm, fp = at(f, -1), at(f, 1)
            if projection == "euler_2nd":
                sig = slope_minmod(fm, f, fp)
                A = a_rho * np.where(up, fm + at(sig, -1) * h, f - sig * h)
            else:
                A = a_rho * np.where(up, fm, f)
            t_q = (m * f - (at(A, 1) - A)) / dx
            v = t_q / rho_new
            lo, hi = _mn(_mn(fm, f), fp), _mx(_mx(fm, f), fp)
            out.append(np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(dtype).ravel())
            raw.append(v.astype(dtype).ravel())
    return out, raw, state


def clamp_excess(plane, raw, new, nx, ny, g, axis, bc_low, bc_high):
    """How far ``raw`` (before the clamp) lies outside the clamp's bounds — the smallest and largest of φ at i−1, i, i+1 of the
    mirrored input ``plane`` — at most, over the real cells; 0 where it lies inside. ``new`` is only checked against it."""
    shape = (ny + 2 * g, nx + 2 * g)
    ax = 1 if axis == 0 else 0
    f = mirror_plus(plane, nx, ny, g, axis, bc_low, bc_high).reshape(shape)
    fm, fp = np.roll(f, 1, axis=ax), np.roll(f, -1, axis=ax)
    lo, hi = np.minimum(np.minimum(fm, f), fp), np.maximum(np.maximum(fm, f), fp)
    real = (slice(g, g + ny), slice(g, g + nx))
    r, o = raw.reshape(shape)[real].astype(np.float64), new.reshape(shape)[real]
    assert ((o >= lo[real]) & (o <= hi[real])).all()
    return float(np.maximum(np.maximum(lo[real] - r, r - hi[real]), 0.).max())


def run_cycles(fields, planes, nx, ny, g, order, cycles, dt, sizes, scheme, limiter, projection, eos, dtype, walls, periodic=(False, False)):
    """``scalars_restated.run_cycles`` under the bounded rule. Returns ``(planes, state, excess)``: ``excess`` is the largest
    ``clamp_excess`` of any plane in any sweep."""
    T = np.dtype(dtype).type
    f = {k: fields[k].copy() for k in STATE}
    ps = [p.copy() for p in planes]
    excess = 0.
    for cycle in range(cycles):
        for axis, factor in order(cycle):
            bc = 0 if periodic[axis] else 1
            if periodic[axis]:
                f = {k: wrap_periodic(f[k], nx, ny, g, axis) for k in STATE}
                ps = [wrap_periodic(p, nx, ny, g, axis) for p in ps]
            f_low, f_high = walls[axis]
            new, raw, f = bounded_sweep(f, ps, nx, ny, g, axis, scheme, limiter, projection, eos, float(T(dt) * T(factor)),
                                        float(sizes[axis]), bc, bc, f_low, f_high, dtype)
            excess = max([excess] + [clamp_excess(p, r, o, nx, ny, g, axis, bc, bc) for p, r, o in zip(ps, raw, new)])
            ps = new
    return ps, f, excess


# ---- the inputs of the single-launch GPU tests (tests/test_gpu_bounded.py), which tests/test_bounded_host.py checks first ----
CONFIGS = [("GAD", "minmod", "euler_2nd", "perfect_gas"), ("Godunov", "minmod", "euler", "bizarrium")]
# X: odd pitch, clamped path, partial strip; the 16-B path, more than one strip; the smallest block (None: LAG x LAG).
# Y: partial lane group, more than one run; three lane groups.
SHAPES = [(0, (123, 5), 5), (0, (250, 9), 4), (0, None, 4), (1, (70, 101), 5), (1, (530, 37), 4)]
BCS = [(1, 1), (0, 0)]


def launch_inputs(axis, shape, g, config, dtype, ns=4):
    """``(nx, ny, state, planes, dt, dx)`` of one single-launch case: ``rand_state``, ``rand_planes`` and ``case_numbers`` of
    tests/scalars_harness.py under a seed of the shape."""
    from scalars_harness import case_numbers, lag_of, rand_planes
    from sweep_reference import rand_state
    scheme, _, projection, eos = config
    nx, ny = shape if shape is not None else (lag_of(scheme, projection),) * 2
    seed = 1717 + 31 * nx + ny
    dt, dx = case_numbers(nx, ny, axis, eos, dtype)
    return nx, ny, rand_state(nx, ny, g, eos, dtype, seed), rand_planes(nx, ny, g, ns, dtype, seed + 1), dt, dx
