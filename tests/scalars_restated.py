"""The passive-scalar sweep restated with the CPU oracle (test infrastructure: a plain helper module, no tests).

A passive scalar is "one more transverse velocity that does not enter the EOS" (include/armon_hip.h). So
``restated_sweep`` composes the oracle's per-step functions exactly as ``sweep_reference.reference_sweep`` does — EOS, mirror,
fluxes and ``cell_update`` on the TRUE state — and then runs ``advection_*`` and ``euler_projection`` once per plane with the
plane standing in the slot of the transverse velocity (v for an X sweep, u for a Y sweep), which the Lagrangian phase never
touches. A wall mirrors the plane with factor +1 whatever the velocity factors; a side with ``bc = 0`` reads the ghosts
given. ``run_cycles`` drives whole cycles (a ``split_axes`` order, constant dt) for a state and its planes, wrapping a
periodic axis with numpy. tests/test_scalars_host.py ties the restatement to ``reference_sweep``: with φ = ut it gives the
oracle's own ut, bit for bit.
"""
import numpy as np

from oracle import oracle as O
from sweep_reference import GAMMA, STATE, uv_factors


def mirror_plus(plane, nx, ny, g, axis, bc_low, bc_high):
    """``plane`` (flat, ghosted) with the ghosts of the mirrored sides of ``axis`` set to the mirrored real cells, factor +1."""
    a = plane.reshape(ny + 2 * g, nx + 2 * g).copy()
    v = a if axis == 1 else a.T                      # v[i] = layer i along the axis (a view either way)
    n = ny if axis == 1 else nx
    for k in range(g):
        if bc_low:
            v[g - 1 - k] = v[g + k]
        if bc_high:
            v[g + n + k] = v[g + n - 1 - k]
    return a.ravel()


def wrap_periodic(plane, nx, ny, g, axis):
    """``plane`` with the ghosts of both sides of ``axis`` taken from the real cells of the opposite border."""
    a = plane.reshape(ny + 2 * g, nx + 2 * g).copy()
    v = a if axis == 1 else a.T
    n = ny if axis == 1 else nx
    v[:g] = v[n:n + g]
    v[g + n:] = v[g:2 * g]
    return a.ravel()


def restated_sweep(fields, planes, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, bc_low, bc_high, f_low, f_high, dtype):
    """One sweep along ``axis`` (0 = x, 1 = y) of the planes ``planes`` (a list of flat ghosted arrays) carried by the state
    ``fields`` (flat ghosted rho, u, v, E); nothing is modified. The arguments are those of ``reference_sweep``. Returns
    ``(new planes, new state)``: flat ghosted arrays of which only the real cells are meaningful, the state as a dict."""
    dtype = np.dtype(dtype)
    L = O.lib(f32=dtype == np.float32)
    L.armon_oracle_set_threads(1)
    P = O.ptr
    X = axis == 0
    row = nx + 2 * g
    s = 1 if X else row
    w = 2 if projection == "euler_2nd" else 1
    n = nx if X else ny
    d = O.alloc_fields(nx, ny, g, dtype=dtype.type)
    for k in STATE:
        assert fields[k].dtype == dtype and fields[k].size == d[k].size
        d[k][:] = fields[k]
    ua, t_name = (d["u"], "v") if X else (d["v"], "u")

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

    lagrangian = {k: d[k].copy() for k in STATE}           # the remap overwrites rho, u, v, E: every plane starts from this
    adv = [P(d[k]) for k in ("us", "rho", "u", "v", "E", "work_1", "work_2", "work_3", "work_4")]

    def remap(transverse):
        for k in STATE:
            d[k][:] = lagrangian[k]
        if transverse is not None:
            d[t_name][:] = transverse
        if projection == "euler_2nd":
            L.armon_oracle_advection_second_order(ad, s, dx, dt, *adv)
        else:
            L.armon_oracle_advection_first_order(ad, s, dt, *adv)
        L.armon_oracle_euler_projection(pr, s, dx, dt, *adv)

    out = []
    for plane in planes:
        assert plane.dtype == dtype and plane.size == d["rho"].size
        remap(mirror_plus(plane, nx, ny, g, axis, bc_low, bc_high))
        out.append(d[t_name].copy())
    remap(None)
    return out, {k: d[k].copy() for k in STATE}


def run_cycles(fields, planes, nx, ny, g, order, cycles, dt, sizes, scheme, limiter, projection, eos, dtype, walls, periodic=(False, False)):
    """``cycles`` cycles at the constant step ``dt`` of the state ``fields`` and its ``planes`` on a lone block: ``order(cycle)``
    gives the sweeps of a cycle as ``(axis, dt_factor)`` with axis 0 / 1 (``solver.split_axes`` with its ``Axis`` mapped),
    ``sizes = (dx, dy)``, ``walls[axis] = (f_low, f_high)`` the mirror factors (along, across) of a walled axis. A periodic axis
    is wrapped with numpy before its sweeps and swept with bc = 0. The step of a sweep is ``T(dt) * T(factor)`` as in the
    solver. Returns ``(planes, state)`` as ``restated_sweep`` does."""
    T = np.dtype(dtype).type
    f = {k: fields[k].copy() for k in STATE}
    ps = [p.copy() for p in planes]
    for cycle in range(cycles):
        for axis, factor in order(cycle):
            bc = 0 if periodic[axis] else 1
            if periodic[axis]:
                f = {k: wrap_periodic(f[k], nx, ny, g, axis) for k in STATE}
                ps = [wrap_periodic(p, nx, ny, g, axis) for p in ps]
            f_low, f_high = walls[axis]
            ps, f = restated_sweep(f, ps, nx, ny, g, axis, scheme, limiter, projection, eos, float(T(dt) * T(factor)),
                                   float(sizes[axis]), bc, bc, f_low, f_high, dtype)
    return ps, f
