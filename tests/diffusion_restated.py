"""The diffusion step of include/armon_hip.h (armon_hip_diffuse) restated in numpy, and a cycle driver built
on it: a plain helper module, no tests, no fixtures.

``step`` works on the real cells as ``(ny, nx)`` arrays of one dtype ``T``. Every operation of the rule is one numpy operation
on arrays or scalars of ``T`` — numpy rounds each once and never contracts two into an FMA — in the order the header writes
them, so the result is what the kernel gives, bit for bit. Cells outside the domain are built by ``extended``: one layer all
round, wrapped on a periodic axis, mirrored otherwise with the side's factors on u and v (both axes independently, so the
factors multiply in a corner).

``run_cycles`` drives whole cycles at a constant step: the oracle's sweeps as tests/scalars_restated.py drives them, then the
sub-steps of ``step``, then the kick of tests/body_force_restated.py.
"""
import math

import numpy as np

SIDES = ("left", "right", "bottom", "top")                 # the ARMON_SIDE_* order
WALL = ((-1., 1.), (-1., 1.), (1., -1.), (1., -1.))        # (u_factor, v_factor) per side of a reflecting wall
FREE = ((1., 1.),) * 4                                     # and of a FreeFlow side


def source_index(n, periodic):
    """For the indices -1 .. n of an axis of ``n`` cells: the real cell that stands for each, and 0 / 1 / 2 = inside / beyond
    the low side / beyond the high side of a non-periodic axis."""
    i = np.arange(-1, n + 1)
    if periodic:
        return i % n, np.zeros(n + 2, dtype=int)
    src = np.where(i < 0, -1 - i, np.where(i >= n, 2 * n - 1 - i, i))
    return src, np.where(i < 0, 1, np.where(i >= n, 2, 0))


def extended(a, periodic, fx=(1., 1.), fy=(1., 1.)):
    """``a`` (ny, nx) with one layer of outside cells all round → (ny + 2, nx + 2); ``fx = (low, high)`` the factors of the x
    sides, ``fy`` of the y sides (not used on a periodic axis)."""
    T = a.dtype.type
    ny, nx = a.shape
    sx, ox = source_index(nx, periodic[0])
    sy, oy = source_index(ny, periodic[1])
    b = a[np.ix_(sy, sx)].copy()
    for side in (1, 2):
        b[:, ox == side] = b[:, ox == side] * T(fx[side - 1])
    for side in (1, 2):
        b[oy == side, :] = b[oy == side, :] * T(fy[side - 1])
    return b


def step(rho, u, v, E, phis, dt, dx, dy, nu, chi, Ds, periodic=(False, False), factors=WALL):
    """One step of length ``dt``. ``rho, u, v, E``: (ny, nx) arrays of one dtype; ``phis``: a list of such planes with their
    diffusivities ``Ds``; ``factors[side] = (u_factor, v_factor)`` in the ``SIDES`` order. Nothing is modified. Returns
    ``(u', v', E', [phi'])``; with nu = chi = 0 the state is not evaluated and u, v, E come back as they are."""
    T = rho.dtype.type
    assert all(a.dtype == rho.dtype for a in [u, v, E] + list(phis)) and len(phis) == len(Ds)
    dt, nu, chi = T(dt), T(nu), T(chi)
    idx, idy = T(1) / T(dx), T(1) / T(dy)
    q4x, q4y = T(0.25) * idx, T(0.25) * idy
    c43, c23, half = T(4) / T(3), T(2) / T(3), T(0.5)
    state = nu != 0 or chi != 0
    fux, fvx = (factors[0][0], factors[1][0]), (factors[0][1], factors[1][1])
    fuy, fvy = (factors[2][0], factors[3][0]), (factors[2][1], factors[3][1])
    R = extended(rho, periodic)
    P = [extended(p, periodic) for p in phis]
    # slices of the extended arrays: C = the real cells; the faces of an axis run from the low face of the first real cell
    # to the high face of the last one
    xL, xR = np.s_[1:-1, 0:-1], np.s_[1:-1, 1:]          # the cells left and right of every x-face of the real rows
    yL, yR = np.s_[0:-1, 1:-1], np.s_[1:, 1:-1]          # the cells below and above every y-face of the real columns
    rfx = half * (R[xL] + R[xR])
    rfy = half * (R[yL] + R[yR])
    F, G = {}, {}
    if state:
        U, V = extended(u, periodic, fux, fuy), extended(v, periodic, fvx, fvy)
        Ee = extended(E, periodic)
        e = Ee - half * (U * U + V * V)
        # x-faces
        mu = nu * rfx
        ux = (U[xR] - U[xL]) * idx
        vx = (V[xR] - V[xL]) * idx
        uy = ((U[2:, 0:-1] - U[:-2, 0:-1]) + (U[2:, 1:] - U[:-2, 1:])) * q4y
        vy = ((V[2:, 0:-1] - V[:-2, 0:-1]) + (V[2:, 1:] - V[:-2, 1:])) * q4y
        txx = mu * (c43 * ux - c23 * vy)
        txy = mu * (uy + vx)
        uf = half * (U[xL] + U[xR])
        vf = half * (V[xL] + V[xR])
        q = (chi * rfx) * ((e[xR] - e[xL]) * idx)
        F["u"], F["v"], F["E"] = txx, txy, (uf * txx + vf * txy) + q
        # y-faces
        mu = nu * rfy
        uy = (U[yR] - U[yL]) * idy
        vy = (V[yR] - V[yL]) * idy
        ux = ((U[0:-1, 2:] - U[0:-1, :-2]) + (U[1:, 2:] - U[1:, :-2])) * q4x
        vx = ((V[0:-1, 2:] - V[0:-1, :-2]) + (V[1:, 2:] - V[1:, :-2])) * q4x
        tyy = mu * (c43 * vy - c23 * ux)
        txy = mu * (uy + vx)
        uf = half * (U[yL] + U[yR])
        vf = half * (V[yL] + V[yR])
        q = (chi * rfy) * ((e[yR] - e[yL]) * idy)
        G["u"], G["v"], G["E"] = txy, tyy, (uf * txy + vf * tyy) + q
    k = dt / rho

    def update(a, f, g):
        return a + k * ((f[:, 1:] - f[:, :-1]) * idx + (g[1:, :] - g[:-1, :]) * idy)

    new_phis = []
    for p, Pe, D in zip(phis, P, Ds):
        D = T(D)
        f = (D * rfx) * ((Pe[xR] - Pe[xL]) * idx)
        g = (D * rfy) * ((Pe[yR] - Pe[yL]) * idy)
        new_phis.append(update(p, f, g))
    if not state:
        return u, v, E, new_phis
    out = [update(a, F[n], G[n]) for n, a in (("u", u), ("v", v), ("E", E))]
    assert all(a.dtype == rho.dtype for a in out + new_phis)
    return out[0], out[1], out[2], new_phis


def substeps(dt, dx, dy, nu, chi, Ds, sigma=0.5):
    """The number of equal steps a cycle of step ``dt`` is diffused in: max(1, ceil(dt·2·κ·(1/dx² + 1/dy²)/σ)) in Python floats."""
    kappa = max([4. * float(nu) / 3., float(chi)] + [float(D) for D in Ds])
    dx, dy = float(dx), float(dy)
    return max(1, math.ceil(float(dt) * 2. * kappa * (1. / (dx * dx) + 1. / (dy * dy)) / sigma))


def run_cycles(fields, planes, Ds, nx, ny, g, order, cycles, dt, sizes, scheme, limiter, projection, eos, dtype, nu, chi,
               sigma=0.5, gravity=(0., 0.), periodic=(False, False), factors=WALL):
    """``cycles`` cycles at the constant step ``dt`` of the flat ghosted state ``fields`` and its flat ghosted ``planes`` (with
    the diffusivities ``Ds``, 0 = the plane is advected only) on a lone block of nx x ny cells with ``g`` ghost layers: the
    sweeps of ``order(cycle)`` as ``scalars_restated.run_cycles`` drives them, then ``substeps`` steps of length T(dt)/T(n) on
    the real cells, then the kick of ``gravity``. ``factors`` as in ``step``; a wall's sweep mirrors with the factors (along,
    across) = (its normal velocity's, its transverse one's). Returns ``(planes, state, launches)``: flat ghosted arrays of
    which the real cells are meaningful, and the number of diffusion steps applied."""
    from body_force_restated import kick_real
    from scalars_restated import restated_sweep, wrap_periodic
    from sweep_reference import STATE
    T = np.dtype(dtype).type
    f = {k: fields[k].copy() for k in STATE}
    ps = [p.copy() for p in planes]
    walls = {0: ((factors[0][0], factors[0][1]), (factors[1][0], factors[1][1])),
             1: ((factors[2][1], factors[2][0]), (factors[3][1], factors[3][0]))}
    real = lambda a: a.reshape(ny + 2 * g, nx + 2 * g)[g:g + ny, g:g + nx]
    diffusing = [k for k, D in enumerate(Ds) if float(T(D)) != 0]
    anything = float(T(nu)) != 0 or float(T(chi)) != 0 or bool(diffusing)
    launches = 0
    for cycle in range(cycles):
        for axis, factor in order(cycle):
            bc = 0 if periodic[axis] else 1
            if periodic[axis]:
                f = {k: wrap_periodic(f[k], nx, ny, g, axis) for k in STATE}
                ps = [wrap_periodic(p, nx, ny, g, axis) for p in ps]
            f_low, f_high = walls[axis]
            ps, f = restated_sweep(f, ps, nx, ny, g, axis, scheme, limiter, projection, eos, float(T(dt) * T(factor)),
                                   float(sizes[axis]), bc, bc, f_low, f_high, dtype)
        if anything:
            n = substeps(T(dt), sizes[0], sizes[1], T(nu), T(chi), [T(Ds[k]) for k in diffusing], sigma)
            h = T(dt) / T(n)
            for _ in range(n):
                u, v, E, new = step(real(f["rho"]), real(f["u"]), real(f["v"]), real(f["E"]), [real(ps[k]) for k in diffusing], h,
                                    sizes[0], sizes[1], nu, chi, [Ds[k] for k in diffusing], periodic, factors)
                u, v, E = u.copy(), v.copy(), E.copy()
                real(f["u"])[...], real(f["v"])[...], real(f["E"])[...] = u, v, E
                for k, a in zip(diffusing, new):
                    real(ps[k])[...] = a
                launches += 1
        kick_real(f, nx, ny, g, T(dt), gravity[0], gravity[1])
    return ps, f, launches
