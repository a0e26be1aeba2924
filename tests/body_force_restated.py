"""The body-force kick of include/armon_hip.h (armon_hip_body_force) restated in numpy: a plain helper
module, no fixtures. Every operation is written on its own line and evaluated in the data type ``T`` of the arrays — numpy
rounds each of them once and never contracts two into an FMA — so that the result is what the kernel gives, bit for bit.
"""
import numpy as np


def kick(u, v, E, dt, gx, gy):
    """The kick on the arrays ``u, v, E`` (any shape, one dtype ``T``; not modified) → the new ``(u, v, E)``. ``dt, gx, gy``
    are rounded to ``T`` first. A component that is exactly zero leaves its plane alone — the very same array object is
    returned — and out of the energy sum; with both zero all three come back as they are."""
    T = E.dtype.type
    dt, gx, gy = T(dt), T(gx), T(gy)
    if gx == 0 and gy == 0:
        return u, v, E
    half = T(0.5)
    work = None
    u_new, v_new = u, v
    if gx != 0:
        hx = half * dt
        hx = hx * gx
        du = dt * gx
        wx = u + hx
        wx = gx * wx
        work = wx
        u_new = u + du
    if gy != 0:
        hy = half * dt
        hy = hy * gy
        dv = dt * gy
        wy = v + hy
        wy = gy * wy
        work = wy if work is None else work + wy
        v_new = v + dv
    dE = dt * work
    E_new = E + dE
    assert u_new.dtype == u.dtype and v_new.dtype == v.dtype and E_new.dtype == E.dtype
    return u_new, v_new, E_new


def kick_real(fields, nx, ny, g, dt, gx, gy):
    """The kick on the real cells of the flat ghosted arrays ``fields["u"], ["v"], ["E"]`` of a block of nx x ny cells with
    ``g`` ghost layers, IN PLACE; ghost cells and the planes of a zero component are not written."""
    sy, sx = ny + 2 * g, nx + 2 * g
    view = {k: fields[k].reshape(sy, sx)[g:g + ny, g:g + nx] for k in ("u", "v", "E")}
    u, v, E = kick(view["u"], view["v"], view["E"], dt, gx, gy)
    for k, new in (("u", u), ("v", v), ("E", E)):
        if new is not view[k]:
            view[k][...] = new
