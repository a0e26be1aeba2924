"""Derived flow fields and in-situ images (csrc/derive.hip): what a run is looked at with — a numerical schlieren, the
vorticity, the velocity divergence, the Mach number — computed where the state lives and reduced over the coarse cells of
``coarsen``. No reference counterpart: the reference writes whole fields (ref src/io.jl:2-27).

PER CELL, all arithmetic in the data type T, one IEEE operation per operation written:

    e          = E - 0.5 (u u + v v)
    p, c       = the EOS of the cell itself (perfect gas: p = (gamma - 1) rho e, c = sqrt((gamma p) / rho)); no p vector is read
    speed      = sqrt(u u + v v),   mach = speed / c
    d_x f      = (f_R - f_L) / (T(w) dx)   f_R = f[i+1] if that cell exists, else f[i]; f_L likewise; w = how many of the two
                 exist (w = 0: the derivative is 0); d_y likewise with dy. A neighbour exists if it is a real cell of the tile
                 or the neighbour tile's cell in the first ghost layer: central differences inside and across tile edges,
                 one-sided ones at the edge of the global domain
    grad_rho   = sqrt(gx gx + gy gy),   vorticity = d_x v - d_y u,   divergence = d_x u + d_y v

Each quantity is reduced over the ``fx x fy`` coarse cells: ``mean`` (the sum in the summation order of ``coarsen`` divided by
the cells covered), ``max`` or ``min``; a NaN among the covered values gives NaN. With exact per-cell arithmetic and that fixed
order the planes of a tile group equal the single block's bit for bit. ``reference_planes`` restates the per-cell rule in numpy;
the tests hold the kernel against it.
"""
import ctypes as C
import os

import numpy as np

from ._lib import DeriveSpec, check, solver_error

QUANTITIES = ("rho", "p", "e", "speed", "mach", "grad_rho", "vorticity", "divergence")      # ARMON_DERIVE_*, in order
REDUCTIONS = ("mean", "max", "min")                                                         # ARMON_REDUCE_*, in order
TRANSFERS = ("linear", "log", "schlieren")
MAX_PLANES = 8
SCHLIEREN_K = 15.0
LEFT, RIGHT, BOTTOM, TOP = 1, 2, 4, 8


# ---- the rule, in numpy (the tests' oracle) --------------------------------------------------------------------------------
def _diff(f, axis, d, T):
    """``d_axis f`` of the 2-D array ``f`` whose every cell is real and whose edges are edges of the domain."""
    n = f.shape[axis]
    hi, lo = np.roll(f, -1, axis), np.roll(f, 1, axis)
    idx = np.arange(n).reshape((-1, 1) if axis == 0 else (1, -1))
    has_hi, has_lo = np.broadcast_to(idx + 1 < n, f.shape), np.broadcast_to(idx > 0, f.shape)
    hi, lo = np.where(has_hi, hi, f), np.where(has_lo, lo, f)
    w = has_hi.astype(np.int64) + has_lo
    den = np.where(w == 2, T(2) * T(d), T(d)).astype(T)
    with np.errstate(all="ignore"):
        return np.where(w == 0, T(0), (hi - lo) / den).astype(T)


def reference_planes(rho, u, v, E, dx, dy, gamma):
    """Every quantity of ``QUANTITIES`` for the ``(ny, nx)`` arrays of a WHOLE domain (perfect gas) → dict name → array of the
    arrays' type. One numpy operation per operation of the rule: numpy's +, -, *, / and sqrt are the IEEE ones."""
    T = rho.dtype.type
    with np.errstate(all="ignore"):
        e = E - T(0.5) * (u * u + v * v)
        p = (T(gamma) - T(1)) * rho * e
        c = np.sqrt((T(gamma) * p) / rho)
        speed = np.sqrt(u * u + v * v)
        gx, gy = _diff(rho, 1, dx, T), _diff(rho, 0, dy, T)
        out = {"rho": rho, "p": p, "e": e, "speed": speed, "mach": speed / c, "grad_rho": np.sqrt(gx * gx + gy * gy),
               "vorticity": _diff(v, 1, dx, T) - _diff(u, 0, dy, T), "divergence": _diff(u, 1, dx, T) + _diff(v, 0, dy, T)}
    return {k: np.asarray(a, dtype=rho.dtype) for k, a in out.items()}


# ---- device side -----------------------------------------------------------------------------------------------------------
SCALAR_QUANTITY = "scalar:"       # "scalar:<name>": the plane of a passive scalar, reduced like rho


def normalize_request(quantities, reduce="mean", scalars=None):
    """``quantities``: a name or a list of at most 8 distinct names of ``QUANTITIES`` or ``"scalar:<name>"``; ``reduce``: one
    name of ``REDUCTIONS`` or a dict quantity → name (``mean`` where the dict is silent) → ``(names, reductions)``.
    ``scalars``: the names of the run's passive scalars (None: any name passes here)."""
    names = (quantities,) if isinstance(quantities, str) else tuple(quantities)
    if not 1 <= len(names) <= MAX_PLANES:
        solver_error("config", f"derive takes 1 to {MAX_PLANES} quantities, got {len(names)}")
    for q in names:
        if isinstance(q, str) and q.startswith(SCALAR_QUANTITY):
            if scalars is not None and q[len(SCALAR_QUANTITY):] not in scalars:
                solver_error("config", f"unknown derived quantity {q!r}: this run carries the scalars {tuple(scalars)!r}")
            continue
        if q not in QUANTITIES:
            solver_error("config", f"unknown derived quantity {q!r}: one of {', '.join(QUANTITIES)} or 'scalar:<name>'")
    if len(set(names)) != len(names):
        solver_error("config", f"a derived quantity may be asked for once, got {names!r}")
    if isinstance(reduce, dict):
        for q in reduce:
            if q not in names:
                solver_error("config", f"reduce names {q!r}, which is not among the quantities {names!r}")
        modes = tuple(reduce.get(q, "mean") for q in names)
    else:
        modes = (reduce,) * len(names)
    for m in modes:
        if m not in REDUCTIONS:
            solver_error("config", f"unknown reduction {m!r}: one of {', '.join(REDUCTIONS)}")
    return names, modes


def _c_spec(params, names, modes, neighbours):
    s = DeriveSpec()
    s.nq = len(names)
    for k, (q, m) in enumerate(zip(names, modes)):
        s.quantity[k], s.reduce[k] = QUANTITIES.index(q), REDUCTIONS.index(m)
    s.eos = 1 if params.test.eos == "bizarrium" else 0
    s.neighbours = int(neighbours)
    s.gamma, s.dx, s.dy = float(params.test.gamma), float(params.cell_size(0)), float(params.cell_size(1))
    return s


def tile_neighbours(params):
    """The bits of the sides of a tile behind which another tile lies."""
    from .blocking import Side
    from .parameters import PROC_NULL
    return sum(bit for side, bit in ((Side.Left, LEFT), (Side.Right, RIGHT), (Side.Bottom, BOTTOM), (Side.Top, TOP))
               if params.neighbours[side] != PROC_NULL)


def derive_state(tiles, quantities, factor=1, reduce="mean", neighbours=None):
    """The derived fields of the state held by the ``(params, grid)`` of ``tiles`` (idle; the first ghost layer of every side
    with a neighbour tile holds that tile's cells: ``TileGroup.derive`` sees to it) → dict name → ``(cny, cnx)`` array of the
    GLOBAL coarse grid. Every tile must start on a coarse-cell boundary (``check_coarsen_alignment``). ``neighbours``: per tile
    the bits to use instead of the tile's own topology. Only the coarse planes cross PCIe."""
    from .parameters import check_coarsen_alignment, coarse_shape, normalize_coarsen_factor
    names, modes = normalize_request(quantities, reduce, scalars=tiles[0][0].scalar_names)
    factor = normalize_coarsen_factor(factor)
    if factor is None:
        solver_error("config", "derive needs a factor >= 1")
    for params, _ in tiles:
        check_coarsen_alignment(params, factor)
    fx, fy = factor
    p0 = tiles[0][0]
    gcnx, gcny = coarse_shape(p0.global_grid, factor)
    res = {q: np.empty((gcny, gcnx), dtype=p0.data_type) for q in names}
    outs = []
    try:
        for i, (params, grid) in enumerate(tiles):
            nx, ny = grid.size.real_size
            cnx, cny = coarse_shape((nx, ny), factor)
            bits = tile_neighbours(params) if neighbours is None else neighbours[i]
            outs.append(params.device.empty(len(names) * cnx * cny, params.data_type))
            # the flow quantities in one pass; then every scalar plane in a pass of its own, in the slot of rho with the
            # quantity rho (no kernel of its own). `layout`: the name of each plane of the output, in its order
            flow = [(q, m) for q, m in zip(names, modes) if not q.startswith(SCALAR_QUANTITY)]
            passes = [(flow, "rho")] if flow else []
            passes += [([("rho", m)], "s:" + q[len(SCALAR_QUANTITY):]) for q, m in zip(names, modes) if q.startswith(SCALAR_QUANTITY)]
            done = 0
            for group, rho_slot in passes:
                spec = _c_spec(params, [q for q, _ in group], [m for _, m in group], bits)
                dst = outs[-1].ptr + done * cnx * cny * params.data_type.itemsize
                check(params.fn("derive")(params.device.ctx, grid.size.size[0], grid.size.ghosts, nx, ny, fx, fy,
                                          *[grid.ptr(f) for f in (rho_slot, "u", "v", "E")], C.byref(spec), C.c_void_p(dst)))
                done += len(group)
        for (params, grid), out in zip(tiles, outs):
            nx, ny = grid.size.real_size
            cnx, cny = coarse_shape((nx, ny), factor)
            planes = out.to_host()[:len(names) * cnx * cny].reshape(len(names), cny, cnx)
            ox, oy = (params.N_origin[0] - 1) // fx, (params.N_origin[1] - 1) // fy
            layout = [q for q in names if not q.startswith(SCALAR_QUANTITY)] + [q for q in names if q.startswith(SCALAR_QUANTITY)]
            for k, q in enumerate(layout):
                res[q][oy:oy + cny, ox:ox + cnx] = planes[k]
    finally:
        for out in outs:
            out.free()
    return res


# ---- images ----------------------------------------------------------------------------------------------------------------
def render(plane, lo=None, hi=None, transfer="linear"):
    """A ``(cny, cnx)`` plane → the ``uint8`` image of the same shape, row 0 of the plane at the BOTTOM. ``transfer``:
    ``"linear"``: ``(d - lo) / (hi - lo)``; ``"log"``: the same of ``log10(d)``, values clipped from below at the smallest
    positive value of the plane (``lo``, ``hi`` are bounds of ``d``, not of its logarithm); ``"schlieren"``:
    ``exp(-k (d - lo) / (hi - lo))`` with k = 15, dark where ``d`` is large. ``lo`` / ``hi`` = None: the finite minimum /
    maximum of the plane. The result is clipped to [0, 1] and rounded to 0 .. 255; pixels that are not finite become 0; a
    constant plane renders as ``lo`` does (nothing is divided by zero)."""
    if transfer not in TRANSFERS:
        solver_error("config", f"unknown transfer {transfer!r}: one of {', '.join(TRANSFERS)}")
    d = np.asarray(plane, dtype=np.float64)
    if d.ndim != 2:
        solver_error("config", f"render takes a 2-D plane, got shape {d.shape}")
    finite = np.isfinite(d)
    with np.errstate(all="ignore"):
        if transfer == "log":
            positive = finite & (d > 0)
            floor = d[positive].min() if positive.any() else 1.0
            d = np.log10(np.where(finite, np.maximum(d, floor), floor))
            lo = None if lo is None else np.log10(max(float(lo), floor))
            hi = None if hi is None else np.log10(max(float(hi), floor))
        lo = (d[finite].min() if finite.any() else 0.0) if lo is None else float(lo)
        hi = (d[finite].max() if finite.any() else 0.0) if hi is None else float(hi)
        span = hi - lo
        t = (np.where(finite, d, lo) - lo) / span if span > 0 else np.zeros_like(d)
        t = np.clip(t, 0.0, 1.0)
        shade = np.exp(-SCHLIEREN_K * t) if transfer == "schlieren" else t
    img = np.rint(np.clip(shade, 0.0, 1.0) * 255.0).astype(np.uint8)
    img[~finite] = 0
    return np.ascontiguousarray(img[::-1])


# ---- the run options (image_step, image_quantity, ..., image_at_end) -------------------------------------------------------
def default_image_factor(global_grid):
    """One isotropic factor: the smallest power of two that brings the longer side to at most 2048 pixels."""
    f = 1
    while -(-max(global_grid) // f) > 2048:
        f *= 2
    return (f, f)


def image_path(params, quantity, cycle):
    return os.path.join(params.output_dir, f"{params.image_file}_{quantity.replace(':', '_')}_{cycle:06d}.png")


def image_run(owner, params, gdt):
    """The frames of the run ``owner`` (a ``BlockGrid`` or a ``TileGroup``) after ``gdt.cycle`` completed cycles: one PNG file
    per quantity of ``image_quantity``, written to ``image_path`` and appended to ``owner.images``."""
    from .io import write_png_gray8
    planes = owner.derive(params.image_quantity, factor=params.image_factor, reduce=dict(params.image_reduce))
    os.makedirs(params.output_dir, exist_ok=True)
    lo, hi = params.image_range if params.image_range is not None else (None, None)
    paths = []
    for q in params.image_quantity:
        paths.append(write_png_gray8(image_path(params, q, gdt.cycle), render(planes[q], lo, hi, params.image_transfer[q])))
    owner.images.extend(paths)
    return paths
