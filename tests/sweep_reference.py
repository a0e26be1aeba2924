"""One directional sweep of the CPU oracle on arbitrary fields (test infrastructure: a plain helper module, no fixtures).

``reference_sweep`` composes the oracle's per-step functions in the order and with the ranges of ``sweep()`` in
oracle/armon_oracle.c, but takes what ``oracle.solve`` fixes through the test case as arguments: the EOS, which sides are
physical boundaries, and the two velocity factors of each mirror. tests/test_sweep_reference.py ties it to ``oracle.solve``.
"""
import numpy as np

from oracle import oracle as O

STATE = ("rho", "u", "v", "E")
GAMMA = 7. / 5.                      # update_eos() of the oracle; ArmonParameters' perfect-gas test cases use the same value


def draw_state(rng, n, eos):
    """``n`` cells of a physically plausible random (rho, u, v, E), drawn from ``rng`` in that order: the one copy of the
    bounds that tests/test_gpu_kernels.py (rand_state, test_bizarrium_EOS) and the fused-sweep tests share."""
    if eos == "bizarrium":
        return dict(rho=rng.uniform(0.9e4, 1.5e4, n), u=rng.uniform(-300, 300, n), v=rng.uniform(-300, 300, n),
                    E=rng.uniform(1e6, 5e6, n))
    return dict(rho=rng.uniform(0.1, 2.0, n), u=rng.uniform(-1, 1, n), v=rng.uniform(-1, 1, n), E=rng.uniform(2.0, 4.0, n))


def rand_state(nx, ny, g, eos, dtype, seed):
    """Random (rho, u, v, E) over the whole ghosted block, ghosts included: every cell differs from its neighbours, both signs
    of both velocities occur."""
    f = draw_state(np.random.default_rng(seed), (nx + 2 * g) * (ny + 2 * g), eos)
    return {k: a.astype(dtype) for k, a in f.items()}


def rand_dt(eos, dx):
    """A step of CFL number 0.2 for the fastest wave the states of ``rand_state`` hold."""
    return 0.2 * float(dx) / (2e4 if eos == "bizarrium" else 3.)


def uv_factors(axis, factors):
    """(factor of u, factor of v) of a mirror whose ``factors`` are (along the sweep axis, across it): the order of the
    oracle's boundary_conditions and of the u_factor_* / v_factor_* fields of armon_sweep_desc."""
    fa, ft = factors
    return (fa, ft) if axis == 0 else (ft, fa)


def real_mask(nx, ny, g, axis, lo=0, hi=None):
    """Flat mask over the ghosted block of the real cells with lo <= i < hi along ``axis`` (default: all of them)."""
    hi = (nx, ny)[axis] if hi is None else hi
    m = np.zeros((ny + 2 * g, nx + 2 * g), dtype=bool)
    if axis == 0:
        m[g:g + ny, g + lo:g + hi] = True
    else:
        m[g + lo:g + hi, g:g + nx] = True
    return m.ravel()


class SweepResult:
    """What ``reference_sweep`` returns. ``rho, u, v, E``: the state after the sweep (flat ghosted arrays; only the real cells
    are meaningful). ``p, c``: EOS pressure and sound speed of the state BEFORE the sweep (real cells). ``cfl(lo, hi)``: the
    CFL step armon_oracle_dtCFL gives for the real cells lo <= i < hi along the sweep axis (default: all) from the new u, v
    and the pre-sweep c — the c the next cycle's dtCFL reads in the oracle's time loop, which runs no EOS between the last
    sweep of a cycle and the reduction, and what include/armon_hip.h documents for ``dt_cfl_out``. ``cfl_fresh_eos``: the same
    reduction after an EOS of the new state (all real cells), for comparison."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def cfl(self, lo=0, hi=None):
        n = self.nx if self.axis == 0 else self.ny
        hi = n if hi is None else hi
        if self.axis == 0:
            r = O.domain_range(self.nx, self.ny, self.g, (lo, 0), (hi - self.nx, 0))
        else:
            r = O.domain_range(self.nx, self.ny, self.g, (0, lo), (0, hi - self.ny))
        L = O.lib(f32=self.f32)
        return self.dtype.type(L.armon_oracle_dtCFL(r, self.cfl_dx, self.cfl_dy, O.ptr(self.u), O.ptr(self.v), O.ptr(self.c)))


def reference_sweep(fields, nx, ny, g, axis, scheme, limiter, projection, eos, dt, dx, bc_low, bc_high, f_low, f_high, dtype,
                    cfl_dx=None, cfl_dy=None):
    """One sweep along ``axis`` (0 = x, 1 = y) of the block ``fields`` (flat ghosted arrays rho, u, v, E; not modified).

    ``scheme`` / ``limiter`` / ``projection``: the oracle's names ("GAD", "minmod", "euler_2nd", ...); ``eos``: "perfect_gas" or
    "bizarrium". ``bc_low`` / ``bc_high``: 1 = that side of the sweep axis is a physical boundary, mirrored with the factors
    ``f_low`` / ``f_high`` = (factor of the velocity along the axis, factor of the transverse velocity); 0 = the ghost cells of
    that side already hold a neighbour's (rho, u, v, E), as they do for a tile, and the EOS is evaluated on them too.
    ``dt``, ``dx``: step and cell size along the axis, rounded to ``dtype`` as the kernels round their descriptor's doubles.
    ``cfl_dx`` / ``cfl_dy``: the cell sizes of the CFL reduction (default ``dx`` for both)."""
    dtype = np.dtype(dtype)
    f32 = dtype == np.float32
    L = O.lib(f32=f32)
    L.armon_oracle_set_threads(1)
    P = O.ptr
    X = axis == 0
    row = nx + 2 * g
    s = 1 if X else row
    w = 2 if projection == "euler_2nd" else 1
    d = O.alloc_fields(nx, ny, g, dtype=dtype.type)
    for k in STATE:
        assert fields[k].dtype == dtype and fields[k].size == d[k].size
        d[k][:] = fields[k]
    ua = d["u"] if X else d["v"]

    def along(lo, hi):
        """Every real cell across the axis, real coordinates lo <= i < hi along it."""
        n = nx if X else ny
        return O.domain_range(nx, ny, g, (lo, 0), (hi - n, 0)) if X else O.domain_range(nx, ny, g, (0, lo), (0, hi - n))

    n = nx if X else ny
    eos_r = along(0 if bc_low else -g, n if bc_high else n + g)
    if eos == "bizarrium":
        L.armon_oracle_bizarrium_EOS(eos_r, *(P(d[k]) for k in ("rho", "u", "v", "E", "p", "c", "g")))
    else:
        L.armon_oracle_perfect_gas_EOS(eos_r, GAMMA, *(P(d[k]) for k in ("rho", "E", "u", "v", "p", "c", "g")))
    p_pre, c_pre = d["p"].copy(), d["c"].copy()

    # border_domain(bsize, side) and the increment towards the edge, as in sweep()
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
    adv = [P(d[k]) for k in ("us", "rho", "u", "v", "E", "work_1", "work_2", "work_3", "work_4")]
    if projection == "euler_2nd":
        L.armon_oracle_advection_second_order(ad, s, dx, dt, *adv)
    else:
        L.armon_oracle_advection_first_order(ad, s, dt, *adv)
    L.armon_oracle_euler_projection(pr, s, dx, dt, *adv)

    cfl_dx = dx if cfl_dx is None else cfl_dx
    cfl_dy = dx if cfl_dy is None else cfl_dy
    res = SweepResult(nx=nx, ny=ny, g=g, axis=axis, dtype=dtype, f32=f32, cfl_dx=cfl_dx, cfl_dy=cfl_dy,
                      rho=d["rho"], u=d["u"], v=d["v"], E=d["E"], p=p_pre, c=c_pre)
    fresh = {k: d[k].copy() for k in ("p", "c", "g")}
    real = along(0, n)
    if eos == "bizarrium":
        L.armon_oracle_bizarrium_EOS(real, *(P(d[k]) for k in ("rho", "u", "v", "E")), *(P(fresh[k]) for k in ("p", "c", "g")))
    else:
        L.armon_oracle_perfect_gas_EOS(real, GAMMA, *(P(d[k]) for k in ("rho", "E", "u", "v")), *(P(fresh[k]) for k in ("p", "c", "g")))
    res.cfl_fresh_eos = dtype.type(L.armon_oracle_dtCFL(real, cfl_dx, cfl_dy, P(d["u"]), P(d["v"]), P(fresh["c"])))
    return res
