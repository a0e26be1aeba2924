"""Exact solutions and error norms, the host side (no GPU): the Riemann and point-blast solutions against published values, what
``reference_for`` refuses, the fixed-point rule and the merge, the ABI and the run options, and the two statements that hold
the CPU oracle to the Euler equations: first-order convergence of Sod in L1 and the radius of Sedov's shock."""
import ctypes as C
import math
import os
import random
import re
import types

import numpy as np
import pytest

import armon_amd
from armon_amd import analytic as an
from armon_amd import io as aio
from armon_amd import profile as prof
from armon_amd._lib import SIGNATURES, ExactNorm, ExactSpec, SolverException
from armon_amd.parameters import ArmonParameters
from armon_amd.solver import SolverStats, graph_cycles_usable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("exact_norms_reset", "exact_norms", "exact_norms_f32", "exact_fill", "exact_fill_f32")
SOD_L, SOD_R = (1.0, 0.0, 1.0), (0.125, 0.0, 0.1)


def test_the_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "armon_hip.h")).read()
    L = armon_amd.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"ARMON_API int armon_hip_%s\(" % name, header), name
        assert "armon_hip_" + name in SIGNATURES
        assert getattr(L, "armon_hip_" + name).argtypes == SIGNATURES["armon_hip_" + name][1]
    assert "ARMON_EXACT_RIEMANN = 0, ARMON_EXACT_TABLE = 1" in header
    assert C.sizeof(ExactNorm) == 128 and ExactNorm.max_abs.offset == 88
    assert ExactSpec.scale_exp.offset == 80 and ExactSpec.time.offset == 112 and ExactSpec.table.offset == C.sizeof(ExactSpec) - 8


def test_sod_star_state_and_its_mirror_image():
    r = an.riemann_exact(SOD_L, SOD_R, 1.4)
    for got, want in ((r.p_star, 0.30313), (r.u_star, 0.92745), (r.rho_star_l, 0.42632), (r.rho_star_r, 0.26557), (r.speeds[4], 1.75216)):
        assert abs(got - want) < 5e-6, (got, want)
    assert r.speeds[3] == r.speeds[4]                               # a shock: head == tail
    assert r.speeds[0] < r.speeds[1] < r.speeds[2] < r.speeds[3]
    assert r.speeds[0] == -math.sqrt(1.4) and abs(r.speeds[1] - (r.u_star - r.c_star_l)) == 0
    # left shock, right fan: the mirror image
    m = an.riemann_exact((SOD_R[0], -SOD_R[1], SOD_R[2]), (SOD_L[0], -SOD_L[1], SOD_L[2]), 1.4)
    assert abs(m.p_star - 0.30313) < 5e-6 and abs(m.u_star + 0.92745) < 5e-6
    assert abs(m.rho_star_l - 0.26557) < 5e-6 and abs(m.rho_star_r - 0.42632) < 5e-6 and abs(m.speeds[0] + 1.75216) < 5e-6
    assert m.speeds[0] == m.speeds[1] < m.speeds[2] < m.speeds[3] < m.speeds[4]
    assert [-s for s in reversed(m.speeds)] == pytest.approx(list(r.speeds), abs=1e-14)
    # two shocks and two fans
    two_shocks = an.riemann_exact((1.0, 2.0, 1.0), (1.0, -2.0, 1.0), 1.4)
    assert two_shocks.speeds[0] == two_shocks.speeds[1] and two_shocks.speeds[3] == two_shocks.speeds[4] and two_shocks.p_star > 1
    assert abs(two_shocks.u_star) < 1e-14
    two_fans = an.riemann_exact((1.0, -0.5, 1.0), (1.0, 0.5, 1.0), 1.4)
    assert two_fans.speeds[0] < two_fans.speeds[1] < two_fans.speeds[2] < two_fans.speeds[3] < two_fans.speeds[4] and two_fans.p_star < 1
    with pytest.raises(SolverException):
        an.riemann_exact((1.0, -20.0, 1.0), (1.0, 20.0, 1.0), 1.4)   # vacuum


def line_spec(solution, n=400, samples=1, **kw):
    return solution.spec((0.0, 0.0), (1.0 / n, 1.0 / n), n, samples, **kw)


@pytest.mark.parametrize("mirror", [False, True])
def test_evaluate_is_continuous_across_a_fan_and_takes_the_outer_states(mirror):
    left, right = (SOD_L, SOD_R) if not mirror else ((SOD_R[0], 0.0, SOD_R[2]), (SOD_L[0], 0.0, SOD_L[2]))
    r = an.riemann_exact(left, right, 1.4)
    t = 0.2
    sol = an.ExactSolution(an.RIEMANN, "x", (0.5, 0.0), 1.4, time=t, riemann=r)
    s = line_spec(sol)
    head, tail = (r.speeds[0], r.speeds[1]) if not mirror else (r.speeds[4], r.speeds[3])
    outer, star = (left, (r.rho_star_l, r.u_star, r.p_star)) if not mirror else (right, (r.rho_star_r, r.u_star, r.p_star))
    for speed, want in ((head, outer), (tail, star)):
        q = speed * t
        for eps in (-1e-9, 1e-9):
            got = an._point(s, np.array([q + eps]))
            assert np.allclose([g[0] for g in got], want, rtol=0, atol=1e-7), (speed, eps, got, want)
    # beyond the heads: the outer states, bit for bit; between: monotone density
    gx = np.arange(400)
    rho, un, p = an.evaluate(s, gx, np.zeros(400, dtype=np.int64))
    x = (gx + 0.5) / 400
    lo, hi = x < 0.5 + r.speeds[0] * t, x >= 0.5 + r.speeds[4] * t
    assert lo.any() and hi.any()
    assert np.all(rho[lo] == left[0]) and np.all(p[lo] == left[2]) and np.all(un[lo] == 0)
    assert np.all(rho[hi] == right[0]) and np.all(p[hi] == right[2]) and np.all(un[hi] == 0)
    assert np.all(np.diff(rho) <= 0) if not mirror else np.all(np.diff(rho) >= 0)
    # more samples: the mean of the points, and the same far from the waves
    s4 = line_spec(sol, samples=4)
    rho4, _, _ = an.evaluate(s4, gx, np.zeros(400, dtype=np.int64))
    far = x + 0.5 / 400 < 0.5 + r.speeds[0] * t                     # the whole cell lies before the first wave
    assert np.all(rho4[far] == left[0]) and np.abs(rho4 - rho).max() < 0.2 and np.abs(rho4 - rho).max() > 0


def test_sedov_similarity():
    s = an.sedov_similarity(1.4, 2, 2000)
    assert s.g[-1] == pytest.approx(6.0, abs=1e-14) and s.v[-1] == pytest.approx(2 / 2.4, abs=1e-15) and s.pi[-1] == pytest.approx(2 / 2.4, abs=1e-15)
    assert abs(s.alpha - 0.98407) < 1e-3
    fine = an.sedov_similarity(1.4, 2, 4000)
    print(f"alpha = {s.alpha:.9f} (2000 nodes), {fine.alpha:.9f} (4000 nodes)")
    assert abs(fine.alpha - s.alpha) < 1e-5
    assert len(s.lam) == 2001 and s.lam[0] == 0 and s.lam[-1] == 1
    assert s.g[0] == 0 and s.v[0] == 0 and s.pi[0] > 0 and np.all(np.diff(s.g) > 0) and np.all(np.isfinite(s.pi))
    with pytest.raises(SolverException):
        an.sedov_similarity(1.4, 2, 7)


def test_the_sedov_table_holds_the_energy_of_the_initial_state(oracle):
    params = ArmonParameters(test="Sedov", N=(100, 100), silent=5)
    E0, cells = an.sedov_energy(params)
    assert cells == 4
    run, _ = oracle.solve(test="Sedov", N=(100, 100), maxcycle=0)
    # conservation_vars holds the background too: rho E_low over the whole domain
    assert abs(run.initial_energy - (E0 + 2.5e-14 * 4.0)) < 1e-12 * E0 and abs(run.initial_energy - 1.0824517) < 1e-7
    sol = an.reference_for(params, 0.5)
    assert sol.form == an.TABLE and sol.coord == "r" and sol.centre == (0.0, 0.0) and sol.outer == (1.0, 0.0, (7 / 5 - 1) * 2.5e-14)
    R, M = sol.scale, sol.values.shape[1] - 1
    r = np.arange(M + 1) / M * R
    rho, un, p = sol.values
    energy = an._simpson((0.5 * rho * un * un + p / 0.4) * 2 * math.pi * r, R / M)
    print(f"E0 = {E0:.10f}, energy of the table = {energy:.10f}, R = {R:.6f}")
    assert abs(energy - E0) < 1e-12 * E0
    assert rho[-1] == pytest.approx(6.0) and sol.info["R"] == R


def test_reference_for_refuses_what_has_no_solution():
    def refused(test, time, **kw):
        with pytest.raises(SolverException) as e:
            an.reference_for(ArmonParameters(test=test, N=(64, 64), silent=5, **kw), time)
        assert e.value.category == "analytic"
        return e.value.msg
    for test in ("Sod_circ", "Bizarrium", "DebugIndexes"):
        assert "closed" in refused(test, 0.1)
    assert "time" in refused("Sod", 0.0) and "time" in refused("Sod", -1.0) and "time" in refused("Sedov", math.nan)
    assert "wall" in refused("Sod", 0.286) and "wall" in refused("Sod_y", 0.5)
    assert "side" in refused("Sedov", 1.0)
    ok = an.reference_for(ArmonParameters(test="Sod", N=(64, 64), silent=5), 0.285)
    assert ok.form == an.RIEMANN and ok.coord == "x" and ok.centre == (0.5, 0.0)
    assert an.reference_for(ArmonParameters(test="Sod_y", N=(64, 64), silent=5), 0.2).coord == "y"
    assert an.reference_for(ArmonParameters(test="Sedov", N=(64, 64), silent=5), 0.5).coord == "r"


def random_record(rng):
    raw = an.neutral()
    for k in range(4):
        raw[k, :2] = [rng.randrange(1 << 40), rng.randrange(1 << 20)]
        raw[k, 2:11] = [rng.randrange(1 << 64) for _ in range(9)]
        if rng.random() < 0.8:
            raw[k, 11], raw[k, 12] = rng.choice([1, 7, 1 << 62]), rng.randrange(1 << 30)
    return raw


def test_the_merge_is_associative_and_commutative():
    rng = random.Random(7)
    for _ in range(200):
        a, b, c = (random_record(rng) for _ in range(3))
        assert np.array_equal(an.merge_raw(a, b), an.merge_raw(b, a))
        assert np.array_equal(an.merge_raw(an.merge_raw(a, b), c), an.merge_raw(a, an.merge_raw(b, c)))
        assert np.array_equal(an.merge_raw(a, an.neutral()), a)


def test_a_record_is_the_merge_of_its_parts_and_decodes_to_the_norms():
    rng = np.random.default_rng(3)
    sol = an.reference_for(ArmonParameters(test="Sod", N=(40, 6), silent=5), 0.15)
    s = sol.spec((0.0, 0.0), (1 / 40, 1 / 6), 40)
    (rho, u, v, E), _ = an.stored_reference(s, np.arange(40)[None, :], np.arange(6)[:, None])
    zero = an.reference_record(s, rho, u, v, E)
    assert not zero[:, 2:12].any() and np.all(zero[:, 0] == 240) and np.all(zero[:, 12] == prof.MASK)     # the filled state is at distance 0
    state = [a + rng.uniform(-0.1, 0.1, a.shape) for a in (rho, u, v, E)]
    whole = an.reference_record(s, *state)
    parts = an.neutral()
    for x0, x1, y0, y1 in ((0, 13, 0, 6), (13, 40, 0, 2), (13, 40, 2, 6)):
        parts = an.merge_raw(parts, an.reference_record(s, *[a[y0:y1, x0:x1] for a in state], origin=(x0, y0)))
    assert np.array_equal(parts, whole)
    norms = an.ErrorNorms(whole, s.scale_exp, 40)
    gx, gy = np.arange(40)[None, :], np.arange(6)[:, None]
    d = state[0] - rho
    assert norms.n == 240 and norms.n_bad == 0
    assert norms.rho.l1 == pytest.approx(np.abs(d).mean(), rel=1e-12) and norms.rho.l2 == pytest.approx(math.sqrt((d * d).mean()), rel=1e-12)
    assert norms.rho.bias == pytest.approx(d.mean(), rel=1e-9) and norms.rho.linf == np.abs(d).max()
    iy, ix = np.unravel_index(np.abs(d).argmax(), d.shape)
    assert norms.rho.linf_at == (ix, iy)
    assert norms.ut.linf == np.abs(state[2]).max()                  # the reference's transverse velocity is 0
    # a NaN and an infinity go to n_bad only; a coordinate range skips cells altogether
    state[0][2, 5], state[3][4, 30] = math.nan, math.inf
    bad = an.reference_record(s, *state)
    skip = np.zeros((6, 40), dtype=bool)
    skip[2, 5] = skip[4, 30] = True
    clean = an.reference_record(s, *state, skip=skip)
    assert np.all(bad[:, 1] == 2) and np.all(bad[:, 0] == 238) and np.array_equal(bad[:, 2:], clean[:, 2:]) and not clean[:, 1].any()
    cut = sol.spec((0.0, 0.0), (1 / 40, 1 / 6), 40, coord_range=(-0.2, 0.1))
    assert int(an.reference_record(cut, *state)[0, :2].sum()) == 6 * int(((gx + 0.5) / 40 - 0.5 >= -0.2).sum() - ((gx + 0.5) / 40 - 0.5 >= 0.1).sum())


def test_the_file_round_trips(tmp_path):
    rng = np.random.default_rng(5)
    sol = an.reference_for(ArmonParameters(test="Sod_y", N=(8, 30), silent=5), 0.1)
    s = sol.spec((0.0, 0.0), (1 / 8, 1 / 30), 8, samples=2)
    state = [rng.uniform(0.5, 1.5, (30, 8)) for _ in range(4)]
    norms = an.ErrorNorms(an.reference_record(s, *state), s.scale_exp, 8, samples=2, cycle=12, time=0.1)
    path = str(tmp_path / "norms.txt")
    aio.write_error_norms_file(path, norms, 17)
    assert aio.read_error_norms_file(path) == norms.table()
    assert "L1" in norms.report() and norms.merge(an.ErrorNorms(an.neutral(), s.scale_exp, 8, samples=2)) == norms


def test_the_run_options():
    p = ArmonParameters(test="Sod", N=(32, 8), silent=5)
    assert p.error_norms_step == 0 and not p.error_norms_at_end and p.start_from_exact is None and not p.exact_solution
    assert SolverStats(0., 0., 0, 0., 0, 0.).error_norms == []
    q = ArmonParameters(test="Sod", N=(32, 8), silent=5, error_norms_step=3, error_norms_samples=2, error_norms_file="en", start_from_exact=0.05)
    assert (q.error_norms_step, q.error_norms_samples, q.error_norms_file, q.start_from_exact, q.exact_solution) == (3, 2, "en", 0.05, True)

    def usable(**kw):
        g = ArmonParameters(test="Sod", N=(32, 8), silent=5, graph_cycles=True, **kw)
        g._device = types.SimpleNamespace(owns_ctx=True)
        return graph_cycles_usable(g)
    assert usable() is True and usable(error_norms_samples=2) is True
    assert usable(error_norms_at_end=True) is False and usable(error_norms_step=4) is False and usable(start_from_exact=0.1) is False

    def refused(**kw):
        with pytest.raises(SolverException) as e:
            ArmonParameters(**{**dict(test="Sod", N=(32, 8), silent=5), **kw})
        assert e.value.category == "config"
    for bad in (dict(error_norms_step=-1), dict(error_norms_step=1.5), dict(error_norms_step=True), dict(error_norms_samples=3),
                dict(error_norms_file="a/b"), dict(start_from_exact=0.0), dict(start_from_exact=-1.0), dict(start_from_exact="x"),
                dict(start_from_exact=0.05, compare=True), dict(start_from_exact=0.05, is_ref=True),
                dict(error_norms_at_end=True, test="Sod_circ"), dict(error_norms_step=2, test="Bizarrium"),
                dict(start_from_exact=0.05, test="Sod_circ"), dict(start_from_exact=0.05, restart_from="x.ckpt")):
        refused(**bad)


def test_the_options_are_refused_for_ranks(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    ArmonParameters(test="Sod", N=(8, 8), use_MPI=True)
    for opts in (dict(error_norms_step=2), dict(error_norms_at_end=True), dict(start_from_exact=0.05)):
        with pytest.raises(SolverException) as e:
            ArmonParameters(test="Sod", N=(8, 8), use_MPI=True, **opts)
        assert e.value.category == "config" and "use_MPI" in e.value.msg


def l1_rho_of_the_oracle(oracle, N):
    run, f = oracle.solve(test="Sod", N=(N, 8))
    params = ArmonParameters(test="Sod", N=(N, 8), silent=5)
    sol = an.reference_for(params, float(run.final_time))
    s = an.spec_of(params, sol, samples=1)
    rec = an.reference_record(s, *[oracle.real_view(f[k], N, 8, 4) for k in ("rho", "u", "v", "E")])
    norms = an.ErrorNorms(rec, s.scale_exp, N)
    assert norms.n == 8 * N and norms.n_bad == 0
    return norms.rho.l1


def test_the_oracle_converges_to_the_exact_sod_solution(oracle):
    """L1(rho) of the CPU oracle against the exact solution at the run's final time, N x 8 cells, samples = 1: the observed order
    log2(L1(N) / L1(2N)) is >= 0.75 at both doublings (a first-order-accurate capture of a shock and a contact; the issue
    measured 0.89 and 0.85)."""
    l1 = {N: l1_rho_of_the_oracle(oracle, N) for N in (100, 200, 400)}
    orders = [math.log2(l1[N] / l1[2 * N]) for N in (100, 200)]
    print("L1(rho):", {N: f"{v:.4e}" for N, v in l1.items()}, "orders:", [f"{o:.3f}" for o in orders])
    assert all(o >= 0.75 for o in orders), (l1, orders)


def test_the_oracles_sedov_shock_sits_at_the_similarity_radius(oracle):
    """Sedov 100 x 100 to t = 0.5: the radius at which the ring-averaged density (rings of one cell) peaks lies within 2 cells of
    R(final_time) = (E0 t^2 / (alpha rho0))^(1/4)."""
    N = 100
    run, f = oracle.solve(test="Sedov", N=(N, N), maxtime=0.5)
    params = ArmonParameters(test="Sedov", N=(N, N), silent=5)
    sol = an.reference_for(params, float(run.final_time))
    rho = oracle.real_view(f["rho"], N, N, 4)
    dx = 2.0 / N
    x = (np.arange(N) + 0.5) * dx - 1.0
    ring = np.floor(np.hypot(x[None, :], x[:, None]) / dx).astype(np.int64)
    mean = np.bincount(ring.ravel(), weights=rho.ravel()) / np.maximum(np.bincount(ring.ravel()), 1)
    peak = (int(np.argmax(mean[:N // 2])) + 0.5) * dx
    print(f"t = {run.final_time:.6f}: R = {sol.scale:.4f}, ring-mean density peaks at r = {peak:.4f}")
    assert abs(peak - sol.scale) <= 2 * dx


def good_c_spec(**kw):
    sol = an.reference_for(ArmonParameters(test="Sod", N=(8, 8), silent=5), 0.1)
    s = an.spec_of(ArmonParameters(test="Sod", N=(8, 8), silent=5), sol)
    c = an._c_spec(s, None)
    for k, v in kw.items():
        if k == "scale_exp":
            for i, pair in enumerate(v):
                c.scale_exp[i][:] = list(pair)
        else:
            setattr(c, k, v)
    return c


def test_a_null_context_and_every_bad_argument_are_refused():
    L = armon_amd.lib()
    ctx = C.cast(C.create_string_buffer(4096), C.c_void_p)      # never dereferenced: every check below comes before the first use of the context
    data = C.cast(C.create_string_buffer(64), C.c_void_p)
    geometry = dict(row_length=16, nghost=4, nx=8, ny=8, col0=0, row0=0, wnx=8, wny=8, gcol=0, grow=0)
    inf, nan = math.inf, math.nan
    for name in ("exact_norms", "exact_norms_f32", "exact_fill", "exact_fill_f32"):
        fn = getattr(L, "armon_hip_" + name)

        def call(ctx=ctx, spec=None, out=data, rho=data, **kw):
            g = {**geometry, **kw}
            spec = good_c_spec() if spec is None else spec
            args = [ctx, g["row_length"], g["nghost"], g["nx"], g["ny"], rho, data, data, data, g["col0"], g["row0"], g["wnx"], g["wny"],
                    g["gcol"], g["grow"], C.byref(spec) if spec is not False else None]
            return fn(*args, out) if "norms" in name else fn(*args)
        assert call(ctx=None) == 1, name
        assert b"ctx" in L.armon_hip_last_error()
        for bad in (dict(nx=0), dict(ny=0), dict(nghost=-1), dict(row_length=15), dict(col0=-1), dict(row0=-1), dict(wnx=0), dict(wny=0),
                    dict(col0=1), dict(row0=1), dict(wnx=9), dict(wny=9), dict(gcol=-1), dict(grow=-1), dict(gcol=1)):
            assert call(**bad) == 1, (name, bad)
        assert call(rho=None) == 1 and call(spec=False) == 1
        if "norms" in name:
            assert call(out=None) == 1
            assert call(spec=good_c_spec(scale_exp=((0, 0), (0, 5000), (0, 0), (0, 0)))) == 1
        for bad in (dict(form=2), dict(coord=3), dict(coord=-1), dict(samples=3), dict(samples=0), dict(eos=1), dict(eos=-1), dict(global_nx=0),
                    dict(dx=0.0), dict(dx=inf), dict(dy=nan), dict(cx=nan), dict(cy=inf), dict(gamma=1.0), dict(gamma=5 / 3), dict(time=0.0),
                    dict(time=nan), dict(coord_min=nan), dict(coord_max=nan)):
            assert call(spec=good_c_spec(**bad)) == 1, (name, bad)
        table = good_c_spec()
        table.form, table.M, table.inv_scale, table.table = an.TABLE, 4, 1.0, None
        assert call(spec=table) == 1 and b"table" in L.armon_hip_last_error()
        table.table, table.M = data.value, 0
        assert call(spec=table) == 1
        table.M, table.inv_scale = 4, 0.0
        assert call(spec=table) == 1
    assert L.armon_hip_exact_norms_reset(None, data) == 1 and L.armon_hip_exact_norms_reset(ctx, None) == 1


def test_a_global_window_is_cut_along_the_tiles():
    tiles = [(types.SimpleNamespace(global_grid=(150, 90), N_origin=(ox + 1, oy + 1), N=(75, 45)), None) for oy in (0, 45) for ox in (0, 75)]
    assert an.tile_windows(tiles, (0, 0, 150, 90)) == [(0, 0, 75, 45)] * 4
    assert an.tile_windows(tiles, (40, 20, 75, 50)) == [(40, 20, 35, 25), (0, 20, 40, 25), (40, 0, 35, 25), (0, 0, 40, 25)]
    assert an.tile_windows(tiles, (80, 50, 10, 5)) == [None, None, None, (5, 5, 10, 5)]
    for bad in ((0, 0, 151, 90), (-1, 0, 10, 10), (0, 0, 0, 10), (100, 80, 10, 11)):
        with pytest.raises(SolverException):
            an.tile_windows(tiles, bad)
