"""End-to-end GPU parity: ``armon(params)`` through the C ABI against the reference's golden results
and against the CPU oracle (bit-exact in exact-arithmetic mode), plus the reference's property tests
(conservation, axis invariance, ghost garbage — ref test/conservation.jl, test/convergence.jl)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
G = 4


def isapprox_count(a, b, atol=1e-13, rtol=4 * EPS):
    return int((np.abs(a - b) > np.maximum(atol, rtol * np.maximum(np.abs(a), np.abs(b)))).sum())


def run(test, N=(100, 100), **kw):
    import armon_amd
    opts = dict(test=test, N=N, maxcycle=1000, silent=5, return_data=True, exact_arithmetic=True)
    opts.update(kw)
    params = armon_amd.ArmonParameters(**opts)
    stats = armon_amd.armon(params)
    host = stats.data.device_to_host()
    return params, stats, host


MODES = [pytest.param(False, id="staged"), pytest.param(True, id="fused")]


@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("test", ["Sod", "Sod_y", "Sod_circ"])
def test_reference_golden_sod_family(test, fused):
    """ref test/gpu.jl:16-44 / test/convergence.jl:5-28 with the reference's own tolerance rule."""
    g = load_golden(test)
    params, stats, host = run(test, use_fused_sweep=fused)
    assert stats.cycles == int(g["cycles"])
    assert abs(stats.last_dt - float(g["dt"])) <= max(1e-13, 4 * EPS * float(g["dt"]))
    grid = stats.data
    for k in ("x", "y", "rho", "u", "v", "p"):
        assert isapprox_count(grid.real_view(host[k]), g[k]) == 0, k


@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("test", ["Bizarrium", "Sedov"])
def test_reference_golden_unasserted_cases(test, fused):
    g = load_golden(test)
    params, stats, host = run(test, use_fused_sweep=fused)
    assert stats.cycles == int(g["cycles"])
    assert abs(stats.last_dt - float(g["dt"])) <= 1e-12 * float(g["dt"])
    for k in ("rho", "u", "v", "p"):
        a = stats.data.real_view(host[k])
        assert np.abs(a - g[k]).max() <= 1e-12 * np.abs(g[k]).max(), k


@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("test,N,opts", [
    ("Sod", (100, 100), {}),
    ("Sod_circ", (67, 41), {}),
    ("Sedov", (50, 50), dict(maxcycle=40)),
    ("Bizarrium", (64, 32), dict(maxcycle=30)),
    ("Sod_circ", (48, 48), dict(scheme="Godunov", maxcycle=25)),
    ("Sod_circ", (48, 48), dict(projection="euler", maxcycle=25)),
    ("Sod_circ", (48, 48), dict(riemann_limiter="superbee", maxcycle=25)),
    ("Sod_circ", (48, 48), dict(riemann_limiter="no_limiter", maxcycle=25)),
    ("Sod_circ", (48, 40), dict(axis_splitting="Strang", maxcycle=15)),
    ("Sod_circ", (48, 40), dict(axis_splitting="Godunov", maxcycle=15)),
    ("Sod", (40, 8), dict(axis_splitting="X_only", maxcycle=15)),
    ("Sod_y", (8, 40), dict(axis_splitting="Y_only", maxcycle=15)),
    ("Sod_circ", (40, 40), dict(cst_dt=True, Dt=1e-3, maxcycle=15)),
    ("Sod_circ", (40, 40), dict(scheme="Godunov", projection="euler", nghost=2, maxcycle=15)),
    ("Sod_circ", (40, 40), dict(nghost=5, maxcycle=15)),
    # several workgroups / strips / runs per axis, odd sizes, odd and wide ghost layers (origin alignment paths)
    ("Sod_circ", (517, 263), dict(nghost=5, maxcycle=8)),
    ("Sod_circ", (1031, 130), dict(nghost=6, maxcycle=8)),
    ("Sedov", (300, 301), dict(nghost=7, maxcycle=8)),
    ("Sod_circ", (770, 515), dict(axis_splitting="Godunov", maxcycle=7)),      # X-last cycles: X sweep dt tracking
    ("Bizarrium", (513, 129), dict(axis_splitting="X_only", maxcycle=8)),
    # row pitch 4 past a multiple of 8 cells: every other row starts mid-sector (X strip origins taken row by row)
    ("Sod_circ", (1004, 37), dict(maxcycle=8)),
])
def test_bit_exact_against_oracle(oracle, test, N, opts, fused):
    """Whole-solver parity: every real cell of ρ,u,v,E,p, the cycle count and dt are identical."""
    params, stats, host = run(test, N=N, use_fused_sweep=fused, **opts)
    orun, f = oracle.solve(test=test, N=N, **{"maxcycle": 1000, **opts})
    assert stats.cycles == orun.cycles
    assert stats.last_dt == orun.last_dt and stats.final_time == orun.final_time
    g = opts.get("nghost", 4)
    for k in ("rho", "u", "v", "E", "p"):
        a = stats.data.real_view(host[k])
        b = oracle.real_view(f[k], N[0], N[1], g)
        assert np.array_equal(a, b), f"{k}: max abs diff {np.abs(a - b).max()}"


@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("test", ["Sod", "Sod_y", "Sod_circ"])
def test_conservation(test, fused):
    """ref test/conservation.jl:1-16"""
    import armon_amd
    from armon_amd.solver import BlockGrid, conservation_vars, init_test, time_loop
    params = armon_amd.ArmonParameters(test=test, N=(100, 100), maxcycle=10000, silent=5, use_fused_sweep=fused,
                                       exact_arithmetic=True)
    grid = BlockGrid(params)
    init_test(params, grid)
    m0, e0 = conservation_vars(params, grid)
    time_loop(params, grid)
    m1, e1 = conservation_vars(params, grid)
    assert abs(m1 - m0) <= 1e-12 and abs(e1 - e0) <= 1e-12


@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("test,axis", [("Sod", 0), ("Sod_y", 1), ("Bizarrium", 0)])
def test_axis_invariance(test, axis, fused):
    """ref test/convergence.jl:31-64"""
    params, stats, host = run(test, N=(40, 40), maxcycle=30, use_fused_sweep=fused)
    for k in ("rho", "u", "v", "p", "E"):
        a = stats.data.real_view(host[k])
        ref = a[0:1, :] if axis == 0 else a[:, 0:1]
        assert np.array_equal(a, np.broadcast_to(ref, a.shape)), k


@pytest.mark.parametrize("fused", MODES)
def test_ghost_garbage_does_not_propagate(fused):
    """ref test/convergence.jl:67-102: 1e100 in every ghost cell of every array, same result."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test, time_loop
    N = (32, 24)
    _, stats0, host0 = run("Sod_circ", N=N, maxcycle=12, use_fused_sweep=fused)
    params = armon_amd.ArmonParameters(test="Sod_circ", N=N, maxcycle=12, silent=5, use_fused_sweep=fused,
                                       exact_arithmetic=True)
    grid = BlockGrid(params)
    init_test(params, grid)
    sx, sy = params.block_size.size
    m = np.ones((sy, sx), dtype=bool)
    m[G:G + N[1], G:G + N[0]] = False
    for k in ("rho", "u", "v", "E", "p", "c", "g", "us", "ps", "work_1", "work_2", "work_3", "work_4"):
        a = grid.data[k].to_host().reshape(sy, sx)
        a[m] = 1e100
        grid.data[k].copy_from_host(a.ravel())
    if grid.alt:
        for k in grid.alt:
            grid.alt[k].copy_from_host(np.full(sx * sy, 1e100))
    t, dt, cycles, _, _ = time_loop(params, grid)
    assert cycles == stats0.cycles and dt == stats0.last_dt
    host = grid.device_to_host()
    for k in ("rho", "u", "v", "E", "p"):
        assert np.array_equal(grid.real_view(host[k]), grid.real_view(host0[k])), k


def test_invalid_time_step_is_reported():
    """ref src/solver_state.jl:123-124 → SolverException(:time)"""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test, time_loop
    params = armon_amd.ArmonParameters(test="Sod", N=(16, 16), maxcycle=3, silent=5, use_fused_sweep=False)
    grid = BlockGrid(params)
    init_test(params, grid)
    grid.data["E"].copy_from_host(np.full(params.block_size.n_cells, -1.0))   # e < 0 → NaN sound speed
    with pytest.raises(armon_amd.SolverException) as e:
        time_loop(params, grid)
    assert e.value.category == "time"


# ---- tuned arithmetic (exact_arithmetic=False): shared 1-ulp reciprocals + FMAs in the fused sweep ----
# Stated fp64 tolerance of the tuned build: same cycle count, |dt - dt_ref| <= 1e-12 dt_ref,
# max|Δ| <= 1e-11 · max|field| for ρ, u, v, p (E included here); conservation to the reference's 1e-12.
FAST_CASES = [
    ("Sod", (100, 100), {}),
    ("Sod_y", (100, 100), {}),
    ("Sod_circ", (100, 100), {}),
    ("Bizarrium", (100, 100), {}),
    ("Sedov", (100, 100), {}),
    ("Sod_circ", (67, 41), dict(scheme="Godunov", maxcycle=40)),
    ("Sod_circ", (48, 48), dict(projection="euler", maxcycle=40)),
    ("Sod_circ", (48, 48), dict(riemann_limiter="superbee", maxcycle=40)),
    ("Sod_circ", (48, 48), dict(riemann_limiter="no_limiter", maxcycle=40)),
    ("Sod_circ", (48, 40), dict(axis_splitting="Strang", maxcycle=20)),
    ("Sod_circ", (40, 40), dict(scheme="Godunov", projection="euler", nghost=2, maxcycle=20)),
    ("Sod_circ", (517, 263), dict(nghost=5, maxcycle=8)),
    ("Sedov", (300, 301), dict(nghost=7, maxcycle=8)),
    ("Sod_circ", (770, 515), dict(axis_splitting="Godunov", maxcycle=7)),
    ("Bizarrium", (513, 129), dict(axis_splitting="X_only", maxcycle=8)),
]


@pytest.mark.parametrize("test,N,opts", FAST_CASES)
def test_fast_arithmetic_within_tolerance_of_oracle(oracle, test, N, opts):
    params, stats, host = run(test, N=N, use_fused_sweep=True, exact_arithmetic=False, **opts)
    orun, f = oracle.solve(test=test, N=N, **{"maxcycle": 1000, **opts})
    assert stats.cycles == orun.cycles
    assert abs(stats.last_dt - orun.last_dt) <= 1e-12 * orun.last_dt
    g = opts.get("nghost", 4)
    for k in ("rho", "u", "v", "E", "p"):
        a = stats.data.real_view(host[k])
        b = oracle.real_view(f[k], N[0], N[1], g)
        scale = max(np.abs(b).max(), 1e-300)
        assert np.abs(a - b).max() <= 1e-11 * scale, f"{k}: {np.abs(a - b).max() / scale:.3e} of max"


@pytest.mark.parametrize("test", ["Sod", "Sod_y", "Sod_circ"])
def test_fast_arithmetic_golden_and_conservation(test):
    import armon_amd
    from armon_amd.solver import BlockGrid, conservation_vars, init_test, time_loop
    g = load_golden(test)
    params = armon_amd.ArmonParameters(test=test, N=(100, 100), maxcycle=1000, silent=5, exact_arithmetic=False)
    grid = BlockGrid(params)
    init_test(params, grid)
    m0, e0 = conservation_vars(params, grid)
    t, dt, cycles, _, _ = time_loop(params, grid)
    m1, e1 = conservation_vars(params, grid)
    assert cycles == int(g["cycles"])
    assert abs(dt - float(g["dt"])) <= max(1e-13, 4 * EPS * float(g["dt"]))
    assert abs(m1 - m0) <= 1e-12 and abs(e1 - e0) <= 1e-12
    host = grid.device_to_host()
    # the reference's own comparison rule (ref test/reference_data/reference_functions.jl:54-57)
    for k in ("rho", "u", "v", "p"):
        assert isapprox_count(grid.real_view(host[k]), g[k]) == 0, k


# ---- alternative X-sweep kernel forms and p/c materialisation on an X sweep ---------------------------------
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("xk", [2, 3], ids=["lds_march", "dpp_k1"])
@pytest.mark.parametrize("test,N,opts", [
    ("Sod_circ", (67, 41), dict(maxcycle=15)),
    ("Sod_circ", (130, 40), dict(maxcycle=10, axis_splitting="Godunov")),     # odd cycles end with an X sweep
    ("Sod", (64, 8), dict(maxcycle=10, axis_splitting="X_only")),
    ("Bizarrium", (64, 32), dict(maxcycle=12, scheme="Godunov")),
])
def test_alternative_x_kernels(oracle, test, N, opts, xk, exact):
    """The measured-and-rejected X forms live in the A/B build only (libarmon_hip_alt.so, -DARMON_ALT_KERNELS)."""
    import armon_amd
    from armon_amd import _lib
    with _lib.alt_kernels():
        params = armon_amd.ArmonParameters(test=test, N=N, silent=5, return_data=True, exact_arithmetic=exact, **opts)
        params.x_kernel = xk
        stats = armon_amd.armon(params)
        host = stats.data.device_to_host()
    orun, f = oracle.solve(test=test, N=N, **opts)
    assert stats.cycles == orun.cycles
    for k in ("rho", "u", "v", "E", "p"):
        a = stats.data.real_view(host[k])
        b = oracle.real_view(f[k], N[0], N[1], 4)
        if exact:
            assert np.array_equal(a, b), k
        else:
            assert np.abs(a - b).max() <= 1e-11 * max(np.abs(b).max(), 1e-300), k
    assert (stats.last_dt == orun.last_dt) if exact else abs(stats.last_dt - orun.last_dt) <= 1e-12 * orun.last_dt


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("axis_name", ["X", "Y"])
@pytest.mark.parametrize("scheme,projection", [("GAD", "euler_2nd"), ("Godunov", "euler"), ("GAD", "euler")])
def test_partial_sweeps_equal_the_full_sweep(axis_name, scheme, projection, exact):
    """interior [LAG, n-LAG) + the two LAG-wide strips == one full sweep, including the fused dt."""
    import armon_amd
    from armon_amd.blocking import Axis
    from armon_amd.solver import BlockGrid, fused_sweep, init_test, sweep_lag
    N = (150, 70)
    axis = Axis.X if axis_name == "X" else Axis.Y
    n = N[int(axis) - 1]
    res = []
    for split in (False, True):
        params = armon_amd.ArmonParameters(test="Sod_circ", N=N, scheme=scheme, projection=projection, silent=5,
                                           exact_arithmetic=exact)
        grid = BlockGrid(params)
        init_test(params, grid)
        lag = sweep_lag(params)
        dx, dt = 1.0 / n, 0.2 / n
        if not split:
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, emit_p=True)
        else:
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, emit_p=True, out_range=(lag, n - lag), swap=False)
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, emit_p=True, out_range=(0, lag), swap=False, dt_accumulate=True)
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, emit_p=True, out_range=(n - lag, n), swap=False, dt_accumulate=True)
            grid.swap_state()
        host = grid.device_to_host(("rho", "u", "v", "E", "p"))
        res.append(({k: grid.real_view(v).copy() for k, v in host.items()}, float(grid.dt_scalar.to_host()[0])))
    for k in res[0][0]:
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
    assert res[0][1] == res[1][1] and np.isfinite(res[0][1])


def test_step_checkpoints_dump_then_compare(tmp_path):
    """compare / is_ref (ref src/io.jl:185-227, src/solver.jl:288-320): dump every sub-step, re-run against the
    dumps, then detect a deliberate change at the first sub-step it affects."""
    import armon_amd
    common = dict(test="Sod_circ", N=(24, 20), maxcycle=3, silent=5, output_dir=str(tmp_path), output_file="chk",
                  compare=True)
    ref = armon_amd.armon(armon_amd.ArmonParameters(is_ref=True, **common))
    assert ref.cycles == 3
    names = sorted(p.name for p in tmp_path.iterdir())
    for expected in ("chk_000_init_test_X", "chk_000_EOS_init_X", "chk_000_time_step_X", "chk_000_EOS_X",
                     "chk_000_boundary_conditions_X", "chk_000_numerical_fluxes_X", "chk_000_cell_update_X",
                     "chk_000_projection_remap_Y", "chk_002_projection_remap_Y"):
        assert expected in names, expected
    same = armon_amd.armon(armon_amd.ArmonParameters(is_ref=False, **common))
    assert same.cycles == 3 and not any(n.endswith("_diff") for n in (p.name for p in tmp_path.iterdir()))
    other = armon_amd.armon(armon_amd.ArmonParameters(is_ref=False, cfl=0.5, **common))
    assert other.cycles == 0                                      # stopped at cycle 0's time step comparison
    

def test_write_output_in_reference_format(tmp_path):
    import armon_amd
    from armon_amd import io as aio
    params = armon_amd.ArmonParameters(test="Sod", N=(100, 100), maxcycle=1000, silent=5, write_output=True,
                                       output_dir=str(tmp_path), output_file="sod", return_data=True, exact_arithmetic=True)
    stats = armon_amd.armon(params)
    g = load_golden("Sod")
    host = aio.read_sub_domain_file(params, "sod")
    for k in ("x", "y", "rho", "u", "v", "p"):
        assert isapprox_count(stats.data.real_view(host[k]), g[k]) == 0, k


@pytest.mark.parametrize("fused", MODES)
@pytest.mark.parametrize("N", [(4, 4), (5, 130), (130, 5), (1, 9), (300, 2), (63, 65), (129, 7)])
def test_tiny_and_skinny_grids(oracle, N, fused):
    """Blocks narrower than a wave / shorter than a run, down to the smallest grid the mirror BC allows."""
    opts = dict(maxcycle=6)
    if min(N) < 4:
        opts.update(scheme="Godunov", projection="euler", nghost=2)     # LAG = 2 <= cells along each axis
        if min(N) < 2:
            opts.update(axis_splitting="Y_only" if N[0] < 2 else "X_only")
    params, stats, host = run("Sod_circ", N=N, use_fused_sweep=fused, **opts)
    orun, f = oracle.solve(test="Sod_circ", N=N, **opts)
    assert stats.cycles == orun.cycles and stats.last_dt == orun.last_dt
    g = opts.get("nghost", 4)
    for k in ("rho", "u", "v", "E", "p"):
        assert np.array_equal(stats.data.real_view(host[k]), oracle.real_view(f[k], N[0], N[1], g)), k


def test_tune_placement_keeps_the_state(oracle):
    """BlockGrid.tune_placement re-allocates the state vectors (measured choice of the HBM placement): the state
    and the results must not change, whichever draw wins."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test
    params = armon_amd.ArmonParameters(test="Sod_circ", N=(96, 64), silent=5, maxcycle=6, placement_tries=4)
    grid = BlockGrid(params)
    init_test(params, grid)                    # small block: tuning skipped by size
    assert grid.placement is None
    before = grid.device_to_host(("rho", "u", "v", "E"))
    rep = grid.tune_placement(min_bytes=0)
    assert rep and 2 <= rep["tries"] <= 4 and len(rep["x_plus_y_ms"]) == rep["tries"]
    after = grid.device_to_host(("rho", "u", "v", "E"))
    for f in before:
        assert np.array_equal(before[f], after[f])
    assert len({grid.data[f].ptr for f in before} | {grid.alt[f].ptr for f in before}) == 8
    # and whole runs with the placement chosen before init_test (armon_hip_choose_placement, what armon() does at
    # full size), forced here on a small block, or with no tuning at all, give the oracle's result
    ref, ref_fields = oracle.solve(test="Sod_circ", N=(96, 64), maxcycle=6)
    for opts in (dict(placement_tries=6, placement_min_bytes=0, placement_rounds=1),
                 dict(placement_tries=4, placement_min_bytes=0, placement_rounds=2), dict(placement_tries=1)):
        _p, stats, host = run("Sod_circ", N=(96, 64), maxcycle=6, **opts)
        assert stats.cycles == ref.cycles
        assert (stats.data.placement is not None) == (opts["placement_tries"] > 1)
        if stats.data.placement:
            rep = stats.data.placement
            assert rep["pool"] == 16 and rep["rounds"] == opts["placement_rounds"]   # a tiny block never reaches the fast mark
            assert rep["tries"] == opts["placement_tries"] * rep["rounds"]
            assert len(rep["x_plus_y_ms"]) == (rep["tries"] if rep["rounds"] == 1 else rep["rounds"])
        assert np.array_equal(oracle.real_view(host["rho"], 96, 64, G), oracle.real_view(ref_fields["rho"], 96, 64, G))
    # the staged path's counterpart: which allocation backs which of the 16 fields is chosen by timing staged cycles
    _p, stats, host = run("Sod_circ", N=(96, 64), maxcycle=6, use_fused_sweep=False, placement_tries=5, placement_min_bytes=0)
    rep = stats.data.placement
    assert rep and rep["staged"] and rep["tries"] == 5 and len(rep["cycle_ms"]) == 5 and rep["pool"] == 24
    assert stats.cycles == ref.cycles and stats.last_dt == ref.last_dt
    for k in ("rho", "u", "v", "E", "p"):
        assert np.array_equal(oracle.real_view(host[k], 96, 64, G), oracle.real_view(ref_fields[k], 96, 64, G)), k


@pytest.mark.parametrize("knobs", [dict(ARMON_SWEEP_ALIGN="0"), dict(ARMON_XS_NITER="1"), dict(ARMON_XS_NITER="3"),
                                   dict(ARMON_XS_NITER="137"), dict(ARMON_Y_SEG="16"), dict(ARMON_Y_SEG="1000"), dict(ARMON_X_XCD="1"),
                                   dict(ARMON_X_XCD="0"), dict(ARMON_X_ROWS="1"), dict(ARMON_X_ROWS="2"),
                                   dict(ARMON_Y_SX="1"), dict(ARMON_Y_SX="2")],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()))
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
def test_tuning_knobs_do_not_change_results(monkeypatch, knobs, exact):
    """Block/strip origins, strips per wave and rows per run only decide WHO computes a cell: every setting
    gives the same bits (in both arithmetic flavours)."""
    import contextlib
    from armon_amd import _lib
    opts = dict(N=(333, 77), maxcycle=9, exact_arithmetic=exact)
    _p, ref_stats, ref = run("Sod_circ", **opts)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    # several strips per wave (with a prefetch buffer) is the round-2 form of the X sweep: the A/B build carries it
    with (_lib.alt_kernels() if "ARMON_XS_NITER" in knobs else contextlib.nullcontext()):
        _p, stats, host = run("Sod_circ", **opts)
    assert stats.cycles == ref_stats.cycles and stats.last_dt == ref_stats.last_dt
    for k in ("rho", "u", "v", "E", "p"):
        assert np.array_equal(stats.data.real_view(host[k]), ref_stats.data.real_view(ref[k])), k


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("test,N,opts", [("Sod_circ", (328, 300), {}),                          # pitch 336: every row on a sector
                                         ("Sod_circ", (332, 300), {}),                          # 340: every other row mid-sector
                                         ("Sedov", (515, 263), dict(nghost=5)),                 # odd pitch, several workgroups per row
                                         ("Sod_circ", (700, 40), dict(axis_splitting="Godunov")),
                                         ("Bizarrium", (40, 600), dict(axis_splitting="Y_only"))])
def test_y_march_store_exchange_gives_the_same_bits(monkeypatch, test, N, opts, exact):
    """The Y march hands its rows over through LDS and stores sector-aligned windows when the pitch is not a multiple of a
    sector (ARMON_Y_SX=0, automatic), always (1) or never (2): who STORES a cell must not change it."""
    o = dict(N=N, maxcycle=7, exact_arithmetic=exact, **opts)
    monkeypatch.setenv("ARMON_Y_SX", "2")
    _p, s0, h0 = run(test, **o)
    for mode in ("1", "0"):
        monkeypatch.setenv("ARMON_Y_SX", mode)
        _p, s1, h1 = run(test, **o)
        assert s1.cycles == s0.cycles and s1.last_dt == s0.last_dt
        for k in ("rho", "u", "v", "E", "p"):
            assert np.array_equal(s1.data.real_view(h1[k]), s0.data.real_view(h0[k])), (mode, k)


@pytest.mark.parametrize("test,N", [("Sod_circ", (300, 200)), ("Sod_circ", (57, 61)), ("Sedov", (123, 77)), ("Sod", (8, 500)),
                                    ("Sod_y", (500, 9))])
def test_whole_cycle_kernel_equals_the_two_sweeps(test, N):
    """armon_hip_cycle_xy (X sweep + Y sweep in ONE pass over memory, the intermediate state in registers) gives the
    bits of armon_hip_sweep(X) followed by armon_hip_sweep(Y): state, fused dt reduction and the materialised p."""
    import ctypes as C
    import armon_amd
    from armon_amd import _lib
    from armon_amd.blocking import Axis
    from armon_amd.solver import STATE_VARS, BlockGrid, init_test, local_time_step, sweep_desc, update_EOS
    with _lib.alt_kernels() as L:        # the whole-cycle kernels live in the A/B build only (libarmon_hip_alt.so)
        _whole_cycle_check(L, test, N)


def _whole_cycle_check(L, test, N):
    import ctypes as C
    import armon_amd
    from armon_amd import _lib
    from armon_amd.blocking import Axis
    from armon_amd.solver import STATE_VARS, BlockGrid, init_test, local_time_step, sweep_desc, update_EOS
    params = armon_amd.ArmonParameters(test=test, N=N, silent=5, maxcycle=10)
    grid = BlockGrid(params)
    init_test(params, grid)
    dev = params.device
    dx, dy = params.cell_size(0), params.cell_size(1)
    update_EOS(params, grid)
    dt = params.cfl * local_time_step(params, grid)               # the reference's first time step
    for emit_p, form in ((False, 0), (True, 0), (False, 4), (True, 4)):       # form 4: producer / consumer waves
        d_x = sweep_desc(params, grid, Axis.X, dt, dx)
        d_y = sweep_desc(params, grid, Axis.Y, dt, dy, emit_dt=True, emit_p=emit_p)
        d_x.x_kernel = form
        _lib.check(L.armon_hip_cycle_xy(dev.ctx, C.byref(d_x), C.byref(d_y)))           # data -> alt
        d_x.x_kernel = 0
        got = {f: grid.alt[f].to_host() for f in STATE_VARS}
        got_dt = grid.dt_scalar.to_host()[0]
        got_p = grid.data["p"].to_host() if emit_p else None
        tmp = {f: dev.empty(grid.data[f].n, grid.data[f].dtype) for f in STATE_VARS}
        _lib.check(params.fn("sweep")(dev.ctx, C.byref(d_x)))                           # data -> alt
        d_y.rho_in, d_y.u_in, d_y.v_in, d_y.E_in = (grid.alt[f].ptr for f in STATE_VARS)
        d_y.rho_out, d_y.u_out, d_y.v_out, d_y.E_out = (tmp[f].ptr for f in STATE_VARS)
        _lib.check(params.fn("sweep")(dev.ctx, C.byref(d_y)))                           # alt -> tmp
        assert got_dt == grid.dt_scalar.to_host()[0]
        for f in STATE_VARS:
            assert np.array_equal(grid.real_view(got[f]), grid.real_view(tmp[f].to_host())), f
        if emit_p:
            assert np.array_equal(grid.real_view(got_p), grid.real_view(grid.data["p"].to_host()))
    # unsupported combinations are refused, not approximated
    d_x = sweep_desc(params, grid, Axis.X, dt, dx)
    d_y = sweep_desc(params, grid, Axis.Y, dt, dy)
    d_x.exact = d_y.exact = 1
    assert L.armon_hip_cycle_xy(dev.ctx, C.byref(d_x), C.byref(d_y)) != 0
    # ... mirror factors of another magnitude than 1 included, as by armon_hip_sweep, whose bits this entry point promises
    for axis, field in ((0, "u_factor_low"), (1, "v_factor_high")):
        d_x = sweep_desc(params, grid, Axis.X, dt, dx)
        d_y = sweep_desc(params, grid, Axis.Y, dt, dy)
        d = (d_x, d_y)[axis]
        assert d.bc_low == 1 and d.bc_high == 1
        setattr(d, field, -2.)
        assert L.armon_hip_cycle_xy(dev.ctx, C.byref(d_x), C.byref(d_y)) == 1 and b"mirror factors" in L.armon_hip_last_error()


def test_product_library_refuses_the_alternative_kernels():
    """libarmon_hip.so carries only what the solver runs: the rejected forms answer with an error, not with a kernel."""
    import ctypes as C
    import armon_amd
    from armon_amd import _lib
    from armon_amd.blocking import Axis
    from armon_amd.solver import BlockGrid, init_test, sweep_desc
    params = armon_amd.ArmonParameters(test="Sod", N=(64, 32), silent=5)
    grid = BlockGrid(params)
    init_test(params, grid)
    L = _lib.lib()
    d_x = sweep_desc(params, grid, Axis.X, 1e-4, params.cell_size(0))
    d_y = sweep_desc(params, grid, Axis.Y, 1e-4, params.cell_size(1))
    assert L.armon_hip_cycle_xy(params.device.ctx, C.byref(d_x), C.byref(d_y)) == 1
    assert b"libarmon_hip_alt.so" in L.armon_hip_last_error()
    for xk in (2, 3):
        d_x.x_kernel = xk
        assert L.armon_hip_sweep(params.device.ctx, C.byref(d_x)) == 1 and b"libarmon_hip_alt.so" in L.armon_hip_last_error()


# ---- parity gaps named by the round-2 review ------------------------------------------------------------------------
@pytest.mark.parametrize("test", ["Bizarrium", "Sedov"])
def test_fast_arithmetic_golden_bizarrium_sedov(test):
    """The TUNED arithmetic (what bench.py's headline runs) held directly against the reference's own golden results of
    the two cases its test suite runs without asserting (ref test/convergence.jl:24-27): cycle count exact, dt to 1e-12,
    every saved field to 1e-11 of its maximum (the exact arithmetic and the oracle sit at <= 6.4e-14 of it)."""
    g = load_golden(test)
    params, stats, host = run(test, use_fused_sweep=True, exact_arithmetic=False)
    assert stats.cycles == int(g["cycles"])
    assert abs(stats.last_dt - float(g["dt"])) <= 1e-12 * float(g["dt"])
    for k in ("rho", "u", "v", "p"):
        a = stats.data.real_view(host[k])
        assert np.abs(a - g[k]).max() <= 1e-11 * np.abs(g[k]).max(), f"{k}: {np.abs(a - g[k]).max() / np.abs(g[k]).max():.3e}"


@pytest.mark.parametrize("test,bound", [("Sod", 6e-13), ("Bizarrium", 1.5e-11)])
def test_whole_physical_run_tuned_vs_exact(test, bound):
    """How fast the two arithmetics of the SAME kernels may drift over a whole physical run (to the test's own maxtime,
    1024²; tools/long_run_cases.py at 2048²: 5.7e-14 on Sod after 944 cycles, 1.3e-12 on Bizarrium after 1546 — the bounds
    keep a decade of margin): equal cycle counts and final times, fields within `bound` of their maximum, rows identical
    (both cases vary along x only), mass and energy conserved on Sod."""
    import armon_amd
    from armon_amd.solver import BlockGrid, conservation_vars, init_test, time_loop
    n, out = 1024, {}
    for exact in (True, False):
        params = armon_amd.ArmonParameters(test=test, N=(n, n), silent=5, exact_arithmetic=exact)
        grid = BlockGrid(params)
        init_test(params, grid)
        m0, e0 = conservation_vars(params, grid)
        t, dt, cycles, _, _ = time_loop(params, grid)
        m1, e1 = conservation_vars(params, grid)
        f = {k: grid.real_view(grid.data[k].to_host()).copy() for k in ("rho", "u", "v", "E")}
        for k, a in f.items():
            assert np.isfinite(a).all() and np.array_equal(a, np.broadcast_to(a[0:1], a.shape)), (exact, k)
        if test == "Sod":
            assert abs(m1 - m0) <= 1e-12 and abs(e1 - e0) <= 1e-12, (exact, m1 - m0, e1 - e0)
        out[exact] = (f, cycles, t, dt)
    (fe, ce, te, de), (ft, ct, tt, dtt) = out[True], out[False]
    assert ce == ct and ce > 300
    assert abs(tt - te) <= 1e-12 * te and abs(dtt - de) <= 1e-11 * de
    for k in fe:
        dev = np.abs(fe[k] - ft[k]).max() / max(np.abs(fe[k]).max(), 1e-300)
        assert dev <= bound, f"{k}: {dev:.3e}"


def _one_bad_cell(grid, params, ix, iy):
    """E = -1 in ONE real cell: its internal energy, hence its sound speed, is not a number any more."""
    g = params.nghost
    a = grid.data["E"].to_host()
    a.reshape(params.block_size.size[1], params.block_size.size[0])[g + iy, g + ix] = -1.0
    grid.data["E"].copy_from_host(a)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_nan_cell_reaches_the_staged_dt_reduction(dtype):
    """ref src/solver_state.jl:123-124 raises on the first non-finite time step. One NaN sound speed among 4096 cells must
    not be dropped by the maxima of the dtCFL reduction."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test, time_loop
    params = armon_amd.ArmonParameters(test="Sod", N=(64, 64), maxcycle=3, silent=5, use_fused_sweep=False, data_type=dtype)
    grid = BlockGrid(params)
    init_test(params, grid)
    _one_bad_cell(grid, params, 37, 11)
    with pytest.raises(armon_amd.SolverException) as e:
        time_loop(params, grid)
    assert e.value.category == "time"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tuned"])
@pytest.mark.parametrize("axis_name", ["X", "Y"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_nan_cell_reaches_the_fused_dt_reduction(axis_name, exact, dtype):
    """The dt/CFL tracking of the fused sweeps (cfl_track, per-wave / per-workgroup maxima, the fold kernels): a sweep over
    a state with ONE bad cell must leave a NaN step in the device scalar — in one launch, and as interior + strips with
    dt_accumulate (the strips are clean there, the NaN must survive the accumulation)."""
    import armon_amd
    from armon_amd.blocking import Axis
    from armon_amd.solver import BlockGrid, fused_sweep, init_test, sweep_lag
    N = (300, 70)
    axis = Axis.X if axis_name == "X" else Axis.Y
    n = N[int(axis) - 1]
    for split in (False, True):
        params = armon_amd.ArmonParameters(test="Sod_circ", N=N, silent=5, exact_arithmetic=exact, data_type=dtype)
        grid = BlockGrid(params)
        init_test(params, grid)
        lag = sweep_lag(params)
        dx, dt = 1.0 / n, 0.2 / n
        fused_sweep(params, grid, axis, dt, dx, emit_dt=True)              # a clean sweep first: a finite step
        assert np.isfinite(float(grid.dt_scalar.to_host()[0]))
        _one_bad_cell(grid, params, 150, 35)
        if not split:
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True)
        else:
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, out_range=(lag, n - lag), swap=False)
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, out_range=(0, lag), swap=False, dt_accumulate=True)
            fused_sweep(params, grid, axis, dt, dx, emit_dt=True, out_range=(n - lag, n), swap=False, dt_accumulate=True)
        assert np.isnan(float(grid.dt_scalar.to_host()[0])), (split, float(grid.dt_scalar.to_host()[0]))


def test_invalid_time_step_is_reported_by_the_fused_path():
    """Whole solver, fused sweeps: the state goes bad in ONE cell after cycle 0 (whose step comes from the staged dtCFL
    kernel); the next cycles' steps come from the sweeps' own tracking and the deferred read-back, and the run must stop
    with SolverException(:time) as the reference does (ref src/solver_state.jl:123-124)."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test, solver_cycle
    params = armon_amd.ArmonParameters(test="Sod_circ", N=(96, 64), maxcycle=20, silent=5, use_fused_sweep=True)
    grid = BlockGrid(params)
    init_test(params, grid)
    gdt = grid.global_dt
    gdt.reset()
    solver_cycle(params, grid, last_cycle=False)
    gdt.next_cycle()
    params.wait()
    _one_bad_cell(grid, params, 40, 30)
    with pytest.raises(armon_amd.SolverException) as e:
        for _ in range(4):
            solver_cycle(params, grid, last_cycle=False)
            gdt.next_cycle()
    assert e.value.category == "time" and gdt.cycle <= 3


@pytest.mark.parametrize("force_peer", [False, True], ids=["direct", "peer_copies"])
def test_invalid_time_step_is_reported_by_a_tile_group(force_peer):
    """Same through a 2 x 2 tile group: the NaN sits in ONE tile and has to win the group's dt reduction (the one-kernel
    form and the gather / fold / scatter form) and the edge fold."""
    import armon_amd
    from armon_amd.multi_tile import TileGroup
    group = TileGroup((2, 2), test="Sod_circ", N=(96, 64), maxcycle=20, silent=5, use_fused_sweep=True, force_peer_copy=force_peer)
    try:
        group.init_test()
        gdt = group.global_dt
        gdt.reset()
        group.solver_cycle(last_cycle=False)
        gdt.next_cycle()
        group.wait()
        _one_bad_cell(group.grids[2], group.params[2], 20, 10)
        with pytest.raises(armon_amd.SolverException) as e:
            for _ in range(4):
                group.solver_cycle(last_cycle=False)
                gdt.next_cycle()
        assert e.value.category == "time" and gdt.cycle <= 3
    finally:
        group.close()


@pytest.mark.parametrize("fused", MODES)
def test_animation_frames_and_slices(tmp_path, fused):
    """animation_step (ref src/solver.jl:373-378: a frame after next_cycle! whenever (cycle - 1) % step == 0, in
    anim/<output_file>_<frame:03d>, the directory emptied first, :436-442) and write_slices (ref src/parameters.jl:229-232:
    middle X row, middle Y column, diagonal). A frame written after cycle c equals the output of a run that stops at c."""
    import os
    import armon_amd
    from armon_amd import io as aio
    N = (40, 28)
    common = dict(test="Sod_circ", N=N, silent=5, use_fused_sweep=fused, exact_arithmetic=True, output_dir=str(tmp_path))
    os.makedirs(tmp_path / "anim")
    (tmp_path / "anim" / "stale_000").write_text("left over from an earlier run\n")
    params = armon_amd.ArmonParameters(maxcycle=8, animation_step=3, write_slices=True, write_output=True, output_file="run",
                                       **common)
    armon_amd.armon(params)
    assert sorted(os.listdir(tmp_path / "anim")) == ["run_000", "run_001", "run_002"]
    for frame, cycle in ((0, 1), (1, 4), (2, 7)):
        p2 = armon_amd.ArmonParameters(maxcycle=cycle, write_output=True, output_file=f"stop{cycle}", **common)
        armon_amd.armon(p2)
        a = aio.read_sub_domain_file(params, os.path.join("anim", f"run_{frame:03d}"))
        b = aio.read_sub_domain_file(p2, f"stop{cycle}")
        for k in aio.SAVED_VARS:
            assert np.array_equal(a[k], b[k], equal_nan=True), (frame, k)
    full = aio.read_sub_domain_file(params, "run")
    g, sx = params.nghost, N[0] + 2 * params.nghost
    cols = np.stack([np.asarray(full[k]).reshape(-1, sx)[g:g + N[1], g:g + N[0]] for k in aio.SAVED_VARS], axis=-1)
    load = lambda tag: np.array([[float(t) for t in line.split(",")] for line in open(tmp_path / f"run_{tag}")])
    assert np.array_equal(load("X"), cols[N[1] // 2]) and np.array_equal(load("Y"), cols[:, N[0] // 2])
    assert np.array_equal(load("diag"), np.array([cols[k, k] for k in range(min(N))]))


@pytest.mark.parametrize("dtype,offset", [("float64", 8), ("float64", 32), ("float32", 4), ("float32", 40)])
@pytest.mark.parametrize("N", [(333, 300), (328, 300), (700, 64)])
def test_vectors_that_do_not_start_on_a_sector(N, dtype, offset):
    """Arrays handed over as views into larger allocations (8 … 40 bytes past a 64-B sector): the sector-aligned forms
    (row-by-row strip origins, the Y march's LDS hand-over, 16-B accesses) must step aside for the plain ones — same bits
    as on ordinary allocations."""
    import armon_amd
    from armon_amd.device import DeviceArray
    from armon_amd.solver import BlockGrid, init_test, time_loop
    opts = dict(test="Sod_circ", N=N, maxcycle=6, silent=5, exact_arithmetic=False, data_type=dtype)
    results = []
    for shifted in (False, True):
        params = armon_amd.ArmonParameters(**opts)
        grid = BlockGrid(params)
        owners = []
        if shifted:
            def shifted_view(v):
                big = params.device.empty(v.n + 64, v.dtype)
                owners.append(big)
                a = DeviceArray.__new__(DeviceArray)
                a.device, a.n, a.dtype, a.nbytes = big.device, v.n, v.dtype, v.nbytes
                a.ptr, a.owner = big.ptr + offset, big
                return a
            for f, v in list(grid.data.items()):          # in place: grid.data also creates c, g when cycle 0 asks for them
                grid.data[f] = shifted_view(v)
            grid.alt = {f: shifted_view(v) for f, v in grid.alt.items()}
        init_test(params, grid)
        _t, dt, cycles, _, _ = time_loop(params, grid)
        results.append((cycles, dt, {k: grid.real_view(grid.data[k].to_host()).copy() for k in ("rho", "u", "v", "E")}))
        del grid, owners
    assert results[0][0] == results[1][0] and results[0][1] == results[1][1]
    for k in results[0][2]:
        assert np.array_equal(results[0][2][k], results[1][2][k]), k


def test_fused_path_allocates_only_what_it_touches():
    """the nine staged-only vectors are created on first access on the fused path (c, g by cycle 0's EOS +
    dtCFL, released right after), the BlockData of the C ABI stays 16 pointers, and whatever is created later holds what
    init_test would have left in it."""
    import armon_amd
    from armon_amd.solver import BlockGrid, init_test, time_loop, FUSED_FIELDS
    params = armon_amd.ArmonParameters(test="Sod_circ", N=(96, 64), maxcycle=6, silent=5)
    grid = BlockGrid(params)
    assert set(grid.data) == set(FUSED_FIELDS) and grid.memory_required() == 11 * grid.size.n_cells * 8
    init_test(params, grid)
    assert set(grid.data) == set(FUSED_FIELDS)
    time_loop(params, grid)
    assert set(grid.data) == set(FUSED_FIELDS), set(grid.data)          # c, g came and went
    g, (nx, ny) = grid.size.ghosts, grid.size.real_size
    mask = grid.data["mask"].to_host().reshape(ny + 2 * g, nx + 2 * g)  # created now, with its initial content
    assert mask[g:g + ny, g:g + nx].all() and mask.sum() == nx * ny
    assert not grid.data["work_3"].to_host().any() and "work_3" in grid.lazy
    # and the staged path keeps the reference's 16
    p2 = armon_amd.ArmonParameters(test="Sod_circ", N=(96, 64), maxcycle=6, silent=5, use_fused_sweep=False)
    assert len(BlockGrid(p2).data) == 16
