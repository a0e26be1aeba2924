"""tests/staged_reference.py, the inputs of the staged-kernel GPU tests, against the CPU oracle alone (no GPU).

A helper that draws a range outside its arrays, a "planted extreme" that does not decide the reduction, a sum that is not exact
or a comparison that lets one ulp through would make the GPU tests that use it pass for the wrong reason."""
import ctypes as C

import numpy as np
import pytest

import staged_reference as S

KERNEL_SHAPES = [(37, 29), (128, 3), (5, 70), (257, 64)]            # tests/test_gpu_kernels_f32.py
SUM_SHAPES = [(37, 29), (257, 64), (1000, 16)]                      # tests/test_gpu_reductions_edges.py
EDGE_SHAPES = [(37, 29), (128, 3), (5, 70), (1027, 6), (600, 7)]
DTYPES = [np.float32, np.float64]


def lib_of(oracle, dtype):
    L = oracle.lib(f32=np.dtype(dtype) == np.float32)
    L.armon_oracle_set_threads(1)
    return L


def oracle_sums(oracle, dtype, nx, ny, g, rho, E, ds):
    T = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    out = (T * 2)()
    lib_of(oracle, dtype).armon_oracle_conservation_vars(oracle.domain_range(nx, ny, g), ds, oracle.ptr(rho), oracle.ptr(E),
                                                         C.byref(out))
    return out[0], out[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", sorted(set(KERNEL_SHAPES + SUM_SHAPES)))
def test_dyadic_sums_are_exact_in_both_oracles(oracle, shape, dtype):
    nx, ny = shape
    for g in (4, 5):
        rho, E, ds = S.dyadic_state(nx, ny, g, dtype, seed=nx + ny + g)
        assert rho.dtype == dtype and E.dtype == dtype and np.log2(float(ds)) % 1 == 0
        want = S.exact_sums(rho, E, ds, nx, ny, g)
        got = oracle_sums(oracle, dtype, nx, ny, g, rho, E, ds)
        assert np.array_equal(np.array(got, dtype=np.float64).view(np.uint64), np.array(want).view(np.uint64)), (got, want)
        # the ghost cells are drawn too, and are not part of the sums
        assert want[0] != float(np.sum(rho.astype(np.float64)) * float(ds))


def test_dyadic_state_refuses_a_shape_whose_sums_outgrow_fp32():
    with pytest.raises(AssertionError):
        S.dyadic_state(1000, 700, 4, np.float32, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", [4, 5])
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_a_planted_extreme_decides_the_oracles_dtCFL(oracle, shape, g, dtype):
    nx, ny = shape
    L = lib_of(oracle, dtype)
    T = np.dtype(dtype).type
    f = S.rand_fields(nx, ny, g, dtype, seed=11)
    r = oracle.domain_range(nx, ny, g)
    positions = S.EXTREME_POSITIONS(nx, ny)
    assert len(positions) >= 4 and len({(row, col) for _w, row, col in positions}) == len(positions)
    for what, row, col in positions:
        i = S.flat_index(nx, g, row, col)
        for name, (dx, dy) in (("u", (0.01, 0.02)), ("v", (0.02, 0.01))):
            a = f[name].copy()
            a[i] = S.PLANTED
            u, v = (a, f["v"]) if name == "u" else (f["u"], a)
            got = T(L.armon_oracle_dtCFL(r, dx, dy, oracle.ptr(u), oracle.ptr(v), oracle.ptr(f["c"])))
            want = S.cfl_closed_form(dx if name == "u" else dy, S.PLANTED, f["c"][i])
            assert got == want, (what, name, got, want)
            # ... and with the other axis' cell size far smaller, the other axis' extreme wins: the unplanted maximum
            dx2, dy2 = (1.0, 0.01) if name == "u" else (0.01, 1.0)
            got = T(L.armon_oracle_dtCFL(r, dx2, dy2, oracle.ptr(u), oracle.ptr(v), oracle.ptr(f["c"])))
            other = f["v"] if name == "u" else f["u"]
            rv = lambda x: S.real_view(x, nx, ny, g)
            assert got == T(0.01) / np.max(np.abs(rv(other)) + rv(f["c"])), (what, name)


def test_extreme_positions_hold_every_class():
    pos = {what: (row, col) for what, row, col in S.EXTREME_POSITIONS(1027, 6)}
    assert pos["odd tail of a row"] == (3, 1026) and pos["last pair .x"] == (3, 1024) and pos["last pair .y"] == (3, 1025)
    assert [pos[f"cell {k} of a row"] for k in (511, 512, 513)] == [(3, 511), (3, 512), (3, 513)]
    assert pos["first row of the last group of rows"] == (4, 513) and pos["last row of the last group of rows"] == (5, 513)
    assert pos["first pair .x"] == (3, 0) and pos["first pair .y"] == (3, 1)
    assert {pos[k] for k in pos if "cell of the" in k} == {(0, 0), (0, 1026), (5, 0), (5, 1026)}
    even = [what for what, _r, _c in S.EXTREME_POSITIONS(128, 4)]
    assert "odd tail of a row" not in even and not any("group" in w or "cell 5" in w for w in even)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seed", [4242, 1, 77])
def test_drawn_ranges_stay_inside_and_cover_the_x_forms(seed, dtype):
    per_sector, wave, group = S.x_form_layout(dtype)
    assert (per_sector, wave, group) == ((16, 48, 192) if dtype == np.float32 else (8, 56, 224))
    cases = S.draw_range_cases(seed, 40, dtype)
    assert len(cases) == 40 and cases == S.draw_range_cases(seed, 40, dtype)
    assert {c[5] for c in cases} == {0, 1} and {c[6] for c in cases} == {0, 1, 2} and {c[2] for c in cases} <= set(S.GHOSTS)
    xs = [c for c in cases if c[5] == 0]
    assert {S.strip_origin(*c[:6], dtype) for c in xs} == set(range(per_sector))
    lengths = sorted(S.range_of(*c[:6])[4] for c in xs)
    for edge in (wave, group, 2 * group):
        assert lengths[0] < edge < lengths[-1]
    for nx, ny, g, lo, hi, axis in (c[:6] for c in cases):
        S.assert_stencil_inside(nx, ny, g, lo, hi, axis)
        # the same bound, cell by cell: the outermost cells of the stencil of the first and the last cell of the range
        col_start, col_step, col_len, row_start, row_len = S.range_of(nx, ny, g, lo, hi, axis)
        assert (col_start, col_step, col_len, row_start, row_len) == tuple(
            getattr(_oracle_range(nx, ny, g, lo, hi, axis), k) for k in ("col_start", "col_step", "col_len", "row_start", "row_len"))
        s = 1 if axis == 0 else col_step
        n = (nx + 2 * g) * (ny + 2 * g)
        assert col_start + row_start - 2 * s >= 0
        assert col_start + (col_len - 1) * col_step + row_start + row_len - 1 + 2 * s <= n - 1
    with pytest.raises(AssertionError):
        S.assert_stencil_inside(10, 10, 3, -2, 0, 0)           # two cells below a ghost width of 3: the stencil leaves the row
    with pytest.raises(AssertionError):
        S.assert_stencil_inside(10, 10, 2, 0, 1, 1)
    with pytest.raises(AssertionError):
        S.assert_range_coverage([c for c in cases if S.strip_origin(*c[:6], dtype) != 3 or c[5] == 1], dtype)
    with pytest.raises(AssertionError):
        S.assert_range_coverage([c for c in cases if c[5] == 1 or S.range_of(*c[:6])[4] < group], dtype)


def _oracle_range(nx, ny, g, lo, hi, axis):
    from oracle import oracle as O
    return O.domain_range(nx, ny, g, *(((lo, 0), (hi, 0)) if axis == 0 else ((0, lo), (0, hi))))


@pytest.mark.parametrize("dtype", DTYPES)
def test_assert_bits_equal_sees_one_ulp_signs_and_cells_outside_a_range(oracle, dtype):
    nx, ny, g = 37, 29, 4
    pitch = nx + 2 * g
    f = S.rand_fields(nx, ny, g, dtype, seed=3)
    r = oracle.domain_range(nx, ny, g, (-2, 0), (2, 0))
    rng = (r.col_start, r.col_step, r.col_len, r.row_start, r.row_len)
    want = f["us"]
    S.assert_bits_equal(want.copy(), want, "us", pitch, rng)
    inside = r.col_start + 3 * r.col_step + r.row_start + 5
    got = want.copy()
    got[inside] = np.nextafter(got[inside], dtype(np.inf))
    with pytest.raises(AssertionError, match=rf"row {g + 3}, column {g - 2 + 5}\) inside the range"):
        S.assert_bits_equal(got, want, "us", pitch, rng)
    for outside, col in ((r.col_start + r.row_start - 1, g - 3), (r.col_start + r.row_start + r.row_len, g + nx + 2)):
        got = want.copy()
        got[outside] = np.nextafter(got[outside], dtype(np.inf))
        with pytest.raises(AssertionError, match=rf"row {g}, column {col}\) OUTSIDE the range"):
            S.assert_bits_equal(got, want, "us", pitch, rng)
    above = r.col_start + r.col_len * r.col_step + r.row_start            # the first cell of the row after the last
    got = want.copy()
    got[above] = 0
    with pytest.raises(AssertionError, match="OUTSIDE"):
        S.assert_bits_equal(got, want, "us", pitch, rng)
    zero, nan = np.zeros(4, dtype), np.full(4, np.nan, dtype)
    S.assert_bits_equal(nan.copy(), nan, "nan")                           # the same NaN is equal
    with pytest.raises(AssertionError, match="index 2"):
        S.assert_bits_equal(np.array([0, 0, -0.0, 0], dtype), zero, "zero")
    other_nan = nan.copy()
    other_nan.view(S.bits(nan).dtype)[1] ^= 1                             # another payload
    with pytest.raises(AssertionError, match="index 1"):
        S.assert_bits_equal(other_nan, nan, "payload")
    with pytest.raises(AssertionError):
        S.assert_bits_equal(zero.astype(np.float64 if dtype == np.float32 else np.float32), zero, "dtype")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rand_fields_are_the_fields_of_the_fp64_kernel_tests(dtype):
    """Same draws as test_gpu_kernels.rand_state at its ghost width, rounded once; any other ghost width just changes the size."""
    from sweep_reference import draw_state
    nx, ny, g = 21, 13, 4
    rng = np.random.default_rng(9)
    n = (nx + 2 * g) * (ny + 2 * g)
    want = {**draw_state(rng, n, "perfect_gas"), "p": rng.uniform(0.1, 2.0, n), "c": rng.uniform(0.5, 2.0, n)}
    got = S.rand_fields(nx, ny, g, dtype, 9)
    for k, a in want.items():
        assert got[k].dtype == dtype and np.array_equal(got[k], a.astype(dtype)), k
    assert set(got) == {"rho", "u", "v", "E", "p", "c", "g", "us", "ps", "work_1", "work_2", "work_3", "work_4"}
    assert S.rand_fields(nx, ny, 6, dtype, 9)["rho"].size == (nx + 12) * (ny + 12)
    biz = S.rand_fields(nx, ny, 3, dtype, 9, eos="bizarrium")
    assert biz["rho"].min() > 0.9e4 and biz["E"].min() >= 1e6
