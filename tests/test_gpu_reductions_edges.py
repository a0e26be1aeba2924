"""The two staged reductions, dtCFL and conservation_vars, at the cells and values where a reduction goes wrong unnoticed.

dtCFL reads two cells per lane (16-B loads in fp64, 8-B in fp32) on the rows that start on such a boundary in all three arrays,
one cell per lane on the others, lets thread 0 pick up the odd last cell, gives a workgroup at least 4 consecutive rows, and
returns min(dx / max a, dy / max b) instead of a per-cell minimum. On uniformly random states the cell that decides the result
almost never sits where these paths differ. Here it is PLANTED there: one cell with a velocity of -7.3 in a state whose other
cells stay below 3 makes the result ``d / (|-7.3| + c)`` of that one cell, which the test computes itself. conservation_vars is
checked on states whose sums are exact in any order (tests/staged_reference.dyadic_state): bit-equal, and one cell moved by
1/8 moves the sum by exactly that.
"""
import ctypes as C

import numpy as np
import pytest

import staged_reference as S
from oracle import oracle as O
from staged_reference import Precision, conv

pytestmark = pytest.mark.gpu

EDGE_SHAPES = [(37, 29), (128, 3), (5, 70), (1027, 6), (600, 7)]      # even and odd pitch: rows alternate between the two paths
SUM_SHAPES = [(37, 29), (257, 64), (1000, 16)]
GHOSTS = [4, 5]
BOTH = [pytest.param(np.float32, id="f32"), pytest.param(np.float64, id="f64")]
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    import armon_amd
    from armon_amd.device import HIPDevice
    d = HIPDevice(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def L():
    import armon_amd
    return armon_amd.lib()


def same_bits(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return a.dtype == b.dtype and np.array_equal(S.bits(a), S.bits(b))


class CflState:
    """u, v, c of one block on the host and on the device — each also one element into a larger allocation, which moves
    every row of it off the boundary it had — with single cells that can be set on all copies at once."""

    def __init__(self, P, dev, nx, ny, g, fields):
        self.P, self.dev, self.nx, self.ny, self.g = P, dev, nx, ny, g
        self.size = P.dtype().itemsize
        self.host = {k: fields[k].copy() for k in "uvc"}
        self.base = {k: fields[k].copy() for k in "uvc"}
        self.at0 = {k: dev.from_host(a) for k, a in self.host.items()}
        self.at1 = {k: dev.from_host(np.concatenate([a[:1], a])) for k, a in self.host.items()}
        self.out = dev.zeros(1, P.dtype)
        self.r = O.domain_range(nx, ny, g)

    def set(self, name, i, value):
        from armon_amd._lib import check
        self.host[name][i] = value
        one = np.array([value], self.P.dtype)
        for arr, lead in ((self.at0[name], 0), (self.at1[name], 1)):
            check(self.P.L.armon_hip_memcpy(self.dev.ctx, C.c_void_p(arr.ptr + (i + lead) * self.size),
                                            one.ctypes.data_as(C.c_void_p), self.size, 1))

    def restore(self, name, i):
        self.set(name, i, self.base[name][i])

    def pointers(self, shifted=""):
        return [C.c_void_p(self.at1[k].ptr + self.size) if k in shifted else C.c_void_p(self.at0[k].ptr) for k in "uvc"]

    def oracle(self, dx, dy):
        return self.P.dtype(self.P.ref("dtCFL")(self.r, dx, dy, *(O.ptr(self.host[k]) for k in "uvc")))

    def device(self, dx, dy, shifted=""):
        """(armon_hip_dtCFL, armon_hip_dtCFL_async) of the current state."""
        P = self.P
        out = P.real(-1.)
        assert P.hip("dtCFL")(self.dev.ctx, conv(self.r), dx, dy, *self.pointers(shifted), C.byref(out)) == 0
        assert P.hip("dtCFL_async")(self.dev.ctx, conv(self.r), dx, dy, *self.pointers(shifted), C.c_void_p(self.out.ptr)) == 0
        self.dev.wait()
        return P.dtype(out.value), self.out.to_host()[0]

    def expect(self, want, dx, dy, what, shifted=""):
        for entry, got in zip(("dtCFL", "dtCFL_async"), self.device(dx, dy, shifted)):
            assert same_bits(got, want), (entry, what, shifted, got, want)


def cfl_state(P, dev, nx, ny, g, seed=11, zero=False):
    f = S.rand_fields(nx, ny, g, P.dtype, seed)
    if zero:
        f = {k: np.zeros_like(f[k]) for k in "uvc"}
    return CflState(P, dev, nx, ny, g, f)


# cell sizes with which the extreme along x decides the result, and with which the one along y does
X_WINS, Y_WINS = (0.01, 0.02), (0.02, 0.01)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_dtCFL_finds_an_extreme_planted_where_a_path_ends(dev, L, shape, g, dtype):
    nx, ny = shape
    P = Precision(L, dtype)
    st = cfl_state(P, dev, nx, ny, g)
    T = P.dtype
    rv = lambda a: S.real_view(a, nx, ny, g)
    for what, row, col in S.EXTREME_POSITIONS(nx, ny):
        i = S.flat_index(nx, g, row, col)
        for name, wins, loses in (("u", X_WINS, (1.0, 0.01)), ("v", Y_WINS, (0.01, 1.0))):
            st.set(name, i, S.PLANTED)
            want = S.cfl_closed_form(wins[0] if name == "u" else wins[1], S.PLANTED, st.host["c"][i])
            assert same_bits(st.oracle(*wins), want), (what, name)
            st.expect(want, *wins, (what, name))
            # the other axis' cell size far smaller: the largest |velocity| + c of the other, unplanted axis decides
            other = st.host["v" if name == "u" else "u"]
            want = T(0.01) / np.max(np.abs(rv(other)) + rv(st.host["c"]))
            assert same_bits(st.oracle(*loses), want), (what, name)
            st.expect(want, *loses, (what, name, "other axis"))
            st.restore(name, i)
    st.expect(st.oracle(*X_WINS), *X_WINS, "restored")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", EDGE_SHAPES)
def test_dtCFL_on_arrays_one_element_into_an_allocation(dev, L, shape, g, dtype):
    """One array off its boundary puts every row on the one-cell-per-lane path; all three off it swap the rows that take the
    pair loads with those that do not. The planted cell decides the result either way: the same bits."""
    nx, ny = shape
    P = Precision(L, dtype)
    st = cfl_state(P, dev, nx, ny, g, seed=12)
    for what, row, col in S.EXTREME_POSITIONS(nx, ny):
        i = S.flat_index(nx, g, row, col)
        for name, wins in (("u", X_WINS), ("v", Y_WINS)):
            st.set(name, i, S.PLANTED)
            want = S.cfl_closed_form(wins[0] if name == "u" else wins[1], S.PLANTED, st.host["c"][i])
            for shifted in ("u", "v", "c", "uvc"):
                st.expect(want, *wins, (what, name), shifted)
            st.restore(name, i)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", [(37, 29), (1027, 6)])
def test_dtCFL_signs_and_zeros_at_a_planted_cell(dev, L, shape, g, dtype):
    """|u| + |c| stands for max(|u + c|, |u - c|) in the kernel: also for a negative c that outweighs u, for c = 0 and for
    u = -0.0. Finite results are the oracle's, which evaluates the reference's expression."""
    nx, ny = shape
    P = Precision(L, dtype)
    T = P.dtype
    st = cfl_state(P, dev, nx, ny, g, seed=13)
    zeros = cfl_state(P, dev, nx, ny, g, zero=True)
    for what, row, col in S.EXTREME_POSITIONS(nx, ny):
        i = S.flat_index(nx, g, row, col)
        for cells in (dict(u=0.5, c=-9.25), dict(u=-0.5, c=-9.25), dict(v=0.25, c=-8.5),    # c < 0, |c| > |u|
                      dict(u=-0.0, c=9.5), dict(v=-0.0, c=9.5),
                      dict(u=-7.3, c=0.), dict(v=7.3, c=0.), dict(u=-7.3, v=-0.0, c=-0.0)):  # c = 0, u != 0
            for k, x in cells.items():
                st.set(k, i, x)
            for sizes in (X_WINS, Y_WINS):
                want = st.oracle(*sizes)
                a = abs(T(st.host["u"][i])) + abs(T(st.host["c"][i]))
                b = abs(T(st.host["v"][i])) + abs(T(st.host["c"][i]))
                with np.errstate(divide="ignore"):
                    closed = min(T(sizes[0]) / a, T(sizes[1]) / b)
                assert np.isfinite(want) and same_bits(want, closed), (what, cells)
                st.expect(want, *sizes, (what, cells))
            for k in cells:
                st.restore(k, i)
        # nothing moves anywhere, one velocity is -0.0: dx / |0| = +inf, never -inf
        zeros.set("u", i, -0.0)
        assert same_bits(zeros.oracle(*X_WINS), T(np.inf))
        zeros.expect(T(np.inf), *X_WINS, (what, "-0.0 in a state at rest"))
        zeros.restore("u", i)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", [(37, 29), (1027, 6)])
def test_dtCFL_of_a_subnormal_speed(dev, L, shape, g, dtype):
    """One cell of a state at rest moves at a subnormal speed, with cell sizes small enough for ``dx / speed`` to be finite:
    the reduction keeps the subnormal, the division takes it. Neither side flushes it to zero (the library's build sets no
    denormal-flushing option, nor does the oracle's): on an MI355X the result is the oracle's and the closed form's to the bit
    in both precisions, so nothing is excused here."""
    nx, ny = shape
    P = Precision(L, dtype)
    T = P.dtype
    tiny = np.finfo(dtype).smallest_subnormal * T(5)
    d = T(2.) ** (-20 if dtype == np.float32 else -60)
    assert 0 < tiny < np.finfo(dtype).tiny and np.isfinite(d / tiny)
    st = cfl_state(P, dev, nx, ny, g, zero=True)
    for what, row, col in S.EXTREME_POSITIONS(nx, ny):
        i = S.flat_index(nx, g, row, col)
        for cells in (dict(u=-tiny), dict(v=tiny), dict(u=tiny, c=-tiny), dict(c=tiny)):
            for k, x in cells.items():
                st.set(k, i, x)
            a = abs(st.host["u"][i]) + abs(st.host["c"][i])
            b = abs(st.host["v"][i]) + abs(st.host["c"][i])
            with np.errstate(divide="ignore"):
                want = min(d / a, d / b)
            assert np.isfinite(want) and same_bits(st.oracle(float(d), float(d)), want), (what, cells)
            st.expect(want, float(d), float(d), (what, cells))
            for k in cells:
                st.restore(k, i)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", [(37, 29), (128, 3), (1027, 6)])
def test_dtCFL_returns_nan_for_a_nan_in_any_cell_of_any_array(dev, L, shape, g, dtype):
    """The reference's ``min`` propagates a NaN to the time step, where ``Invalid time step`` stops the run (ref
    src/solver_state.jl:123). That is the expectation here, not the oracle's value: its ``mn`` drops a NaN that comes last."""
    nx, ny = shape
    P = Precision(L, dtype)
    st = cfl_state(P, dev, nx, ny, g, seed=14)
    for what, row, col in S.EXTREME_POSITIONS(nx, ny):
        i = S.flat_index(nx, g, row, col)
        for name in "uvc":
            st.set(name, i, np.nan)
            for sizes in (X_WINS, Y_WINS):
                for entry, got in zip(("dtCFL", "dtCFL_async"), st.device(*sizes)):
                    assert np.isnan(got), (entry, what, name, got)
            st.restore(name, i)
    st.expect(st.oracle(*X_WINS), *X_WINS, "restored")


# ---- conservation_vars ----------------------------------------------------------------------------------------------------
def conservation(P, dev, nx, ny, g, ds, rho, E):
    out = (P.real * 2)(-1., -1.)
    assert P.hip("conservation_vars")(dev.ctx, conv(O.domain_range(nx, ny, g)), float(ds), C.c_void_p(rho.ptr), C.c_void_p(E.ptr),
                                      C.byref(out)) == 0
    return np.array([out[0], out[1]], P.dtype)


def poke(P, dev, arr, i, value):
    from armon_amd._lib import check
    one = np.array([value], P.dtype)
    check(P.L.armon_hip_memcpy(dev.ctx, C.c_void_p(arr.ptr + i * one.itemsize), one.ctypes.data_as(C.c_void_p), one.itemsize, 1))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", SUM_SHAPES)
def test_conservation_sums_are_exact_on_dyadic_states(dev, L, shape, g, dtype):
    """Sums that are exact in any order leave no room for a tolerance: a cell counted twice, skipped or paired with the wrong
    E changes a bit. One real cell more by 1/8 moves the mass by ds/8 and the energy by ds·E/8; a ghost cell moves nothing."""
    nx, ny = shape
    P = Precision(L, dtype)
    rho, E, ds = S.dyadic_state(nx, ny, g, dtype, seed=5)
    mass, energy = S.exact_sums(rho, E, ds, nx, ny, g)
    d_rho, d_E = dev.from_host(rho), dev.from_host(E)
    exact = lambda m, e: np.array([m, e], np.float64).astype(dtype)
    assert np.array_equal(exact(mass, energy).astype(np.float64), [mass, energy])          # representable as they are
    got = conservation(P, dev, nx, ny, g, ds, d_rho, d_E)
    assert same_bits(got, exact(mass, energy)), (got, mass, energy)
    for what, row, col in S.EXTREME_POSITIONS(nx, ny):
        i = S.flat_index(nx, g, row, col)
        poke(P, dev, d_rho, i, rho[i] + dtype(0.125))
        got = conservation(P, dev, nx, ny, g, ds, d_rho, d_E)
        want = exact(mass + float(ds) / 8, energy + float(ds) * float(E[i]) / 8)
        assert same_bits(got, want), (what, got, want)
        poke(P, dev, d_rho, i, rho[i])
    pitch = nx + 2 * g
    ghosts = {"below": S.flat_index(nx, g, -1, nx // 2), "above": S.flat_index(nx, g, ny, nx // 2),
              "left": S.flat_index(nx, g, ny // 2, -1), "right": S.flat_index(nx, g, ny // 2, nx),
              "left of the first cell": S.flat_index(nx, g, 0, -1), "right of the last cell": S.flat_index(nx, g, ny - 1, nx)}
    for what, i in ghosts.items():
        assert 0 <= i < pitch * (ny + 2 * g)
        poke(P, dev, d_rho, i, rho[i] + dtype(0.125))
        got = conservation(P, dev, nx, ny, g, ds, d_rho, d_E)
        assert same_bits(got, exact(mass, energy)), (what, got)
        poke(P, dev, d_rho, i, rho[i])
    assert same_bits(conservation(P, dev, nx, ny, g, ds, d_rho, d_E), exact(mass, energy))


@pytest.mark.parametrize("g", GHOSTS)
@pytest.mark.parametrize("shape", [(37, 29), (257, 64), (1000, 700)])
def test_conservation_sums_of_random_fp32_data(dev, L, shape, g):
    """Against the float64 sum of the float32 summands (rho, and the fp32 products rho·E), not against the fp32 oracle, whose
    serial sum is the less accurate of the two. Bound: any order of n - 1 fp32 additions is within (n - 1)·(eps32 / 2)·Σ|x| of
    the exact sum to first order (Higham, Accuracy and Stability of Numerical Algorithms, §4.2); n·eps32·Σ|x| is twice that and
    leaves room for the second-order terms and for the one rounding of the product with ds. The measured ratio is printed
    (pytest -s): a pairwise-style tree should stay orders of magnitude below 1."""
    nx, ny = shape
    P = Precision(L, np.float32)
    f = S.rand_fields(nx, ny, g, np.float32, seed=9)
    ds = np.float32(1.0 / (nx * ny))
    got = conservation(P, dev, nx, ny, g, ds, dev.from_host(f["rho"]), dev.from_host(f["E"]))
    rho, E = S.real_view(f["rho"], nx, ny, g), S.real_view(f["E"], nx, ny, g)
    n = nx * ny
    for name, value, x in (("mass", got[0], rho.astype(np.float64)), ("energy", got[1], (rho * E).astype(np.float64))):
        assert (rho * E).dtype == np.float32
        exact = float(np.sum(x)) * float(ds)
        bound = n * EPS32 * float(np.sum(np.abs(x))) * float(ds)
        ratio = abs(float(value) - exact) / bound
        print(f"conservation_vars_f32 {nx}x{ny} g={g} {name}: error / (n eps32 sum|x|) = {ratio:.3e}")
        assert ratio <= 1., (name, value, exact)
