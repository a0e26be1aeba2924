"""The arithmetic primitives of the hot path, operand by operand, through tests/native/arith_probe.hip (one elementwise kernel
per primitive, built by armon.jl_amd/build.py with the product's flags into libarmon_arith_probe.so).

Exact flavour (csrc/physics.hpp): ``xct::Den<T>::quo``, ``quo_t``, ``twice().quo`` and ``xct::sqrt_`` give the bits of IEEE
division and square root — numpy's, which tests/test_arith_cases_host.py shows to be the correctly rounded values on these very
operands — on random operands of the documented range [1e-30, 1e30], on denominators at the edges of a binade, on zero
remainders, zero numerators of either sign, quotients within 1 ... 8 parts in 2^p of a tie, and for ``quo_t`` down through the
subnormal range to underflow. Tuned flavour (csrc/sweep_stages.hpp): the error of ``fused::fast::rcp``, ``rcp1``, ``sqrt_`` is
measured against the exact value and held to the figure their comments state. Run with -s for the measured figures."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import arith_cases as AC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "armon.jl_amd", "libarmon_arith_probe.so")
SUFFIX = {"float64": "f64", "float32": "f32"}


class Probe:
    def __init__(self):
        from armon_amd.device import HIPDevice
        assert os.path.exists(PROBE), f"{PROBE} is missing: python armon.jl_amd/build.py builds it"
        self.dev = HIPDevice(0)
        self.lib = C.CDLL(PROBE)

    def __call__(self, name, *arrays):
        """out = primitive(*arrays), elementwise on the device; host arrays in, host array out."""
        n, dtype = arrays[0].size, arrays[0].dtype
        fn = getattr(self.lib, "arith_probe_" + name)
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p] * (len(arrays) + 1) + [C.c_size_t]
        ins = [self.dev.from_host(a) for a in arrays]
        marker = np.full(n, np.nan, dtype=dtype)
        out = self.dev.from_host(marker)
        self.dev.wait()
        rc = fn(*[C.c_void_p(d.ptr) for d in ins], C.c_void_p(out.ptr), n)
        assert rc == 0, f"arith_probe_{name}: HIP status {rc}"
        res = out.to_host()
        for d in ins + [out]:
            d.free()
        return res


@pytest.fixture(scope="module")
def probe():
    p = Probe()
    yield p
    p.dev.wait()
    p.dev.close()


@pytest.fixture(scope="module")
def quotient_operands():
    """Per format: (a, b, {set: slice}) of tests/arith_cases.quotient_sets — generated once, shared, read-only."""
    out = {}
    for name, fmt in AC.FORMATS.items():
        a, b, where = AC.concat(AC.quotient_sets(fmt))
        a.setflags(write=False)
        b.setflags(write=False)
        out[name] = (a, b, where)
    return out


@pytest.fixture(scope="module")
def root_operands():
    out = {}
    for name, fmt in AC.FORMATS.items():
        x, where = AC.concat(AC.root_sets(fmt))
        x.setflags(write=False)
        out[name] = (x, where)
    return out


def assert_same_bits(got, want, where, what, operands):
    """Bit for bit, as integers (a NaN or a zero of the other sign is a difference); names the set and the first operands."""
    diff = AC.bits(got) != AC.bits(want)
    if not diff.any():
        return
    lines = []
    for name, sl in where.items():
        idx = np.flatnonzero(diff[sl])
        if idx.size:
            i = sl.start + idx[0]
            lines.append(f"{name}: {idx.size} of {sl.stop - sl.start}, first {tuple(float(o[i]).hex() for o in operands)} -> "
                         f"{float(got[i]).hex()} != {float(want[i]).hex()}")
    raise AssertionError(f"{what} differs from IEEE in {int(diff.sum())} of {diff.size} elements\n  " + "\n  ".join(lines))


# ---- exact flavour -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["quo", "quo_t", "twice_quo"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_exact_quotients_are_ieee_division(probe, quotient_operands, dtype, form):
    """Den(b).quo(a), .quo_t(a) = a / b and Den(b).twice().quo(a) = a / (2 b), the reference's bits on every set: random operands
    of [1e-30, 1e30], denominators that are powers of two, all ones, one plus an ulp, a == b, zero remainders, zero numerators of
    both signs against both signs of denominator (the sign of the zero is part of the bits), near ties."""
    a, b, where = quotient_operands[dtype]
    got = probe(f"{form}_{SUFFIX[dtype]}", a, b)
    want = AC.ref_quotient(a, b.dtype.type(2) * b if form == "twice_quo" else b)
    assert_same_bits(got, want, where, f"{form} ({dtype})", (a, b))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_quo_t_is_ieee_division_below_the_normal_range(probe, dtype):
    """quo_t where quo is documented to be off: quotients from 2^72 above the smallest normal number (fp64: either side of the
    2^-960 switch) through the subnormal range down to underflow to zero, numerators down to the smallest subnormal."""
    a, b, where = AC.concat(AC.tiny_quotient_sets(AC.FORMATS[dtype]))
    got = probe(f"quo_t_{SUFFIX[dtype]}", a, b)
    assert_same_bits(got, AC.ref_quotient(a, b), where, f"quo_t ({dtype})", (a, b))


def test_exact_root_is_ieee_square_root(probe, root_operands):
    """xct::sqrt_ on random x of [1e-60, 1e60], perfect squares and their neighbours, the neighbours of squares of midpoints
    (roots next to a tie), +0 and -0 (sqrt(-0) = -0)."""
    x, where = root_operands["float64"]
    assert_same_bits(probe("xct_sqrt_f64", x), AC.ref_root(x), where, "xct::sqrt_", (x,))


def test_exact_root_of_a_negative_number_or_a_nan_is_a_nan(probe):
    """What the invalid-time-step path relies on: a negative radicand (a negative pressure) reaches the host as a NaN."""
    x = np.array([-1.0, -1e-30, -1e30, -5e-324, -2.5, -np.inf, np.nan, -np.nan] * 8, dtype=np.float64)
    got = probe("xct_sqrt_f64", x)
    assert np.isnan(got).all(), got[:8]


def test_range_of_the_exact_quotient_measured(probe):
    """Not asserted: operand exponents out to 2^+-450 with the quotient inside 2^+-450. Prints the smallest and largest binary
    exponent (of a, b or the quotient) at which quo or quo_t differs from IEEE division, if any. The asserted range stays the
    documented one (test_exact_quotients_are_ieee_division)."""
    a, b = AC.wide_quotient_set(AC.F64)
    want = AC.ref_quotient(a, b)
    e = np.stack([np.frexp(v)[1] - 1 for v in (a, b, want)])
    print(f"\nwide quotients: {a.size} operand pairs, exponents {e[0].min()} ... {e[0].max()} (a), {e[1].min()} ... {e[1].max()} (b), "
          f"{e[2].min()} ... {e[2].max()} (a / b)")
    for form in ("quo_f64", "quo_t_f64", "twice_quo_f64"):
        got = probe(form, a, b)
        ref = AC.ref_quotient(a, 2. * b) if form == "twice_quo_f64" else want
        bad = np.flatnonzero(AC.bits(got) != AC.bits(ref))
        if bad.size == 0:
            print(f"  {form}: IEEE's bits on all of them")
        else:
            eb = e[:, bad]
            print(f"  {form}: {bad.size} differ; exponents of a {eb[0].min()} ... {eb[0].max()}, of b {eb[1].min()} ... {eb[1].max()}, "
                  f"of a / b {eb[2].min()} ... {eb[2].max()}; smallest |exponent| involved {np.abs(eb).max(axis=0).min()}")
        assert np.isfinite(got).all()


# ---- tuned flavour: measured against the exact value ----------------------------------------------------------------------------

def two_prod(x, y):
    """x y = p + e exactly (Dekker / Veltkamp), float64 arrays, no overflow for the magnitudes used here."""
    p = x * y
    s = 134217729.0
    cx = s * x
    xh = cx - (cx - x)
    xl = x - xh
    cy = s * y
    yh = cy - (cy - y)
    yl = y - yh
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


def worst_of(estimate, exact_of, keep=128):
    """The largest error: ``estimate`` (vectorised, good to many digits) picks the ``keep`` worst elements, ``exact_of(i)`` measures
    those with rational arithmetic; the estimate must agree with it there, so that no element left out can be worse."""
    order = np.argsort(estimate)[::-1][:keep]
    exact = np.array([float(exact_of(int(i))) for i in order])
    assert np.abs(exact - estimate[order]).max() <= 1e-6 * max(exact.max(), 1e-30), (exact[:4], estimate[order][:4])
    k = int(np.argmax(exact))
    return float(exact[k]), int(order[k])


def rcp_error(x, y, fmt, relative=False):
    """max |y - 1/x| in ulps of the exact 1/x (``relative``: as a fraction of it), and where."""
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    p, e = two_prod(xd, yd)
    rho = np.abs((p - 1.0) + e)                            # |x y - 1| = |y - 1/x| / |1/x|
    m = 2.0 * np.frexp(1.0 / np.abs(xd))[0]                # 1/|x| = m 2^E, m in [1, 2): one ulp is 2^(1 - p) / m of it
    scale = np.ones_like(m) if relative else m * 2.0 ** (fmt.p - 1)

    def exact_of(i):
        v = 1 / Fraction(float(x[i]))
        err = abs(Fraction(float(y[i])) - v)
        return err / abs(v) if relative else err / AC.ulp_of(abs(v), fmt)
    return worst_of(rho * scale, exact_of)


def sqrt_error(x, g, fmt):
    """max |g - sqrt(x)| in ulps of the exact root, and where. Exact side: the root to 2^-80 of its last place by math.isqrt."""
    xd, gd = x.astype(np.float64), g.astype(np.float64)
    p, e = two_prod(gd, gd)
    d = (p - xd) + e                                       # g^2 - x = (g - sqrt x)(g + sqrt x)
    root = np.sqrt(xd)
    ex = np.frexp(xd)[1] - 1                               # x in [2^ex, 2^(ex+1)): sqrt(x) in [2^floor(ex/2), 2 2^floor(ex/2))
    ulp = np.ldexp(1.0, ex // 2 - (fmt.p - 1))
    est = np.abs(d) / (gd + root) / ulp

    def exact_of(i):
        fx = Fraction(float(x[i]))                         # >= 1e-30: sqrt(x) 2^200 has more than 100 bits before the point
        r = Fraction(math.isqrt((fx.numerator << 400) // fx.denominator), 1 << 200)
        return abs(Fraction(float(g[i])) - r) / AC.ulp_of(r, fmt)
    return worst_of(est, exact_of)


RCP1_F64_BOUND = 2.0 ** -48 + 2.0 ** -52      # one Newton step from v_rcp_f64's 2^-24 (the figure csrc/sweep_stages.hpp states; the
                                              # ISA guide gives none): the squared error of the start plus one rounding of the FMA


def tuned_operands(quotient_operands, root_operands, dtype):
    """The denominators of the quotient sets and the radicands of the root sets, those within [1e-30, 1e30]."""
    _a, b, _w = quotient_operands[dtype]
    x, _w = root_operands[dtype]
    b, x = b[AC.in_documented_range(b)], x[AC.in_documented_range(x)]
    return b[: b.size // 2 * 2], x[: x.size // 2 * 2]     # an even count: the float2v forms take pairs


def test_tuned_double_primitives_keep_their_stated_accuracy(probe, quotient_operands, root_operands):
    """fast::rcp(double) <= 1 ulp (its last Newton step is one FMA rounding, <= 1/2 ulp, on an iterate whose own error, squared,
    is below 2^-90); fast::rcp1(double) <= eps_hw^2 + 2^-52 relative with eps_hw = 2^-24; fast::sqrt_(double) <= 2 ulp, the upper
    figure of its comment; sqrt_(0) == 0."""
    fmt = AC.F64
    b, x = tuned_operands(quotient_operands, root_operands, "float64")
    worst, i = rcp_error(b, probe("fast_rcp_f64", b), fmt)
    print(f"\nfast::rcp(double): worst {worst:.4f} ulp at x = {float(b[i]).hex()} ({b.size} operands)")
    assert worst <= 1.0
    rel, i = rcp_error(b, probe("fast_rcp1_f64", b), fmt, relative=True)
    print(f"fast::rcp1(double): worst relative error {rel:.4e} = 2^{math.log2(rel):.2f} at x = {float(b[i]).hex()} (bound {RCP1_F64_BOUND:.4e})")
    assert rel <= RCP1_F64_BOUND
    g = probe("fast_sqrt_f64", x)
    worst, i = sqrt_error(x[x != 0], g[x != 0], fmt)
    print(f"fast::sqrt_(double): worst {worst:.4f} ulp at x = {float(x[x != 0][i]).hex()} ({x.size} operands)")
    assert worst <= 2.0
    assert (probe("fast_sqrt_f64", np.array([0.0, -0.0] * 4)) == 0).all()


def test_tuned_float_primitives_keep_their_stated_accuracy(probe, quotient_operands, root_operands):
    """The float forms (v_rcp_f32, v_sqrt_f32) <= 1 ulp, as their comments and the ISA say; both components of the float2v forms
    equal the scalar form bit for bit; sqrt_(0) == 0."""
    fmt = AC.F32
    b, x = tuned_operands(quotient_operands, root_operands, "float32")
    scalar = {}
    for name in ("rcp", "rcp1"):
        scalar[name] = probe(f"fast_{name}_f32", b)
        worst, i = rcp_error(b, scalar[name], fmt)
        print(f"\nfast::{name}(float): worst {worst:.4f} ulp at x = {float(b[i]).hex()} ({b.size} operands)")
        assert worst <= 1.0, name
    scalar["sqrt"] = probe("fast_sqrt_f32", x)
    worst, i = sqrt_error(x[x != 0], scalar["sqrt"][x != 0], fmt)
    print(f"fast::sqrt_(float): worst {worst:.4f} ulp at x = {float(x[x != 0][i]).hex()} ({x.size} operands)")
    assert worst <= 1.0
    zeros = np.array([0.0, -0.0] * 4, dtype=np.float32)
    assert (probe("fast_sqrt_f32", zeros) == 0).all() and (probe("fast_sqrt_f32x2", zeros) == 0).all()
    for name, operand in (("rcp", b), ("rcp1", b), ("sqrt", x)):
        pair = probe(f"fast_{name}_f32x2", operand)
        diff = np.flatnonzero(AC.bits(pair) != AC.bits(scalar[name]))
        assert diff.size == 0, (f"float2v {name}: {diff.size} elements differ from the scalar form, first at {diff[0]} "
                                f"(component {diff[0] % 2}): {pair[diff[0]]!r} != {scalar[name][diff[0]]!r}")
