"""tests/arith_cases.py on the CPU: the operand sets are what they claim to be, and the reference the GPU tests compare with
(numpy's IEEE / and sqrt) is the correctly rounded value on these very operands — shown with integer arithmetic alone."""
import math
from fractions import Fraction

import numpy as np
import pytest

import arith_cases as AC

FORMATS = [AC.F64, AC.F32]
N_RANDOM = 10_000                                          # of the random operands; every special case is checked


@pytest.fixture(scope="module", params=FORMATS, ids=repr)
def quotients(request):
    fmt = request.param
    return fmt, AC.quotient_sets(fmt), AC.tiny_quotient_sets(fmt, n=20_000)


@pytest.fixture(scope="module", params=FORMATS, ids=repr)
def roots(request):
    return request.param, AC.root_sets(request.param)


def same_bits(x, y, fmt):
    return np.array([x], dtype=fmt.dtype).view(fmt.uint)[0] == np.array([y], dtype=fmt.dtype).view(fmt.uint)[0]


def test_rounding_of_a_fraction_by_hand():
    """round_fraction on values whose rounding is known: ties to even, the subnormal grid, underflow, overflow."""
    f = AC.F64
    assert AC.round_fraction(1, 3, f) == 1 / 3 and AC.round_fraction(2, 3, f) == 2 / 3
    assert AC.round_fraction((1 << 53) + 1, 1, f) == float(1 << 53)               # tie, to even (down)
    assert AC.round_fraction((1 << 53) + 3, 1, f) == float((1 << 53) + 4)         # tie, to even (up)
    assert AC.round_fraction(3, 1 << 1075, f) == 2 * 5e-324                       # 1.5 units of the subnormal grid: tie to even
    assert AC.round_fraction(1, 1 << 1075, f) == 0.0 and AC.round_fraction(3, 1 << 1076, f) == 5e-324
    assert AC.round_fraction(1 << 1024, 1, f) == math.inf
    assert AC.round_fraction((1 << 1024) - (1 << 970), 1, f) == math.inf          # halfway to 2^1024 rounds to even: overflow
    g = AC.F32
    assert AC.round_fraction(1, 3, g) == float(np.float32(1) / np.float32(3))
    assert AC.round_fraction(1, 1 << 149, g) == float(np.float32(1.4e-45)) and AC.round_fraction(1, 1 << 150, g) == 0.0
    assert AC.exact_root(2.0, f) == math.sqrt(2.0) and AC.exact_root(4.0, g) == 2.0 and AC.exact_root(5e-324, f) == math.sqrt(5e-324)
    assert math.copysign(1.0, AC.exact_root(-0.0, f)) == -1.0 and math.copysign(1.0, AC.exact_quotient(-0.0, 3.0, f)) == -1.0
    assert AC.ulp_of(1.0, f) == Fraction(1, 1 << 52) and AC.ulp_of(1.5, g) == Fraction(1, 1 << 23) and AC.ulp_of(0.75, f) == Fraction(1, 1 << 53)


def test_the_quotient_reference_is_correctly_rounded_on_these_operands(quotients):
    fmt, sets, tiny = quotients
    checked = 0
    for group in (sets, tiny):
        for name, (a, b) in group.items():
            q = AC.ref_quotient(a, b)
            idx = range(len(a)) if name != "random" else range(N_RANDOM)
            for i in idx:
                want = AC.exact_quotient(a[i], b[i], fmt)
                assert same_bits(q[i], want, fmt), (fmt, name, i, a[i], b[i], q[i], want)
            checked += len(idx)
    assert checked > 100_000


def test_the_root_reference_is_correctly_rounded_on_these_operands(roots):
    fmt, sets = roots
    for name, x in sets.items():
        r = AC.ref_root(x)
        for i in (range(len(x)) if name != "random" else range(N_RANDOM)):
            want = AC.exact_root(x[i], fmt)
            assert same_bits(r[i], want, fmt), (fmt, name, i, x[i], r[i], want)


def test_near_ties_are_near_ties(quotients):
    """The exact remainder lies within delta = 1 ... 8 (each of them, on either side) of half the denominator: the quotient is
    within delta / B of the midpoint of two neighbouring values, and never on it."""
    fmt, sets, _tiny = quotients
    a, b = sets["near_tie"]
    seen = set()
    for i in range(len(a)):
        r, B = AC.tie_remainder(a[i], b[i], fmt)
        d = Fraction(r) - Fraction(B, 2)
        assert B & 1 and 0 < abs(d) <= 8, (i, a[i], b[i], r, B)
        seen.add((int(abs(d) + Fraction(1, 2)), d > 0))
        q = Fraction(float(a[i])) / Fraction(float(b[i]))
        off = abs(q) / AC.ulp_of(abs(q), fmt) % 1 - Fraction(1, 2)                 # in units of the last place, from the midpoint
        assert abs(off) == abs(d) / B, (i, off, d, B)
    assert seen == {(k, s) for k in range(1, 9) for s in (False, True)}
    assert AC.in_documented_range(a).all() and AC.in_documented_range(b).all()


def test_the_sets_hold_what_they_say(quotients):
    fmt, sets, tiny = quotients
    p = fmt.p
    for name in ("random", "power_of_two_denominator", "all_ones_denominator", "one_plus_ulp_denominator", "equal", "near_tie"):
        a, b = sets[name]
        assert (a < 0).any() and (a > 0).any() and (b < 0).any() and (b > 0).any(), name
        assert AC.in_documented_range(b).all() and (name == "exact_quotient" or AC.in_documented_range(a).all()), name
    m = np.frexp(sets["power_of_two_denominator"][1].astype(np.float64))[0]
    assert (np.abs(m) == 0.5).all()
    m = np.frexp(sets["all_ones_denominator"][1].astype(np.float64))[0]
    assert (np.abs(m) == 1.0 - 2.0 ** -p).all()
    m = np.frexp(sets["one_plus_ulp_denominator"][1].astype(np.float64))[0]
    assert (np.abs(m) == 0.5 + 2.0 ** -p).all()
    a, b = sets["equal"]
    assert np.array_equal(AC.bits(a), AC.bits(b))
    a, b = sets["exact_quotient"]
    for i in range(0, len(a), 7):
        q = Fraction(float(a[i])) / Fraction(float(b[i]))
        assert Fraction(float(AC.ref_quotient(a, b)[i])) == q, (i, a[i], b[i])     # zero remainder
    a, b = sets["zero_numerator"]
    assert (a == 0).all()
    assert {(bool(s), bool(t)) for s, t in zip(np.signbit(a), np.signbit(b))} == {(False, False), (False, True), (True, False), (True, True)}
    # quo_t's range: quotients on both sides of the 2^-960 switch (fp64), subnormal ones, and ones that underflow to zero
    a, b = tiny["graded"]
    q = np.abs(AC.ref_quotient(a, b).astype(np.float64))
    small = float(np.finfo(fmt.dtype).tiny)
    assert (q == 0).any() and ((q > 0) & (q < small)).sum() > 1000 and (q >= small).sum() > 1000
    if fmt is AC.F64:
        assert ((q < 2.0 ** -960) & (q >= small)).sum() > 100 and (q > 2.0 ** -960).sum() > 100 and q.max() >= 2.0 ** -951
        s = np.abs(AC.ref_quotient(*tiny["at_the_switch"]))
        assert (s < 2.0 ** -960).sum() > 100 and (s >= 2.0 ** -960).sum() > 100
    a, b = tiny["smallest_numerators"]
    assert np.abs(a).min() == np.ldexp(1.0, fmt.sub_exp) and AC.in_documented_range(b).all()


def test_the_root_sets_hold_what_they_say(roots):
    fmt, sets = roots
    sq = sets["perfect_square"]
    r = AC.ref_root(sq)
    assert np.array_equal(r.astype(np.float64) ** 2, sq.astype(np.float64))        # roots of p/2 bits: their squares are exact
    assert (sets["below_a_square"] < sq).all() and (sets["above_a_square"] > sq).all()
    lo, hi = sets["below_a_midpoint"], sets["above_a_midpoint"]
    rl, rh = AC.ref_root(lo), AC.ref_root(hi)
    assert np.array_equal(np.nextafter(rl, fmt.dtype.type(np.inf)), rh)            # the midpoint of two neighbours lies between
    for i in range(0, len(lo), 5):
        mid = (Fraction(float(rl[i])) + Fraction(float(rh[i]))) / 2
        assert Fraction(float(lo[i])) < mid * mid < Fraction(float(hi[i])), i
    z = sets["zeros"]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    x = sets["random"].astype(np.float64)
    decades = 60 if fmt is AC.F64 else 30
    assert x.min() < 10.0 ** (5 - decades) and x.max() > 10.0 ** (decades - 5)


def test_the_wide_set_keeps_the_quotient_inside():
    a, b = AC.wide_quotient_set(AC.F64)
    for v in (a, b, AC.ref_quotient(a, b)):
        e = np.frexp(v)[1] - 1
        assert e.min() >= -451 and e.max() <= 451
    assert (np.frexp(a)[1] > 440).any() and (np.frexp(b)[1] < -440).any()


def test_the_sets_are_seeded():
    a1, b1 = AC.quotient_sets(AC.F32, n_random=100, n_special=16, n_ties=16)["near_tie"]
    a2, b2 = AC.quotient_sets(AC.F32, n_random=100, n_special=16, n_ties=16)["near_tie"]
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
    a3, _ = AC.quotient_sets(AC.F32, seed=AC.SEED + 1, n_random=100, n_special=16, n_ties=16)["near_tie"]
    assert not np.array_equal(a1, a3)
