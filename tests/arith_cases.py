"""Operands for the arithmetic primitives of the hot path, and the reference they are held to (test infrastructure: a plain
helper module, no fixtures).

The primitives: ``xct::Den<T>::quo / quo_t / twice`` and ``xct::sqrt_`` (csrc/physics.hpp, exact flavour) and
``fused::fast::rcp / rcp1 / sqrt_`` (csrc/sweep_stages.hpp, tuned flavour). Every generator is seeded and builds its operands
from integer significands and exponents, so that what a set claims (a tie, a zero remainder, a neighbour of a square) holds
exactly. The reference is numpy's IEEE ``/`` and ``sqrt`` in the operand's precision; ``exact_quotient`` / ``exact_root`` round the
exact value with integers alone, and tests/test_arith_cases_host.py shows the two agree on these very operands.

Sets are dicts name -> (a, b) or name -> x of arrays in the format's dtype; ``concat`` joins them for one launch.
"""
import math
import os
from fractions import Fraction

import numpy as np

SEED = int(os.environ.get("ARMON_RANDOM_SEED", "20261019"))


class Format:
    """An IEEE binary format: ``p`` significand bits, ``emin`` the exponent of the smallest normal number."""

    def __init__(self, name, p, emin, emax):
        self.name, self.p, self.emin, self.emax = name, p, emin, emax
        self.dtype = np.dtype(name)
        self.uint = np.dtype(np.uint64 if p == 53 else np.uint32)
        self.sub_exp = emin - (p - 1)                     # exponent of the smallest subnormal: one unit of the subnormal grid
        self.eps = 2.0 ** (1 - p)

    def __repr__(self):
        return self.name


F64 = Format("float64", 53, -1022, 1023)
F32 = Format("float32", 24, -126, 127)
FORMATS = {"float64": F64, "float32": F32}

# The range everything the solver divides lies in (csrc/physics.hpp): [1e-30, 1e30]; values built from a significand and a
# binary exponent take exponents within +-98 (2^-98 = 3.2e-30, 2^99 = 6.3e29).
E_RANGE = 98
LOG_RANGE = 30.0


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _signs(rng, n):
    return rng.choice(np.array([-1.0, 1.0]), n)


def _log_uniform(rng, n, decades, fmt):
    """Magnitudes log-uniform in [10^-decades, 10^decades], both signs, rounded to the format."""
    return (_signs(rng, n) * 10.0 ** rng.uniform(-decades, decades, n)).astype(fmt.dtype)


def _sig(rng, n, fmt, bits_=None):
    """``n`` random significands of ``bits_`` bits (default: the format's), top bit set, as Python-int-safe int64."""
    b = fmt.p if bits_ is None else bits_
    return rng.integers(1 << (b - 1), 1 << b, n, dtype=np.int64)


def _ldexp(sig, e, fmt):
    """sig * 2^e, exact: the caller keeps it representable."""
    out = np.ldexp(sig.astype(np.float64), e).astype(fmt.dtype)
    return out


def _exp_of_value(rng, n, fmt, sig_bits=None):
    """Exponents e such that sig * 2^e, sig of ``sig_bits`` bits, has a binary exponent within +-E_RANGE."""
    b = fmt.p if sig_bits is None else sig_bits
    return rng.integers(-E_RANGE, E_RANGE + 1, n) - (b - 1)


# ---- exact rounding with integers ----------------------------------------------------------------------------------------

def round_fraction(num, den, fmt):
    """The positive rational num / den rounded to nearest, ties to even, in ``fmt`` (subnormals, underflow to zero and
    overflow to infinity included), as a Python float."""
    assert num > 0 and den > 0
    e = num.bit_length() - den.bit_length() - fmt.p      # num / den / 2^e lies in (2^(p-1), 2^(p+1))
    if (num >> e if e >= 0 else num << -e) >= den << fmt.p:
        e += 1
    e = max(e, fmt.sub_exp)
    if e >= 0:
        den <<= e
    else:
        num <<= -e
    q, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and q & 1):
        q += 1
    if q.bit_length() + e - 1 > fmt.emax:
        return math.inf
    return math.ldexp(q, e)


def exact_quotient(a, b, fmt):
    """a / b correctly rounded in ``fmt`` from the exact rational value; a, b finite floats, b != 0."""
    a, b = float(a), float(b)
    sign = math.copysign(1.0, a) * math.copysign(1.0, b)
    if a == 0.0:
        return sign * 0.0
    fa, fb = Fraction(abs(a)), Fraction(abs(b))
    return sign * round_fraction(fa.numerator * fb.denominator, fa.denominator * fb.numerator, fmt)


def exact_root(x, fmt):
    """sqrt(x) correctly rounded in ``fmt`` with math.isqrt; x a finite float >= 0."""
    x = float(x)
    if x == 0.0:
        return x                                           # sqrt(-0) = -0
    m, e = math.frexp(x)
    X, e = int(math.ldexp(m, 53)), e - 53                  # x = X 2^e
    if e & 1:
        X, e = X << 1, e - 1
    shift = 2 * (fmt.p + 2)                                # the root to p + 2 bits and more: a sticky remainder decides the rest
    r = math.isqrt(X << shift)
    exact = r * r == X << shift
    h = (e - shift) // 2                                   # sqrt(x) = sqrt(X 2^shift) 2^h
    drop = r.bit_length() - fmt.p                          # > 0
    q, rem = r >> drop, r & ((1 << drop) - 1)
    half = 1 << (drop - 1)
    if rem > half or (rem == half and (not exact or q & 1)):
        q += 1
    return math.ldexp(q, h + drop)


def ulp_of(value, fmt):
    """One unit in the last place of ``fmt`` at the positive float (or Fraction) ``value`` (normal range)."""
    fr = Fraction(value)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    return Fraction(2) ** (e - (fmt.p - 1))


# ---- quotients ---------------------------------------------------------------------------------------------------------------

def near_tie(rng, fmt, delta, above):
    """Integer significands (A, B, k): B odd, both of p bits, with A 2^k = Q B + r, Q of exactly p bits, and r within ``delta``
    of B / 2 — on the side ``above`` or below: the quotient A / B lies |r - B/2| / B <= delta / B ~ delta 2^-p units of
    its last place from the midpoint of two neighbours.

    k = p for A < B (the quotient lies in [1/2, 1)), k = p - 1 for A > B (in (1, 2)): r is fixed first, A follows as
    r (2^k)^-1 mod B, taken as it is (k = p) or plus B (k = p - 1); redrawn while that is not a p-bit significand."""
    p = fmt.p
    while True:
        B = int(rng.integers(1 << (p - 1), 1 << p)) | 1
        r = (B + 1) // 2 + (delta - 1) if above else (B - 1) // 2 - (delta - 1)
        k = p - int(rng.integers(0, 2))
        A = r * pow(1 << k, -1, B) % B
        if k == p - 1:
            A += B
        if (1 << (p - 1)) <= A < (1 << p) and ((A < B) == (k == p)):
            return A, B, k


def tie_remainder(a, b, fmt):
    """For floats a, b: (r, B) with |a| 2^j = Q |b|_sig + r scaled so that Q has exactly p bits; |r - B/2| is the distance of the
    exact quotient from the midpoint of two neighbouring values of the format, in units of 1/B of the last place."""
    A, B = Fraction(abs(float(a))), Fraction(abs(float(b)))
    ma, mb = math.frexp(float(A))[0], math.frexp(float(B))[0]
    A, B = int(math.ldexp(ma, fmt.p)), int(math.ldexp(mb, fmt.p))
    k = fmt.p if A < B else fmt.p - 1
    return (A << k) % B, B


def quotient_sets(fmt, seed=SEED, n_random=200_000, n_special=8192, n_ties=65536):
    """The operand sets of a / b inside the documented range (quotients stay normal in fp64; in fp32 random operands of
    1e+-30 also overflow and underflow, which IEEE division defines and the compiler's fp32 expansion implements)."""
    rng = np.random.default_rng([seed, fmt.p, 1])
    p, dt = fmt.p, fmt.dtype
    sets = {}
    sets["random"] = (_log_uniform(rng, n_random, LOG_RANGE, fmt), _log_uniform(rng, n_random, LOG_RANGE, fmt))

    n = n_special
    a = _log_uniform(rng, n, LOG_RANGE, fmt)
    sets["power_of_two_denominator"] = (a, (_signs(rng, n) * np.ldexp(1.0, rng.integers(-E_RANGE, E_RANGE + 1, n))).astype(dt))
    ones = np.full(n, (1 << p) - 1, dtype=np.int64)
    sets["all_ones_denominator"] = (_log_uniform(rng, n, LOG_RANGE, fmt), _signs(rng, n).astype(dt) * _ldexp(ones, _exp_of_value(rng, n, fmt), fmt))
    plus = np.full(n, (1 << (p - 1)) + 1, dtype=np.int64)
    sets["one_plus_ulp_denominator"] = (_log_uniform(rng, n, LOG_RANGE, fmt), _signs(rng, n).astype(dt) * _ldexp(plus, _exp_of_value(rng, n, fmt), fmt))
    a = _log_uniform(rng, n, LOG_RANGE, fmt)
    sets["equal"] = (a, a.copy())
    # zero remainder: q and b of p // 2 bits each, a = q b exact
    h = p // 2
    q, b = _sig(rng, n, fmt, h), _sig(rng, n, fmt, h)
    eq, eb = rng.integers(-40, 41, n) - (h - 1), rng.integers(-40, 41, n) - (h - 1)
    sets["exact_quotient"] = (_signs(rng, n).astype(dt) * _ldexp(q * b, eq + eb, fmt), _signs(rng, n).astype(dt) * _ldexp(b, eb, fmt))
    # zero numerators: the four sign combinations in turn
    b = np.abs(_log_uniform(rng, n, LOG_RANGE, fmt))
    b[1::2] *= -1
    a = np.zeros(n, dtype=dt)
    a[(np.arange(n) // 2) % 2 == 1] = -0.0
    sets["zero_numerator"] = (a, b)

    A, B = np.empty(n_ties, dtype=np.int64), np.empty(n_ties, dtype=np.int64)
    for i in range(n_ties):
        A[i], B[i], _k = near_tie(rng, fmt, 1 + i % 8, bool((i // 8) % 2))
    sets["near_tie"] = (_signs(rng, n_ties).astype(dt) * _ldexp(A, _exp_of_value(rng, n_ties, fmt), fmt),
                        _signs(rng, n_ties).astype(dt) * _ldexp(B, _exp_of_value(rng, n_ties, fmt), fmt))
    for a, b in sets.values():
        assert a.dtype == dt and b.dtype == dt and a.shape == b.shape
    return sets


def tiny_quotient_sets(fmt, seed=SEED, n=100_000):
    """For quo_t: quotients from 2^12 above the smallest normal number (fp64: 2^-950 ... through the 2^-960 switch) down
    through the subnormal range to underflow to zero, denominators in [1e-30, 1e30], numerators down to the smallest subnormal."""
    rng = np.random.default_rng([seed, fmt.p, 2])
    dt = fmt.dtype
    b = _log_uniform(rng, n, LOG_RANGE, fmt)
    # the wanted exponent of the quotient: from emin + 72 down to four binades below the smallest subnormal
    t = rng.integers(fmt.sub_exp - 4, fmt.emin + 73, n)
    m = rng.uniform(1.0, 2.0, n)
    with np.errstate(under="ignore"):
        a = (_signs(rng, n) * np.ldexp(np.abs(b.astype(np.float64)) * m, t)).astype(dt)    # rounds into the subnormal grid
    keep = a != 0                                            # where |b| 2^t is below the grid there is no such numerator
    sets = {"graded": (a[keep], b[keep])}
    k = n // 8
    tiny = np.ldexp(1.0, fmt.sub_exp)
    sets["smallest_numerators"] = ((_signs(rng, k) * tiny * rng.integers(1, 5, k)).astype(dt), _log_uniform(rng, k, LOG_RANGE, fmt))
    # around the switch itself: |q| in [2^-962, 2^-958) (fp32: the same distance above its smallest normal number)
    b = _log_uniform(rng, k, 10.0, fmt)
    with np.errstate(under="ignore"):
        a = (_signs(rng, k) * np.ldexp(np.abs(b.astype(np.float64)) * rng.uniform(1.0, 2.0, k), rng.integers(fmt.emin + 60, fmt.emin + 64, k))).astype(dt)
    sets["at_the_switch"] = (a[a != 0], b[a != 0])
    return sets


def wide_quotient_set(fmt, seed=SEED, n=400_000, e_max=450):
    """Operand exponents out to 2^+-e_max with the quotient kept inside 2^+-e_max (fp64 only: the measured range)."""
    rng = np.random.default_rng([seed, fmt.p, 3])
    ea = rng.integers(-e_max, e_max + 1, n)
    eb = rng.integers(-e_max, e_max + 1, n)
    bad = np.abs(ea - eb) > e_max - 1
    eb[bad] = ea[bad] - rng.integers(-100, 101, int(bad.sum()))
    eb = np.clip(eb, -e_max, e_max)
    a = _signs(rng, n) * np.ldexp(rng.uniform(1.0, 2.0, n), ea)
    b = _signs(rng, n) * np.ldexp(rng.uniform(1.0, 2.0, n), eb)
    return a.astype(fmt.dtype), b.astype(fmt.dtype)


# ---- roots ---------------------------------------------------------------------------------------------------------------------

def root_sets(fmt, seed=SEED, n_random=200_000, n_special=16384):
    rng = np.random.default_rng([seed, fmt.p, 4])
    p, dt = fmt.p, fmt.dtype
    decades = 60.0 if fmt is F64 else 30.0               # fp32: 1e+-60 does not exist
    sets = {"random": np.abs(_log_uniform(rng, n_random, decades, fmt))}
    n = n_special
    h = p // 2
    q = _sig(rng, n, fmt, h)
    e = 2 * rng.integers(-45, 46, n) - 2 * (h - 1)
    sq = _ldexp(q * q, e, fmt)
    sets["perfect_square"] = sq
    sets["below_a_square"] = np.nextafter(sq, dt.type(0))
    sets["above_a_square"] = np.nextafter(sq, dt.type(np.inf))
    # the two neighbours of (Q + 1/2)^2: their roots lie just below and just above the midpoint of Q and Q + 1
    lo = np.empty(n, dtype=np.int64)
    ex = np.empty(n, dtype=np.int64)
    Q = _sig(rng, n, fmt)
    for i in range(n):
        v4 = (2 * int(Q[i]) + 1) ** 2                     # 4 (Q + 1/2)^2, never a p-bit number times a power of two
        s = v4.bit_length() - p
        lo[i], ex[i] = v4 >> s, s - 2
    e = 2 * rng.integers(-45, 46, n) - 2 * (p - 1)
    sets["below_a_midpoint"] = _ldexp(lo, ex + e, fmt)
    sets["above_a_midpoint"] = np.nextafter(sets["below_a_midpoint"], dt.type(np.inf))
    sets["zeros"] = np.array([0.0, -0.0] * 8, dtype=dt)
    return sets


def in_documented_range(x):
    """Mask of the operands with 1e-30 <= |x| <= 1e30."""
    ax = np.abs(x.astype(np.float64))
    return (ax >= 1e-30) & (ax <= 1e30)


# ---- reference -----------------------------------------------------------------------------------------------------------------

def ref_quotient(a, b):
    with np.errstate(all="ignore"):
        return a / b


def ref_root(x):
    with np.errstate(all="ignore"):
        return np.sqrt(x)


def concat(sets):
    """The sets joined for one launch: (arrays..., {name: slice})."""
    names = list(sets)
    first = sets[names[0]]
    cols = len(first) if isinstance(first, tuple) else 0
    where, at = {}, 0
    for k in names:
        n = len(sets[k][0]) if cols else len(sets[k])
        where[k] = slice(at, at + n)
        at += n
    if cols:
        return tuple(np.concatenate([sets[k][c] for k in names]) for c in range(cols)) + (where,)
    return np.concatenate([sets[k] for k in names]), where
