// exact_sum.hpp — the fixed-point addends of the decomposition-independent sums (profile.hip and mixing.hip through
// binned.hpp, analytic.hip, history.hip).
// A term t is rounded ONCE, on its own, to Q = round-half-even(t / 2^s); |Q| is cut into three limbs below
// 2^32, each negated when Q < 0 and each added to its own int64. Everything after the rounding is integer addition, so a
// sum is a function of its addends only, word for word.
#pragma once

#include "window.hpp"

namespace armon {
namespace exact {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

using win::bits_of;

// Q = round-half-even(t / 2^s) → a = |Q|; false when t is not finite or |Q| >= 2^95
__device__ __forceinline__ bool quantise(double t, int s, u128& a)
{
    const u64 b = bits_of(t), frac = b & ((1ull << 52) - 1);
    const int ef = (int)((b >> 52) & 0x7ff);
    a = 0;
    if (ef == 0x7ff) return false;
    const u64 m = ef ? (frac | (1ull << 52)) : frac;                // t = ±m 2^e
    if (m == 0) return true;
    const int64_t sh = (int64_t)(ef ? ef : 1) - 1075 - (int64_t)s;
    if (sh >= 0) {
        if (sh >= 95) return false;
        const int room = 95 - (int)sh;                              // m << sh < 2^95  <=>  m < 2^room
        if (room < 64 && (m >> room) != 0) return false;
        a = (u128)m << (int)sh;
    } else if (sh > -64) {
        const int r = (int)-sh;
        const u64 rem = m & ((1ull << r) - 1), half = 1ull << (r - 1);
        u64 q = m >> r;
        q += (rem > half) || (rem == half && (q & 1));
        a = q;                                                      // <= 2^52: never near the edge
    }                                                               // (m < 2^53: a shift by 64 or more rounds to 0)
    return true;
}

// the three limbs of a = |Q| into their sums, negated when the term is negative
__device__ __forceinline__ void add_limbs(long long sum[3], u128 a, bool neg)
{
    const long long l0 = (long long)((u64)a & 0xffffffffull), l1 = (long long)((u64)a >> 32), l2 = (long long)(u64)(a >> 64);
    sum[0] += neg ? -l0 : l0;
    sum[1] += neg ? -l1 : l1;
    sum[2] += neg ? -l2 : l2;
}

}  // namespace exact
}  // namespace armon
