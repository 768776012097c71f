/*
 * float_pair.h -- what the kernels that reduce float columns (agg_float.hip; group_lds.h's group_reduce) share: the double-double sum
 * of include/cryo_codec.h ("A float column's cell", "The reduction") and the fold of a column's state into its cell.
 *
 * The sum is part of the contract, byte for byte, so the helpers are written for the compiler to leave alone: IEEE binary64,
 * round to nearest, adds and subtracts only -- nothing a contraction could fuse --, every intermediate named, no fast-math flag
 * in the build.  Doubles keep their subnormals on this hardware whatever the single-precision mode is.
 */
#pragma once
#include "agg_cell.h"
#include "filter_walk.h"

namespace cryo {

constexpr uint32_t kFloatPosInf = 1u, kFloatNegInf = 2u, kFloatIsNan = 4u; /* a column's flags: some value is +Inf, -Inf, NaN */
constexpr uint64_t kFloatInf = 0x7FF0000000000000ull, kFloatMag = 0x7FFFFFFFFFFFFFFFull;

struct FloatPair { double hi, lo; };

/* x (+) y of the header: TwoSum of the high parts, the low parts added into its error, FastTwoSum.  Commutative by
 * construction: a + b and b + a round alike, and TwoSum's error term is symmetric in exact arithmetic and here, where both
 * orders compute the same s */
__device__ inline FloatPair float_pair_add(FloatPair x, FloatPair y)
{
    const double s = x.hi + y.hi;
    const double bb = s - x.hi;
    const double e1 = x.hi - (s - bb);
    const double e2 = y.hi - bb;
    const double e = e1 + e2;
    const double lows = x.lo + y.lo;
    const double t = e + lows;
    const double h = s + t;
    const double d = h - s;
    const double l = t - d;
    FloatPair r;
    r.hi = h;
    r.lo = l;
    return r;
}

/* a pair kept in the two 64-bit registers where an integer column keeps its sum's halves: hi's bits in a, lo's in b */
__device__ inline FloatPair float_pair_of(uint64_t a, uint64_t b)
{
    FloatPair x;
    x.hi = __longlong_as_double((long long)a);
    x.lo = __longlong_as_double((long long)b);
    return x;
}

__device__ inline void float_pair_to(FloatPair x, uint64_t &a, uint64_t &b)
{
    a = (uint64_t)__double_as_longlong(x.hi);
    b = (uint64_t)__double_as_longlong(x.lo);
}

/* the finite double of bits v joins the pair in (a, b) */
__device__ inline void float_pair_take(uint64_t v, uint64_t &a, uint64_t &b)
{
    float_pair_to(float_pair_add(float_pair_of(a, b), float_pair_of(v, 0u)), a, b); /* bits 0: +0.0 */
}

/* the flag of the double of bits b when it is not finite, else 0 */
__device__ inline uint32_t float_flag(uint64_t b)
{
    const uint64_t mag = b & kFloatMag;
    if (mag < kFloatInf) return 0u;
    return mag > kFloatInf ? kFloatIsNan : (b >> 63) ? kFloatNegInf : kFloatPosInf;
}

/* The cell of a float column as five words {n, min, max, sum, err}: n > 0 values whose mapped minimum and maximum are lo and hi,
 * flags what float_flag gave of them, (sum, err) the pair over the finite ones.  NaN or both infinities: (NaN, +0); one infinity:
 * (that, +0); a pair that left the double range -- it is not finite then, and stays so -- : (NaN, NaN) */
__device__ inline void float_cell(uint64_t out[5], uint64_t n, int64_t lo, int64_t hi, uint32_t flags, FloatPair sum)
{
    uint64_t s = (uint64_t)__double_as_longlong(sum.hi), e = (uint64_t)__double_as_longlong(sum.lo);
    const uint32_t inf = flags & (kFloatPosInf | kFloatNegInf);
    if ((flags & kFloatIsNan) != 0u || inf == (kFloatPosInf | kFloatNegInf)) { s = kFloatNan; e = 0u; }
    else if (inf != 0u) { s = inf == kFloatNegInf ? (kFloatInf | 1ull << 63) : kFloatInf; e = 0u; }
    else if ((s & kFloatMag) >= kFloatInf || (e & kFloatMag) >= kFloatInf) { s = kFloatNan; e = kFloatNan; }
    out[0] = n;
    out[1] = n ? float_unmap(lo) : 0u;
    out[2] = n ? float_unmap(hi) : 0u;
    out[3] = n ? s : 0u;
    out[4] = n ? e : 0u;
}

} // namespace cryo
