/*
 * agg_cell.h -- the 40-byte cell of an aggregate column and an integer column's way into it, shared by the kernels that reduce
 * columns (agg.hip, agg_float.hip and, through group_lds.h's group_reduce, the grouped scan's block kernels in group.hip,
 * group_float.hip, group_bucket.hip and group_text.hip; include/cryo_codec.h: "aggregating a scan").  A column's running
 * state is its count n of non-NULL values, their minimum and maximum, and their sum in two 64-bit halves: lo the low 32 bits of
 * every value summed unsigned, hi the high 32 bits summed signed (kept in an unsigned register: it wraps as the signed sum does).
 * A block has at most 290 values, so neither half overflows.  A float column keeps count, minimum and maximum the same way, over
 * mapped values, and a pair where the halves are (float_pair.h).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cryo_codec.h"

namespace cryo {

/* cryo_agg_cell {n, min, max, sum_lo, sum_hi} and cryo_agg_cell_f {n, min, max, sum, err} alike */
struct AggCell { uint64_t w[5]; };
static_assert(sizeof(AggCell) == 40 && sizeof(cryo_agg_cell) == 40 && sizeof(cryo_agg_cell_f) == 40, "the cell's layout is the header's");

__device__ inline void cell_minmax(int64_t v, int64_t &min, int64_t &max)
{
    min = v < min ? v : min;
    max = v > max ? v : max;
}

__device__ inline void cell_sum(int64_t v, uint64_t &lo, uint64_t &hi)
{
    lo += (uint64_t)v & 0xFFFFFFFFull;
    hi += (uint64_t)(v >> 32); /* arithmetic: v = (v >> 32) * 2^32 + (v & 0xFFFFFFFF) */
}

/* one value joins an integer column's state */
__device__ inline void cell_add(int64_t v, uint32_t &n, int64_t &min, int64_t &max, uint64_t &lo, uint64_t &hi)
{
    n++;
    cell_minmax(v, min, max);
    cell_sum(v, lo, hi);
}

/* one step of the butterfly: the minimum and maximum of the lane d away join this lane's */
__device__ inline void cell_meet_minmax(uint32_t d, int64_t &min, int64_t &max)
{
    const int64_t omin = __shfl_xor((long long)min, d), omax = __shfl_xor((long long)max, d);
    min = omin < min ? omin : min;
    max = omax > max ? omax : max;
}

/* the same for an integer column's whole state */
__device__ inline void cell_meet(uint32_t d, uint32_t &n, int64_t &min, int64_t &max, uint64_t &lo, uint64_t &hi)
{
    n += __shfl_xor(n, d);
    cell_meet_minmax(d, min, max);
    lo += __shfl_xor((unsigned long long)lo, d);
    hi += __shfl_xor((unsigned long long)hi, d);
}

/* The finished cell of an integer column; a column without a value reports 0 for min and max.  sum = hi * 2^32 + lo as a 128-bit
 * two's-complement number: hi * 2^32 has the low word hi << 32 and the high word hi >> 32 (arithmetic); adding the unsigned lo
 * carries at most one into the high word */
__device__ inline AggCell cell_int(uint64_t n, int64_t min, int64_t max, uint64_t lo, uint64_t hi)
{
    const uint64_t low = hi << 32;
    AggCell c;
    c.w[0] = n;
    c.w[1] = n ? (uint64_t)min : 0u;
    c.w[2] = n ? (uint64_t)max : 0u;
    c.w[3] = low + lo;
    c.w[4] = (uint64_t)(((int64_t)hi >> 32) + (c.w[3] < low ? 1 : 0));
    return c;
}

} // namespace cryo
