/*
 * agg_float.hip -- the scan aggregate's kernel for descriptors with a float key or a float aggregate column (CRYO_KEY_FLOAT4,
 * CRYO_KEY_FLOAT8; include/cryo_codec.h: "A float column's cell", "The reduction").  Every other descriptor runs agg.hip's
 * k_agg_block, which has no register to spare for this.
 *   k_aggf_block  the sweep is k_agg_block's: one wave per block, four blocks per workgroup, a lane takes one item per turn, the
 *                 walk of filter_walk.h with its FLOATS parameter set and the truth table's verdict path (the AND table from the
 *                 host when the caller gave none).  Per aggregate column a uniform branch on the column's type.  An integer
 *                 column reduces as in k_agg_block and its cell is byte for byte that kernel's.  A float column keeps the count,
 *                 the minimum and the maximum of the values mapped onto signed integers (float_map) -- so the compares and the
 *                 butterfly are the integer column's --, the double-double pair (hi, lo) in the two registers where the integer
 *                 column keeps its sum's halves, and three flag bits: some value is +Inf, -Inf, NaN.  Those values never enter
 *                 the sum.  A lane's pair is leaf S_lane of the contract: it takes its matches in ascending position.  The
 *                 butterfly applies the pair sum for d = 32 .. 1, every lane with its partner at once; lane 0 folds the flags
 *                 and writes the cell.
 * Every device write is a vector store in plain C++.  No LDS, no scratch, no atomics.
 */
#include "kernels.h"
#include "float_pair.h"

namespace cryo {

struct AggWords { uint64_t w[5]; }; /* cryo_agg_cell and cryo_agg_cell_f alike */
static_assert(sizeof(AggWords) == 40, "the cell's layout is the header's");

/* the wave count asked for: without it the scheduler spends 86 registers on the same code (5 waves per SIMD); with it the kernel
 * needs 72 and runs 7, as k_agg_block<true> does, without scratch */
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
k_aggf_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
             const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
             const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint4 *__restrict__ blocks,
             AggWords *__restrict__ cells)
{
    const uint32_t k = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (k >= cnt) return;
    uint32_t status = 0, n_items = 0, n_match = 0, n_bad = 0, flags = 0; /* flags: three bits per column */
    uint32_t cn[kAggMaxCols]; /* wave-uniform, as flags is: counted and gathered by ballot, they take no vector register */
    int64_t cmin[kAggMaxCols], cmax[kAggMaxCols];
    uint64_t ca[kAggMaxCols], cb[kAggMaxCols]; /* an integer column's sum_lo and sum_hi halves; a float column's hi and lo bits */
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) { cn[j] = 0; cmin[j] = INT64_MAX; cmax[j] = INT64_MIN; ca[j] = 0; cb[j] = 0; }
    if (dec_status[k] != 0) status = kFilterStream;
    else {
        const uint8_t *p = dec + (uint64_t)k * dec_stride;
        const uint2 hdr = *reinterpret_cast<const uint2 *>(p);
        uint32_t n, upper;
        if (!heap_header(hdr, B, n, upper))
            status = kFilterHeader;
        else {
            n_items = n;
            for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
                const uint32_t i = t0 + lane;
                const bool valid = i < n;
                uint32_t verdict = kFilterNoMatch, len = 0, src = 0;
                if (valid) {
                    const uint2 it = *reinterpret_cast<const uint2 *>(p + 8u + 8u * i); /* 8 + 8 n = lower <= B */
                    if (!heap_item(it, upper, B, src, len)) verdict = kFilterItem;
                }
                const bool live = valid && verdict != kFilterItem;
                WalkCapture cap;
                cap.has = 0;
#pragma unroll
                for (uint32_t j = 0; j < kAggMaxCols; j++) cap.v[j] = 0;
                const uint32_t walked = walk_tuple<true, kAggMaxCols, true, false, true>(p + src, len, live, atts, keys, nkeys, max_att,
                                                                                         cols, ncols, &cap, WalkKeys<true>());
                if (live) verdict = walked;
                const bool match = verdict == 0u, bad = verdict == kFilterItem || verdict == kFilterTuple || verdict == kFilterUndecided;
                n_match += (uint32_t)__popcll(__ballot(match));
                n_bad += (uint32_t)__popcll(__ballot(bad));
#pragma unroll
                for (uint32_t j = 0; j < kAggMaxCols; j++) {
                    if (j >= ncols) continue;                                  /* uniform */
                    const uint32_t type = cols[j].type;                        /* uniform */
                    const bool on = match && ((cap.has >> j) & 1u) != 0;       /* a NULL adds nothing */
                    cn[j] += (uint32_t)__popcll(__ballot(on));
                    if (type >= kKeyFloat4) {
                        const uint64_t b = float_bits(cap.v[j], type == kKeyFloat4);
                        const uint32_t f = on ? float_flag(b) : 0u;
                        const uint32_t seen = (__ballot((f & kFloatPosInf) != 0u) ? kFloatPosInf : 0u) |
                                              (__ballot((f & kFloatNegInf) != 0u) ? kFloatNegInf : 0u) |
                                              (__ballot((f & kFloatIsNan) != 0u) ? kFloatIsNan : 0u);
                        flags |= seen << (3u * j);
                        if (!on) continue;
                        const int64_t v = float_map(b);
                        cmin[j] = v < cmin[j] ? v : cmin[j];
                        cmax[j] = v > cmax[j] ? v : cmax[j];
                        if (f == 0u) {
                            FloatPair x, y;
                            x.hi = __longlong_as_double((long long)ca[j]);
                            x.lo = __longlong_as_double((long long)cb[j]);
                            y.hi = __longlong_as_double((long long)b);
                            y.lo = 0.0;
                            x = float_pair_add(x, y);
                            ca[j] = (uint64_t)__double_as_longlong(x.hi);
                            cb[j] = (uint64_t)__double_as_longlong(x.lo);
                        }
                    } else {
                        if (!on) continue;
                        const int64_t v = cap.v[j];
                        cmin[j] = v < cmin[j] ? v : cmin[j];
                        cmax[j] = v > cmax[j] ? v : cmax[j];
                        ca[j] += (uint64_t)v & 0xFFFFFFFFull;
                        cb[j] += (uint64_t)(v >> 32); /* arithmetic: v = (v >> 32) * 2^32 + (v & 0xFFFFFFFF); wraps as the signed sum does */
                    }
                }
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) {
        if (j >= ncols) continue; /* uniform */
        const bool isf = cols[j].type >= kKeyFloat4; /* uniform */
#pragma unroll
        for (uint32_t d = 32; d >= 1u; d >>= 1) {
            const int64_t omin = __shfl_xor((long long)cmin[j], d), omax = __shfl_xor((long long)cmax[j], d);
            cmin[j] = omin < cmin[j] ? omin : cmin[j];
            cmax[j] = omax > cmax[j] ? omax : cmax[j];
            const uint64_t oa = __shfl_xor((unsigned long long)ca[j], d), ob = __shfl_xor((unsigned long long)cb[j], d);
            if (isf) {
                FloatPair x, y;
                x.hi = __longlong_as_double((long long)ca[j]);
                x.lo = __longlong_as_double((long long)cb[j]);
                y.hi = __longlong_as_double((long long)oa);
                y.lo = __longlong_as_double((long long)ob);
                x = float_pair_add(x, y);
                ca[j] = (uint64_t)__double_as_longlong(x.hi);
                cb[j] = (uint64_t)__double_as_longlong(x.lo);
            } else {
                ca[j] += oa;
                cb[j] += ob;
            }
        }
    }
    if (lane == 0) {
        blocks[k] = make_uint4(status, n_items, n_match, n_bad);
#pragma unroll
        for (uint32_t j = 0; j < kAggMaxCols; j++) {
            if (j >= ncols) continue;
            AggWords c;
            if (cols[j].type >= kKeyFloat4) {
                FloatPair x;
                x.hi = __longlong_as_double((long long)ca[j]);
                x.lo = __longlong_as_double((long long)cb[j]);
                float_cell(c.w, cn[j], cmin[j], cmax[j], (flags >> (3u * j)) & 7u, x);
            } else {
                /* sum = chi * 2^32 + clo as a 128-bit two's-complement number, as in agg.hip */
                const int64_t chi = (int64_t)cb[j];
                const uint64_t low = (uint64_t)chi << 32;
                c.w[0] = cn[j];
                c.w[1] = cn[j] ? (uint64_t)cmin[j] : 0u;
                c.w[2] = cn[j] ? (uint64_t)cmax[j] : 0u;
                c.w[3] = low + ca[j];
                c.w[4] = (uint64_t)((chi >> 32) + (c.w[3] < low ? 1 : 0));
            }
            cells[(uint64_t)k * ncols + j] = c;
        }
    }
}

hipError_t launch_aggf(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                       const int32_t *d_dec_status, const void *d_atts, const void *d_keys, uint32_t nkeys, const void *d_cols,
                       uint32_t ncols, uint32_t max_att, uint32_t truth, uint4 *d_blocks, void *d_cells)
{
    /* the arguments are launch_agg's, which checked them; the one verdict path needs a table */
    if (truth == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_aggf_block, dim3((cnt + 3u) / 4u), dim3(256), 0, s, d_dec, dec_stride, block_size, cnt, d_dec_status,
                       (const FilterAtt *)d_atts, (const FilterKey *)d_keys, nkeys | truth << 16, (const AggCol *)d_cols, ncols, max_att,
                       d_blocks, (AggWords *)d_cells);
    return hipGetLastError();
}

} // namespace cryo
