/*
 * agg_float.hip -- the scan aggregate's kernel for descriptors with a float key or a float aggregate column (CRYO_KEY_FLOAT4,
 * CRYO_KEY_FLOAT8; include/cryo_codec.h: "A float column's cell", "The reduction").  Every other descriptor runs agg.hip's
 * k_agg_block, which has no register to spare for this.
 *   k_aggf_block  the sweep is k_agg_block's (scan_sweep.h), with the walk's FLOATS parameter set and the truth table's verdict
 *                 path (the AND table from the host when the caller gave none).  Per aggregate column a uniform branch on the
 *                 column's type.  An integer
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
#include "scan_sweep.h"

namespace cryo {

/* the body of k_aggf_block and -- LIKE -- of k_aggl_block */
template <bool LIKE>
__device__ inline void aggf_block_body(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
                                       const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts,
                                       const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ cols, uint32_t ncols,
                                       uint32_t max_att, uint4 *__restrict__ blocks, AggCell *__restrict__ cells)
{
    uint32_t k, lane;
    sweep_wave(4u, k, lane);
    if (k >= cnt) return;
    uint32_t n_match = 0, n_bad = 0, flags = 0; /* flags: three bits per column */
    uint32_t cn[kAggMaxCols]; /* wave-uniform, as flags is: counted and gathered by ballot, they take no vector register */
    int64_t cmin[kAggMaxCols], cmax[kAggMaxCols];
    uint64_t ca[kAggMaxCols], cb[kAggMaxCols]; /* an integer column's sum_lo and sum_hi halves; a float column's hi and lo bits */
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) { cn[j] = 0; cmin[j] = INT64_MAX; cmax[j] = INT64_MIN; ca[j] = 0; cb[j] = 0; }
    const uint8_t *__restrict__ p;
    uint32_t n, upper;
    const uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        WalkCapture cap;
        const SweepItem it = sweep_turn<true, kAggMaxCols, true, false, true, false, LIKE>(p, B, n, upper, t0 + lane, atts, keys, nkeys,
                                                                                           max_att, cols, ncols, &cap);
        n_match += (uint32_t)__popcll(__ballot(it.match));
        n_bad += (uint32_t)__popcll(__ballot(it.bad));
#pragma unroll
        for (uint32_t j = 0; j < kAggMaxCols; j++) {
            if (j >= ncols) continue;                                  /* uniform */
            const uint32_t type = cols[j].type;                        /* uniform */
            const bool on = it.match && ((cap.has >> j) & 1u) != 0;    /* a NULL adds nothing */
            cn[j] += (uint32_t)__popcll(__ballot(on));
            if (type >= kKeyFloat4) {
                const uint64_t b = float_bits(cap.v[j], type == kKeyFloat4);
                const uint32_t f = on ? float_flag(b) : 0u;
                const uint32_t seen = (__ballot((f & kFloatPosInf) != 0u) ? kFloatPosInf : 0u) |
                                      (__ballot((f & kFloatNegInf) != 0u) ? kFloatNegInf : 0u) |
                                      (__ballot((f & kFloatIsNan) != 0u) ? kFloatIsNan : 0u);
                flags |= seen << (3u * j);
                if (!on) continue;
                cell_minmax(float_map(b), cmin[j], cmax[j]);
                if (f == 0u) float_pair_take(b, ca[j], cb[j]);
            } else if (on) {
                cell_minmax(cap.v[j], cmin[j], cmax[j]);
                cell_sum(cap.v[j], ca[j], cb[j]);
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) {
        if (j >= ncols) continue; /* uniform */
        const bool isf = cols[j].type >= kKeyFloat4; /* uniform */
#pragma unroll
        for (uint32_t d = 32; d >= 1u; d >>= 1) {
            cell_meet_minmax(d, cmin[j], cmax[j]);
            const uint64_t oa = __shfl_xor((unsigned long long)ca[j], d), ob = __shfl_xor((unsigned long long)cb[j], d);
            if (isf) float_pair_to(float_pair_add(float_pair_of(ca[j], cb[j]), float_pair_of(oa, ob)), ca[j], cb[j]);
            else {
                ca[j] += oa;
                cb[j] += ob;
            }
        }
    }
    if (lane == 0) {
        blocks[k] = make_uint4(status, n, n_match, n_bad);
#pragma unroll
        for (uint32_t j = 0; j < kAggMaxCols; j++) {
            if (j >= ncols) continue;
            AggCell c;
            if (cols[j].type >= kKeyFloat4) float_cell(c.w, cn[j], cmin[j], cmax[j], (flags >> (3u * j)) & 7u, float_pair_of(ca[j], cb[j]));
            else c = cell_int(cn[j], cmin[j], cmax[j], ca[j], cb[j]);
            cells[(uint64_t)k * ncols + j] = c;
        }
    }
}

#ifndef CRYO_LIKE_UNIT
/* the wave count asked for: without it the scheduler spends 86 registers on the same code (5 waves per SIMD); with it the kernel
 * needs 72 and runs 7, as k_agg_block<true> does, without scratch */
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(6)))
k_aggf_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
             const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
             const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint4 *__restrict__ blocks,
             AggCell *__restrict__ cells)
{
    aggf_block_body<false>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, cols, ncols, max_att, blocks, cells);
}

hipError_t launch_aggf(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a) { return agg_launch(k_aggf_block, true, c, d, a); }

#else /* CRYO_LIKE_UNIT */
/* k_aggf_block whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like), for every descriptor
 * with such a key, integer columns or float: a kernel of its own name, because the matcher's registers come on top of the
 * walk's and the four cells' -- no wave count is asked for here, the kernel takes the registers it needs.  Built from this
 * source compiled a second time with CRYO_LIKE_UNIT (agg_float_like.o) */
__global__ void __launch_bounds__(256)
k_aggl_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
             const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
             const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint4 *__restrict__ blocks,
             AggCell *__restrict__ cells)
{
    aggf_block_body<true>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, cols, ncols, max_att, blocks, cells);
}

hipError_t launch_aggl(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a) { return agg_launch(k_aggl_block, true, c, d, a); }
#endif

} // namespace cryo
