/*
 * agg.hip -- the device side of the scan aggregate (cryo_codec_agg_batch / _blocks, include/cryo_codec.h: the rules).
 *
 * The host (cryo_codec.cpp, agg_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); this kernel looks into every heap tuple of the decoded chunk as the scan filter does, and instead of packing the
 * tuples that pass the keys it reduces up to four of their integer columns, so that a row and a few cells per block leave the
 * device:
 *   k_agg_block   one wave per block, four blocks per workgroup, as k_filter_match.  A block the decoders rejected gets STREAM
 *                 without a load, a bad header (heap_header, heap_block.h) HEADER.  Otherwise a lane takes one item per turn (290 items: five turns): the
 *                 ITEM rule (heap_item), then the walk of filter_walk.h over the columns 1 .. max(highest key column, highest aggregate
 *                 column), which tests the keys and notes the aggregate columns' values as it passes them.  Descriptor, keys and
 *                 aggregate columns are read at addresses that depend on loop counters only (uniform loads); no load leaves
 *                 [t, t + len).  A descriptor with a byte-string key runs k_agg_block<true>, whose walk compares those too and
 *                 counts an undecided tuple in n_bad; every other descriptor runs k_agg_block<false>.  There is no OVERLAP verdict and nothing to place, so one sweep suffices.  A lane keeps, per
 *                 aggregate column, the count of non-NULL matches, their min and max, and their sum in two 64-bit halves: the low
 *                 32 bits of every value summed unsigned, the high 32 bits summed signed -- at most 290 values, so neither half
 *                 overflows.  After the sweep a butterfly (__shfl_xor) reduces the five words per column across the wave; lane 0
 *                 joins the halves into the 128-bit sum and writes the block's row and its cells straight to the call's output.
 * A descriptor with a float key or a float aggregate column runs agg_float.hip's k_aggf_block instead (launch_agg's `floats`).
 * Every device write is a vector store in plain C++.  No LDS, no scratch, no atomics; no running totals, no second kernel.
 */
#include "kernels.h"
#include "filter_walk.h"

namespace cryo {

struct AggCell { uint64_t n; int64_t min, max; uint64_t sum_lo; int64_t sum_hi; }; /* cryo_agg_cell */
static_assert(sizeof(AggCell) == 40, "the cell's layout is the header's");

template <bool BYTES>
__global__ void __launch_bounds__(256)
k_agg_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
            const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
            const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint4 *__restrict__ blocks,
            AggCell *__restrict__ cells)
{
    /* the wave's number through readfirstlane, as in k_filter_match: the block, its header and the trip counts are the same in
     * all 64 lanes and stay, with the descriptor reads, in scalar registers */
    const uint32_t k = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    if (k >= cnt) return;
    uint32_t status = 0, n_items = 0, n_match = 0, n_bad = 0;
    uint32_t cn[kAggMaxCols];
    int64_t cmin[kAggMaxCols], cmax[kAggMaxCols], chi[kAggMaxCols];
    uint64_t clo[kAggMaxCols];
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) { cn[j] = 0; cmin[j] = INT64_MAX; cmax[j] = INT64_MIN; clo[j] = 0; chi[j] = 0; }
    if (dec_status[k] != 0) status = kFilterStream; /* the decoders rejected the stream: nothing decoded to look at */
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
                const uint32_t walked = walk_tuple<true>(p + src, len, live, atts, keys, nkeys, max_att, cols, ncols, &cap, WalkKeys<BYTES>());
                if (live) verdict = walked;
                const bool match = verdict == 0u,
                           bad = verdict == kFilterItem || verdict == kFilterTuple || (BYTES && verdict == kFilterUndecided);
                n_match += (uint32_t)__popcll(__ballot(match));
                n_bad += (uint32_t)__popcll(__ballot(bad));
#pragma unroll
                for (uint32_t j = 0; j < kAggMaxCols; j++) {
                    if (!match || ((cap.has >> j) & 1u) == 0) continue; /* a NULL adds nothing */
                    const int64_t v = cap.v[j];
                    cn[j]++;
                    cmin[j] = v < cmin[j] ? v : cmin[j];
                    cmax[j] = v > cmax[j] ? v : cmax[j];
                    clo[j] += (uint64_t)v & 0xFFFFFFFFull;
                    chi[j] += v >> 32; /* arithmetic: v = (v >> 32) * 2^32 + (v & 0xFFFFFFFF) */
                }
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) {
        if (j >= ncols) continue; /* uniform */
#pragma unroll
        for (uint32_t d = 32; d >= 1u; d >>= 1) {
            cn[j] += __shfl_xor(cn[j], d);
            const int64_t omin = __shfl_xor((long long)cmin[j], d), omax = __shfl_xor((long long)cmax[j], d);
            cmin[j] = omin < cmin[j] ? omin : cmin[j];
            cmax[j] = omax > cmax[j] ? omax : cmax[j];
            clo[j] += __shfl_xor((unsigned long long)clo[j], d);
            chi[j] += __shfl_xor((long long)chi[j], d);
        }
    }
    if (lane == 0) {
        blocks[k] = make_uint4(status, n_items, n_match, n_bad);
#pragma unroll
        for (uint32_t j = 0; j < kAggMaxCols; j++) {
            if (j >= ncols) continue;
            AggCell c;
            /* sum = chi * 2^32 + clo as a 128-bit two's-complement number: chi * 2^32 has the low word chi << 32 and the high
             * word chi >> 32 (arithmetic); adding the unsigned clo carries at most one into the high word */
            const uint64_t low = (uint64_t)chi[j] << 32;
            c.n = cn[j];
            c.min = cn[j] ? cmin[j] : 0;
            c.max = cn[j] ? cmax[j] : 0;
            c.sum_lo = low + clo[j];
            c.sum_hi = (chi[j] >> 32) + (c.sum_lo < low ? 1 : 0);
            cells[(uint64_t)k * ncols + j] = c;
        }
    }
}

hipError_t launch_agg(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                      const int32_t *d_dec_status, const void *d_atts, const void *d_keys, uint32_t nkeys, const void *d_cols,
                      uint32_t ncols, uint32_t max_att, uint32_t truth, bool floats, uint4 *d_blocks, void *d_cells)
{
    if (cnt == 0) return hipSuccess;
    if ((dec_stride & 15u) != 0 || (((uintptr_t)d_dec | (uintptr_t)d_blocks) & 15u) != 0 ||
        (((uintptr_t)d_cells | (uintptr_t)d_keys | (uintptr_t)d_cols) & 7u) != 0 || ((uintptr_t)d_atts & 3u) != 0 || block_size < 16u ||
        nkeys > 4u || truth > 0xFFFFu || ncols == 0u || ncols > kAggMaxCols)
        return hipErrorInvalidValue;
    if (floats) /* a float key or a float aggregate column: agg_float.hip's kernel */
        return launch_aggf(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_cols, ncols, max_att, truth,
                           d_blocks, d_cells);
    hipLaunchKernelGGL(truth ? k_agg_block<true> : k_agg_block<false>, dim3((cnt + 3u) / 4u), dim3(256), 0, s, d_dec, dec_stride,
                       block_size, cnt, d_dec_status, (const FilterAtt *)d_atts, (const FilterKey *)d_keys, nkeys | truth << 16,
                       (const AggCol *)d_cols, ncols, max_att, d_blocks, (AggCell *)d_cells);
    return hipGetLastError();
}

} // namespace cryo
