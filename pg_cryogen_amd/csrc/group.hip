/*
 * group.hip -- the device side of the grouped scan (cryo_codec_group_batch / _blocks, include/cryo_codec.h: the rules).
 *
 * The host (cryo_codec.cpp, group_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); these kernels look into every heap tuple of the decoded chunk as the scan aggregate does, partition each block's
 * matches by one or two integer columns and reduce up to four more columns per group, so that a row per block and a record and a
 * few cells per group leave the device:
 *   k_group_block    one wave per block, two blocks per workgroup (a wave's share of LDS is 16 240 bytes).  A block the decoders
 *                    rejected gets STREAM without a load, a bad header (heap_header, heap_block.h) HEADER.  Otherwise the sweep is k_agg_block's -- a lane
 *                    takes one item per turn (290 items: five turns), the ITEM rule (heap_item), then the walk of filter_walk.h over the
 *                    columns 1 .. max(highest key, group, aggregate column) with six capture slots -- and instead of reducing as
 *                    it goes the wave
 *                      1. compacts the matches in position order into LDS (ballot + popcount prefix): per match the two group
 *                         values, the null bits and the captured aggregate values;
 *                      2. ranks them: match i counts the matches with a smaller key and the EARLIER matches with an equal key,
 *                         m uniform LDS reads per lane and turn (m <= 290).  The two counts add up to the match's place in the
 *                         contract's order -- a stable sort without a single exchange, so equal keys lie together in position
 *                         order and the result does not depend on timing -- and a match whose second count is 0 is its group's
 *                         head.  A bitonic network over 512 padded slots would need 45 compare-exchange steps with a wave
 *                         barrier each and an index to break ties; the rank pass needs two barriers in all;
 *                      3. counts the heads in sorted order with a ballot prefix across the turns (n_groups); the lane that holds
 *                         a head walks its run and reduces n, min, max and the two 64-bit halves of the sum as agg.hip does (a
 *                         run has at most 290 values, so neither half overflows), and writes the group's record and cells to the
 *                         block's row of a side area in handle workspace.
 *                    Descriptor, keys and columns are read at addresses that depend on loop counters only (uniform loads); no
 *                    load leaves [t, t + len).  A descriptor with a byte-string key runs k_group_block<true>, whose walk compares
 *                    those too and counts an undecided tuple in n_bad; every other descriptor runs k_group_block<false>.
 *   k_group_offsets  one workgroup per chunk: the tiled scan of heap_block.h (offsets_tile) over the blocks' n_groups, from the running
 *                    total the chunk before left in device memory; it writes first_group into the rows.
 *   k_group_copy     a grid stride over the blocks: block k's records and cells from the side area to first_group of the call's
 *                    output, word by word, cut off at group_cap.
 * A descriptor with a float key or a float aggregate column runs group_float.hip's k_groupf_block in k_group_block's place
 * (launch_group's `floats`); the other two kernels serve both.
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "filter_walk.h"
#include "group_lds.h"

namespace cryo {

template <bool BYTES>
__global__ void __launch_bounds__(64 * kGroupWaves)
k_group_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
              const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
              const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t side_stride,
              uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, GroupCell *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
    /* the wave's number through readfirstlane, as in k_filter_match: the block, its header and the trip counts are the same in
     * all 64 lanes and stay, with the descriptor reads, in scalar registers */
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t k = blockIdx.x * kGroupWaves + wave;
    const uint32_t lane = threadIdx.x & 63u;
    if (k >= cnt) return;
    GroupLds &L = lds[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t by_mask = (1u << nby) - 1u;
    uint32_t status = 0, n_items = 0, n_match = 0, n_bad = 0, n_groups = 0;
    if (dec_status[k] != 0) status = kFilterStream; /* the decoders rejected the stream: nothing decoded to look at */
    else {
        const uint8_t *p = dec + (uint64_t)k * dec_stride;
        const uint2 hdr = *reinterpret_cast<const uint2 *>(p);
        uint32_t n, upper;
        if (!heap_header(hdr, B, n, upper))
            status = kFilterHeader;
        else {
            n_items = n;
            /* 1. the sweep: the matches into LDS in position order */
            for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
                const uint32_t i = t0 + lane;
                const bool valid = i < n;
                uint32_t verdict = kFilterNoMatch, len = 0, src = 0;
                if (valid) {
                    const uint2 it = *reinterpret_cast<const uint2 *>(p + 8u + 8u * i); /* 8 + 8 n = lower <= B */
                    if (!heap_item(it, upper, B, src, len)) verdict = kFilterItem;
                }
                const bool live = valid && verdict != kFilterItem;
                WalkCaptureN<kGroupSlots> cap;
                cap.has = 0;
#pragma unroll
                for (uint32_t j = 0; j < kGroupSlots; j++) cap.v[j] = 0;
                const uint32_t walked =
                    walk_tuple<true, kGroupSlots>(p + src, len, live, atts, keys, nkeys, max_att, slots, kGroupSlots, &cap, WalkKeys<BYTES>());
                if (live) verdict = walked;
                const bool match = verdict == 0u,
                           bad = verdict == kFilterItem || verdict == kFilterTuple || (BYTES && verdict == kFilterUndecided);
                const unsigned long long mm = __ballot(match);
                if (match) {
                    const uint32_t at = n_match + (uint32_t)__popcll(mm & below); /* below n <= 290 */
#pragma unroll
                    for (uint32_t j = 0; j < kGroupMaxBy; j++) L.key[j][at] = cap.v[j]; /* 0 when NULL or not a group column */
#pragma unroll
                    for (uint32_t j = 0; j < kAggMaxCols; j++) L.val[j][at] = cap.v[kGroupMaxBy + j];
                    L.meta[at] = (~cap.has & by_mask) | (cap.has & ~3u);
                }
                n_match += (uint32_t)__popcll(mm);
                n_bad += (uint32_t)__popcll(__ballot(bad));
            }
            const uint32_t m = n_match;
            group_wave_sync();
            /* 2. the rank pass: the place of match i is (matches with a smaller key) + (earlier matches with an equal key).  A
             * key is (null 1, value 1, null 2, value 2) with NULL after every value; a NULL's value is 0, so equal null bits and
             * equal values make equal keys */
            for (uint32_t t0 = 0; t0 < m; t0 += 64u) {
                const uint32_t i = t0 + lane;
                const bool on = i < m;
                const uint32_t me = on ? i : 0u;
                const int64_t k0 = L.key[0][me], k1 = L.key[1][me];
                const uint32_t kn = L.meta[me] & 3u;
                uint32_t less = 0, same_before = 0;
                for (uint32_t j = 0; j < m; j++) { /* uniform addresses: one LDS read serves the wave */
                    const int64_t a0 = L.key[0][j], a1 = L.key[1][j];
                    const uint32_t an = L.meta[j] & 3u;
                    const bool lt0 = (an & 1u) != (kn & 1u) ? (an & 1u) == 0u : a0 < k0;
                    const bool eq0 = (an & 1u) == (kn & 1u) && a0 == k0;
                    const bool lt1 = (an & 2u) != (kn & 2u) ? (an & 2u) == 0u : a1 < k1;
                    const bool eq1 = (an & 2u) == (kn & 2u) && a1 == k1;
                    less += (lt0 || (eq0 && lt1)) ? 1u : 0u;
                    same_before += (eq0 && eq1 && j < i) ? 1u : 0u;
                }
                if (on) L.order[less + same_before] = i | (same_before == 0u ? 1u << 16 : 0u); /* a permutation of 0 .. m - 1 */
            }
            group_wave_sync();
            /* 3. one lane per group: the head's lane walks the run up to the next head */
            GroupRec *out_rec = side_rec + (uint64_t)k * side_stride;
            GroupCell *out_cell = side_cell + (uint64_t)k * side_stride * ncols;
            for (uint32_t t0 = 0; t0 < m; t0 += 64u) {
                const uint32_t s = t0 + lane;
                const uint32_t o = s < m ? L.order[s] : 0u;
                const bool head = (o >> 16) != 0u;
                const unsigned long long mh = __ballot(head);
                if (head) {
                    const uint32_t g = n_groups + (uint32_t)__popcll(mh & below); /* below m <= n <= side_stride */
                    const uint32_t first = o & 0xFFFFu;
                    uint32_t rows = 0;
                    uint32_t cn[kAggMaxCols];
                    int64_t cmin[kAggMaxCols], cmax[kAggMaxCols], chi[kAggMaxCols];
                    uint64_t clo[kAggMaxCols];
#pragma unroll
                    for (uint32_t j = 0; j < kAggMaxCols; j++) { cn[j] = 0; cmin[j] = INT64_MAX; cmax[j] = INT64_MIN; clo[j] = 0; chi[j] = 0; }
                    for (uint32_t r = s;;) {
                        const uint32_t i = L.order[r] & 0xFFFFu;
                        const uint32_t has = L.meta[i] >> 2;
                        rows++;
#pragma unroll
                        for (uint32_t j = 0; j < kAggMaxCols; j++) {
                            if (j >= ncols || ((has >> j) & 1u) == 0) continue; /* a NULL adds nothing */
                            const int64_t v = L.val[j][i];
                            cn[j]++;
                            cmin[j] = v < cmin[j] ? v : cmin[j];
                            cmax[j] = v > cmax[j] ? v : cmax[j];
                            clo[j] += (uint64_t)v & 0xFFFFFFFFull;
                            chi[j] += v >> 32; /* arithmetic: v = (v >> 32) * 2^32 + (v & 0xFFFFFFFF) */
                        }
                        r++;
                        if (r >= m || (L.order[r] >> 16) != 0u) break;
                    }
                    GroupRec rec;
                    rec.key[0] = L.key[0][first];
                    rec.key[1] = L.key[1][first];
                    rec.n_rows = rows;
                    rec.nulls = L.meta[first] & 3u;
                    out_rec[g] = rec;
#pragma unroll
                    for (uint32_t j = 0; j < kAggMaxCols; j++) {
                        if (j >= ncols) continue; /* uniform */
                        GroupCell c;
                        /* sum = chi * 2^32 + clo as a 128-bit two's-complement number, as in agg.hip */
                        const uint64_t low = (uint64_t)chi[j] << 32;
                        c.n = cn[j];
                        c.min = cn[j] ? cmin[j] : 0;
                        c.max = cn[j] ? cmax[j] : 0;
                        c.sum_lo = low + clo[j];
                        c.sum_hi = (chi[j] >> 32) + (c.sum_lo < low ? 1 : 0);
                        out_cell[(uint64_t)g * ncols + j] = c;
                    }
                }
                n_groups += (uint32_t)__popcll(mh);
            }
        }
    }
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n_items, n_match, n_bad);
        blocks[2u * k + 1u] = make_uint4(n_groups, 0u, 0u, 0u); /* first_group: k_group_offsets */
    }
}

/* first_group of every row of the chunk: the groups before block k, counted from the call's start; *running: the total before
 * the chunk in, after it out */
__global__ void __launch_bounds__(256)
k_group_offsets(uint32_t cnt, uint64_t *__restrict__ running, uint4 *__restrict__ blocks)
{
    __shared__ uint64_t wave_sum[4];
    uint64_t run = running[0]; /* the same in every thread; written again only after the tiles' barriers */
    for (uint32_t t = 0; t < cnt; t += 256u) {
        const uint32_t k = t + threadIdx.x;
        const uint64_t a[1] = {k < cnt ? blocks[2u * k + 1u].x : 0u};
        uint64_t before[1], tile[1];
        offsets_tile(a, wave_sum, before, tile);
        if (k < cnt) {
            const uint64_t first = run + before[0];
            blocks[2u * k + 1u] = make_uint4((uint32_t)a[0], 0u, (uint32_t)first, (uint32_t)(first >> 32));
        }
        run += tile[0];
    }
    if (threadIdx.x == 0) running[0] = run;
}

/* records (3 words each) and cells (5 words each) of the chunk's blocks from the side area to their places within the call */
__global__ void __launch_bounds__(256)
k_group_copy(uint32_t cnt, uint32_t side_stride, uint32_t ncols, const uint4 *__restrict__ blocks,
             const uint64_t *__restrict__ side_rec, const uint64_t *__restrict__ side_cell, uint64_t *__restrict__ rec,
             uint64_t *__restrict__ cells, uint64_t group_cap)
{
    for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
        const uint4 row = blocks[2u * k + 1u];
        const uint64_t first = (uint64_t)row.z | (uint64_t)row.w << 32;
        uint32_t ng = row.x;
        if (ng > side_stride) ng = side_stride;
        if (first >= group_cap) continue;
        if (group_cap - first < ng) ng = (uint32_t)(group_cap - first); /* nothing at or beyond group_cap */
        const uint64_t *sr = side_rec + (uint64_t)k * side_stride * 3u;
        for (uint32_t w = threadIdx.x; w < ng * 3u; w += 256u) rec[first * 3u + w] = sr[w];
        const uint32_t cw = 5u * ncols;
        const uint64_t *sc = side_cell + (uint64_t)k * side_stride * cw;
        for (uint32_t w = threadIdx.x; w < ng * cw; w += 256u) cells[first * cw + w] = sc[w];
    }
}

hipError_t launch_group(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                        const int32_t *d_dec_status, const void *d_atts, const void *d_keys, uint32_t nkeys, const void *d_slots,
                        uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t truth, bool floats, uint4 *d_blocks, void *d_side_rec, void *d_side_cell,
                        uint64_t *d_running, void *d_rec, void *d_cells, uint64_t group_cap, int cus)
{
    if (cnt == 0) return hipSuccess;
    if ((dec_stride & 15u) != 0 || (((uintptr_t)d_dec | (uintptr_t)d_blocks) & 15u) != 0 ||
        (((uintptr_t)d_rec | (uintptr_t)d_cells | (uintptr_t)d_keys | (uintptr_t)d_slots | (uintptr_t)d_side_rec |
          (uintptr_t)d_side_cell | (uintptr_t)d_running) & 7u) != 0 ||
        ((uintptr_t)d_atts & 3u) != 0 || block_size < 16u || nkeys > 4u || truth > 0xFFFFu || (floats && truth == 0u) || nby == 0u || nby > kGroupMaxBy || ncols > kAggMaxCols ||
        !d_slots || !d_side_rec || !d_running || (ncols > 0u && !d_side_cell) || (group_cap > 0u && (!d_rec || (ncols > 0u && !d_cells))))
        return hipErrorInvalidValue;
    const uint32_t stride = filter_side_stride(block_size);
    hipError_t e;
    if (floats) /* a float key or a float aggregate column: group_float.hip's block kernel, then the same two */
        e = launch_groupf_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, nby, ncols, max_att,
                                truth, stride, d_blocks, d_side_rec, d_side_cell);
    else {
        hipLaunchKernelGGL(truth ? k_group_block<true> : k_group_block<false>, dim3((cnt + kGroupWaves - 1u) / kGroupWaves), dim3(64 * kGroupWaves), 0, s, d_dec, dec_stride,
                           block_size, cnt, d_dec_status, (const FilterAtt *)d_atts, (const FilterKey *)d_keys, nkeys | truth << 16,
                           (const AggCol *)d_slots, nby, ncols, max_att, stride, d_blocks, (GroupRec *)d_side_rec,
                           (GroupCell *)d_side_cell);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_group_offsets, dim3(1), dim3(256), 0, s, cnt, d_running, d_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    /* four workgroups per compute unit, but never more than the chunk has blocks */
    uint64_t grid = (uint64_t)(cus > 0 ? cus : 256) * 4u;
    if (grid > cnt) grid = cnt;
    hipLaunchKernelGGL(k_group_copy, dim3((uint32_t)grid), dim3(256), 0, s, cnt, stride, ncols, (const uint4 *)d_blocks,
                       (const uint64_t *)d_side_rec, (const uint64_t *)d_side_cell, (uint64_t *)d_rec, (uint64_t *)d_cells, group_cap);
    return hipGetLastError();
}

} // namespace cryo
