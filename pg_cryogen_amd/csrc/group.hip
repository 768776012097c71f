/*
 * group.hip -- the device side of the grouped scan (cryo_codec_group_batch / _blocks, include/cryo_codec.h: the rules).
 *
 * The host (cryo_codec.cpp, group_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); these kernels look into every heap tuple of the decoded chunk as the scan aggregate does, partition each block's
 * matches by one or two integer columns and reduce up to four more columns per group, so that a row per block and a record and a
 * few cells per group leave the device:
 *   k_group_block    one wave per block, two blocks per workgroup (a wave's share of LDS is 16 240 bytes): the sweep of
 *                    scan_sweep.h, whose walk runs over the columns 1 .. max(highest key, group, aggregate column) with six
 *                    capture slots, and instead of reducing as it goes the wave (group_lds.h, group_block: the three steps are
 *                    stated there once for every block kernel of the grouped scan)
 *                      1. compacts the matches in position order into LDS (group_matches);
 *                      2. ranks them, which sorts them by key without an exchange and marks every group's head (group_rank);
 *                      3. counts the heads in sorted order with a ballot prefix across the turns (n_groups); the lane that holds
 *                         a head walks its run, reduces every aggregate column into the running state of agg_cell.h (a run has
 *                         at most 290 values, a block's), and writes the group's record and cells to the block's row of a side
 *                         area in handle workspace (group_reduce).
 *                    A descriptor with a byte-string key runs k_group_block<true>, whose walk compares
 *                    those too and counts an undecided tuple in n_bad; every other descriptor runs k_group_block<false>.
 *   k_group_offsets  one workgroup per chunk: the tiled scan of heap_block.h (offsets_of_rows) over the blocks' n_groups, from the
 *                    running total the chunk before left in device memory; it writes first_group into the rows.
 *   k_group_copy     a grid stride over the blocks: block k's records and cells from the side area to first_group of the call's
 *                    output, word by word, cut off at group_cap.
 * A descriptor with a float key or a float aggregate column runs group_float.hip's k_groupf_block in k_group_block's place
 * (launch_group's `floats`), a descriptor with bucketed group columns group_bucket.hip's k_groupb_block (launch_group's
 * d_buckets), a descriptor with a byte-string group column group_text.hip's k_groupt_block (launch_group's text); the other two
 * kernels serve all of them.
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "group_lds.h"

namespace cryo {

template <bool BYTES>
__global__ void __launch_bounds__(64 * kGroupWaves)
k_group_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
              const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
              const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t side_stride,
              uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
    uint32_t k, lane;
    GroupLds &L = lds[sweep_wave(kGroupWaves, k, lane)];
    if (k >= cnt) return;
    group_block<BYTES, false>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, max_att, side_stride, blocks,
                              side_rec, side_cell);
}

/* first_group of every row of the chunk: the groups before block k, counted from the call's start; *running: the total before
 * the chunk in, after it out */
__global__ void __launch_bounds__(256)
k_group_offsets(uint32_t cnt, uint64_t *__restrict__ running, uint4 *__restrict__ blocks)
{
    __shared__ uint64_t wave_sum[4];
    offsets_of_rows(cnt, running, blocks, wave_sum);
}

/* records (3 words each) and cells (5 words each) of the chunk's blocks from the side area to their places within the call;
 * ncols: the cells of a group (with a text group column its key cells count, launch_group) */
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
                        uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t truth, bool floats, bool like, uint4 *d_blocks, void *d_side_rec, void *d_side_cell,
                        uint64_t *d_running, void *d_rec, void *d_cells, uint64_t group_cap, int cus, const void *d_buckets, uint32_t text)
{
    if (cnt == 0) return hipSuccess;
    const uint32_t cpg = ncols + (uint32_t)__builtin_popcount(text); /* a group's cells: ncols unless it has key cells */
    if (!scan_launch_ok(dec_stride, d_dec, d_blocks, d_atts, d_keys,
                        (uintptr_t)d_rec | (uintptr_t)d_cells | (uintptr_t)d_slots | (uintptr_t)d_side_rec | (uintptr_t)d_side_cell |
                            (uintptr_t)d_running,
                        block_size, nkeys, truth, floats || like) ||
        nby == 0u || nby > kGroupMaxBy || ncols > kAggMaxCols || (text >> nby) != 0u || (text != 0u && d_buckets) ||
        !d_slots || !d_side_rec || !d_running || (cpg > 0u && !d_side_cell) || (group_cap > 0u && (!d_rec || (cpg > 0u && !d_cells))))
        return hipErrorInvalidValue;
    const uint32_t stride = filter_side_stride(block_size);
    hipError_t e;
    if (text && like) /* a byte-string group column and a pattern key: group_text.hip's second unit, then the same two on cpg cells */
        e = launch_grouptl_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, nby, ncols, text,
                                 max_att, truth, stride, d_blocks, d_side_rec, d_side_cell);
    else if (text) /* a byte-string group column: group_text.hip's block kernels, then the same two on cpg cells a group */
        e = launch_groupt_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, nby, ncols, text,
                                max_att, truth, floats, stride, d_blocks, d_side_rec, d_side_cell);
    else if (d_buckets && like) /* buckets and a pattern key: group_bucket.hip's second unit, then the same two */
        e = launch_groupbl_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, d_buckets, nby, ncols,
                                 max_att, truth, stride, d_blocks, d_side_rec, d_side_cell);
    else if (d_buckets) /* a CRYO_GROUP_BUCKETS descriptor: group_bucket.hip's block kernels, then the same two */
        e = launch_groupb_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, d_buckets, nby, ncols,
                                max_att, truth, floats, stride, d_blocks, d_side_rec, d_side_cell);
    else if (like) /* a pattern key: group_float.hip's second unit, then the same two */
        e = launch_groupl_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, nby, ncols, max_att,
                                truth, stride, d_blocks, d_side_rec, d_side_cell);
    else if (floats) /* a float key or a float aggregate column: group_float.hip's block kernel, then the same two */
        e = launch_groupf_block(s, d_dec, dec_stride, block_size, cnt, d_dec_status, d_atts, d_keys, nkeys, d_slots, nby, ncols, max_att,
                                truth, stride, d_blocks, d_side_rec, d_side_cell);
    else {
        hipLaunchKernelGGL(truth ? k_group_block<true> : k_group_block<false>, dim3((cnt + kGroupWaves - 1u) / kGroupWaves), dim3(64 * kGroupWaves), 0, s, d_dec, dec_stride,
                           block_size, cnt, d_dec_status, (const FilterAtt *)d_atts, (const FilterKey *)d_keys, nkeys | truth << 16,
                           (const AggCol *)d_slots, nby, ncols, max_att, stride, d_blocks, (GroupRec *)d_side_rec,
                           (AggCell *)d_side_cell);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_group_offsets, dim3(1), dim3(256), 0, s, cnt, d_running, d_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    /* four workgroups per compute unit, but never more than the chunk has blocks */
    uint64_t grid = (uint64_t)(cus > 0 ? cus : 256) * 4u;
    if (grid > cnt) grid = cnt;
    hipLaunchKernelGGL(k_group_copy, dim3((uint32_t)grid), dim3(256), 0, s, cnt, stride, cpg, (const uint4 *)d_blocks,
                       (const uint64_t *)d_side_rec, (const uint64_t *)d_side_cell, (uint64_t *)d_rec, (uint64_t *)d_cells, group_cap);
    return hipGetLastError();
}

} // namespace cryo
