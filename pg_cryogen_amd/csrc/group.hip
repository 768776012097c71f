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
 * (ScanDesc::floats), a descriptor with bucketed group columns group_bucket.hip's k_groupb_block (ScanDesc::d_buckets), a
 * descriptor with a byte-string group column group_text.hip's k_groupt_block (ScanDesc::text); the other two kernels serve all
 * of them.
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
 * ncols: the cells of a group (with a text group column its key cells count: launch_group's cpg) */
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

hipError_t launch_group(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    if (c.cnt == 0) return hipSuccess;
    if (!group_launch_ok(c, d, g)) return hipErrorInvalidValue;
    /* the block kernel of the descriptor's route (kernels.h: the table), then the same two for all: on ncols cells a group, and
     * behind group_text.hip's kernels on the key cells too */
    hipError_t e = hipErrorInvalidValue;
    switch (group_route(d.text, d.d_buckets != nullptr, d.truth, d.floats, d.like)) {
    case kGroupTextLike: e = launch_grouptl_block(c, d, g); break;
    case kGroupText:
    case kGroupTextFloat: e = launch_groupt_block(c, d, g); break;
    case kGroupBucketLike: e = launch_groupbl_block(c, d, g); break;
    case kGroupBucket:
    case kGroupBucketFloat: e = launch_groupb_block(c, d, g); break;
    case kGroupLike: e = launch_groupl_block(c, d, g); break;
    case kGroupFloat: e = launch_groupf_block(c, d, g); break;
    case kGroupTable: e = group_launch(k_group_block<true>, true, c, d, g); break;
    case kGroupPlain: e = group_launch(k_group_block<false>, false, c, d, g); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_group_offsets, dim3(1), dim3(256), 0, c.stream, c.cnt, g.d_running, g.d_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t cpg = g.ncols + (uint32_t)__builtin_popcount(d.text); /* a group's cells: ncols unless it has key cells */
    hipLaunchKernelGGL(k_group_copy, dim3(scan_copy_grid(c.cus, c.cnt)), dim3(256), 0, c.stream, c.cnt, filter_side_stride(c.block_size), cpg,
                       (const uint4 *)g.d_blocks, (const uint64_t *)g.d_side_rec, (const uint64_t *)g.d_side_cell, (uint64_t *)g.d_rec,
                       (uint64_t *)g.d_cells, g.group_cap);
    return hipGetLastError();
}

} // namespace cryo
