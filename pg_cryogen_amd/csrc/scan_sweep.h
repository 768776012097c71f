/*
 * scan_sweep.h -- where the block rules (heap_block.h) meet the tuple walk (filter_walk.h): the sweep over a decoded block's items
 * that the six block kernels of the scan calls share (filter.hip, project.hip, agg.hip, agg_float.hip, group.hip, group_float.hip).
 * One wave takes one block.  A block the decoders rejected gets STREAM without a load, a bad header HEADER.  Otherwise a lane
 * takes one item per turn (290 items: five turns): the ITEM rule, then the walk over the tuple's columns, which tests the keys and
 * notes the columns a kernel captures.  Every turn is the same trip for all 64 lanes: the descriptor, the keys and the captured
 * columns are read at addresses that depend on loop counters only (uniform loads); what differs per lane is the offset, the
 * null bit and the varlena branch.  A column's value is loaded at its proven alignment (tuples start at multiples of 8, hoff is
 * one, attalign >= attlen is the argument rule); everything else of a tuple is read bytewise or, the three header fields, at
 * their fixed even offsets.  No load leaves [t, t + len): every read is preceded by its bound.  What a kernel does with a
 * turn's matches and bad items is its own.
 *   sweep_wave   which block the wave takes and the lane's number in it
 *   sweep_open   STREAM, HEADER, or the block's items and tuples
 *   sweep_turn   one item: ITEM, the walk, and the verdict sorted into match / bad / neither
 * And, for the host, the launch of such a kernel: scan_block_launch, and on it the helpers of the three calls whose units share
 * this header alone (filter_launch, agg_launch, project_launch; the grouped scan's is group_lds.h's, the ordered scan's topn.hip's).
 */
#pragma once
#include "kernels.h"
#include "heap_block.h"
#include "filter_walk.h"

namespace cryo {

/* The block of this wave, of `waves` per workgroup; the wave's number comes back.  It goes through readfirstlane: the compiler
 * then knows the block, its header and the trip counts to be the same in all 64 lanes, and keeps them and the descriptor reads
 * in scalar registers */
__device__ inline uint32_t sweep_wave(uint32_t waves, uint32_t &k, uint32_t &lane)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    k = blockIdx.x * waves + wave;
    lane = threadIdx.x & 63u;
    return wave;
}

/* Block k of the decoded chunk: 0 -- its n item ids lie at p + 8 and its tuples in [upper, B) --, kFilterStream (the decoders
 * rejected the stream: nothing decoded to look at, nothing loaded) or kFilterHeader; n is 0 with either status */
__device__ inline uint32_t sweep_open(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B,
                                      const int32_t *__restrict__ dec_status, uint32_t k, const uint8_t *__restrict__ &p, uint32_t &n,
                                      uint32_t &upper)
{
    p = dec + (uint64_t)k * dec_stride;
    n = upper = 0;
    if (dec_status[k] != 0) return kFilterStream;
    const uint2 hdr = *reinterpret_cast<const uint2 *>(p);
    if (heap_header(hdr, B, n, upper)) return 0u;
    n = 0;
    return kFilterHeader;
}

/* what a turn found of item i: the verdict (0, kFilterNoMatch -- a lane without an item has it too --, kFilterItem, kFilterTuple,
 * kFilterUndecided), the tuple's place in the block and its length when the item is good, and the verdict's class: a match, a
 * bad item (counted in n_bad, listed where the call lists), or neither */
struct SweepItem { uint32_t verdict, src, len; bool match, bad; };

/* One turn of the sweep for item i of an opened block (i >= n: a lane without an item, which makes the same trips and loads
 * nothing).  The template parameters and atts .. cols, ncols are walk_tuple's; *cap is cleared, then filled (CAPTURE alone: the
 * filter passes null; TEXT and LIKE are the walk's too).  Without BYTES no tuple is undecided: the float kernels, which always run the table's path, are BYTES */
template <bool CAPTURE, uint32_t SLOTS, bool BYTES, bool NARROW, bool FLOATS, bool TEXT = false, bool LIKE = false>
__device__ inline SweepItem sweep_turn(const uint8_t *__restrict__ p, uint32_t B, uint32_t n, uint32_t upper, uint32_t i,
                                       const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                                       uint32_t max_att, const AggCol *__restrict__ cols, uint32_t ncols,
                                       typename WalkPlain<WalkCaptureN<SLOTS>>::type *cap)
{
    SweepItem it;
    it.verdict = kFilterNoMatch;
    it.src = it.len = 0;
    const bool valid = i < n;
    if (valid) {
        const uint2 id = *reinterpret_cast<const uint2 *>(p + 8u + 8u * i); /* 8 + 8 n = lower <= B */
        if (!heap_item(id, upper, B, it.src, it.len)) it.verdict = kFilterItem;
    }
    const bool live = valid && it.verdict != kFilterItem;
    if (CAPTURE) {
        cap->has = 0;
#pragma unroll
        for (uint32_t j = 0; j < SLOTS; j++) cap->v[j] = 0;
    }
    const uint32_t walked = walk_tuple<CAPTURE, SLOTS, BYTES, NARROW, FLOATS, TEXT, LIKE>(p + it.src, it.len, live, atts, keys, nkeys, max_att, cols,
                                                                              ncols, cap, WalkKeys<BYTES>());
    if (live) it.verdict = walked;
    it.match = it.verdict == 0u;
    it.bad = it.verdict == kFilterItem || it.verdict == kFilterTuple || (BYTES && it.verdict == kFilterUndecided);
    return it;
}

/* ---- the host's side: the block-kernel launch of the scan calls (kernels.h: ScanChunk, ScanDesc, the calls' own structs) ---- */

/* a block kernel: the eight arguments every one begins with -- the chunk, the descriptor and the keys, scan_nkeys_arg --, then
 * the call's own */
template <class... OWN>
using ScanKernel = void (*)(const uint8_t *, uint64_t, uint32_t, uint32_t, const int32_t *, const FilterAtt *, const FilterKey *, uint32_t, OWN...);

/* The launch, all of it: one wave per block and `waves` blocks per workgroup; the eight arguments, then `own`.  table: the kernel
 * has the truth table's verdict path alone -- every kernel but a call's <false> one --, which needs a table */
template <class... OWN, class... ARGS>
inline hipError_t scan_block_launch(ScanKernel<OWN...> kernel, uint32_t waves, bool table, const ScanChunk &c, const ScanDesc &d, ARGS... own)
{
    if (table && d.truth == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((c.cnt + waves - 1u) / waves), dim3(64u * waves), 0, c.stream, c.d_dec, c.dec_stride, c.block_size, c.cnt,
                       c.d_dec_status, (const FilterAtt *)d.d_atts, (const FilterKey *)d.d_keys, scan_nkeys_arg(d.nkeys, d.truth), own...);
    return hipGetLastError();
}

/* the filter's, the aggregate's and the projection's block kernels: four blocks per workgroup */
template <class K> inline hipError_t filter_launch(K kernel, bool table, const ScanChunk &c, const ScanDesc &d, const FilterLaunch &f)
{
    return scan_block_launch(kernel, 4u, table, c, d, d.max_att, f.count_only ? 1u : 0u, filter_side_stride(c.block_size), f.d_blocks, f.d_side,
                             f.d_sum);
}
struct AggCell; /* agg_cell.h */
template <class K> inline hipError_t agg_launch(K kernel, bool table, const ScanChunk &c, const ScanDesc &d, const AggLaunch &a)
{
    return scan_block_launch(kernel, 4u, table, c, d, (const AggCol *)a.d_cols, a.ncols, d.max_att, a.d_blocks, (AggCell *)a.d_cells);
}
template <class K> inline hipError_t project_launch(K kernel, bool table, const ScanChunk &c, const ScanDesc &d, const ProjectLaunch &p)
{
    return scan_block_launch(kernel, 4u, table, c, d, (const AggCol *)p.d_cols, p.ncols, d.max_att, p.row_bytes / 8u,
                             filter_side_stride(c.block_size), p.d_blocks, (uint2 *)p.d_side_rec, (uint2 *)p.d_side_rows);
}

} // namespace cryo
