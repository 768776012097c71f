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
 */
#pragma once
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

} // namespace cryo
