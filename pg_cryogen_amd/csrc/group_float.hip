/*
 * group_float.hip -- the grouped scan's block kernel for descriptors with a float key or a float aggregate column
 * (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8; include/cryo_codec.h: "A float column's cell", "The reduction").  Every other descriptor runs
 * group.hip's k_group_block; k_group_offsets and k_group_copy serve both.
 *   k_groupf_block  k_group_block with the walk's FLOATS parameter set and the truth table's verdict path (the AND table from the
 *                   host when the caller gave none): the same LDS layout -- a captured value is its raw 64-bit word, a float4's
 *                   32 bits sign-extended --, the same steps 1 and 2 over the integer group columns (group_lds.h), the same side
 *                   area.  Only step 3 differs (group_reduce's FLOATS), per aggregate column by a uniform branch on its type:
 *                   the head lane that walks its run reduces an integer column as k_group_block does, cell byte for byte, and a
 *                   float column into the count, the minimum and maximum of the mapped values (float_map), three flag bits
 *                   (+Inf, -Inf, NaN seen) and the double-double pair over the finite values, started at (+0, +0) and taken in
 *                   position order -- the order the run has, equal keys lying in position order.
 *                   The body is group_block<true, true> (group_lds.h), k_group_block's with another pair of parameters: the
 *                   branch costs the integer kernels nothing, which compile it away (56 vector registers against 74 here).
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "group_lds.h"

namespace cryo {

#ifndef CRYO_LIKE_UNIT
__global__ void __launch_bounds__(64 * kGroupWaves)
k_groupf_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
               const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
               const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t side_stride,
               uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
    uint32_t k, lane;
    GroupLds &L = lds[sweep_wave(kGroupWaves, k, lane)];
    if (k >= cnt) return;
    group_block<true, true>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, max_att, side_stride, blocks,
                            side_rec, side_cell);
}

hipError_t launch_groupf_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g) { return group_launch(k_groupf_block, true, c, d, g); }

#else /* CRYO_LIKE_UNIT */
/* k_groupf_block whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like), for every descriptor
 * with such a key that has neither buckets nor a text group column: a kernel of its own name, so that k_group_block<true> and
 * k_groupf_block stay the code they were.  Built from this source compiled a second time with CRYO_LIKE_UNIT
 * (group_float_like.o) */
__global__ void __launch_bounds__(64 * kGroupWaves)
k_groupl_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
               const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
               const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t side_stride,
               uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
    uint32_t k, lane;
    GroupLds &L = lds[sweep_wave(kGroupWaves, k, lane)];
    if (k >= cnt) return;
    group_block<true, true, true>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, max_att, side_stride,
                                  blocks, side_rec, side_cell);
}

hipError_t launch_groupl_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g) { return group_launch(k_groupl_block, true, c, d, g); }
#endif

} // namespace cryo
