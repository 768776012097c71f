/*
 * group_lds.h -- what the grouped scan's two block kernels (group.hip: k_group_block; group_float.hip: k_groupf_block) share: the
 * records' layout, a wave's matches in LDS and the wave's barrier between its LDS writes and reads.
 */
#pragma once
#include "kernels.h"
#include "filter_walk.h"

namespace cryo {

constexpr uint32_t kGroupMaxBy = 2u;
constexpr uint32_t kGroupSlots = kGroupMaxBy + kAggMaxCols; /* capture slots: the group columns, then the aggregate columns */
constexpr uint32_t kGroupWaves = 2u;                        /* blocks per workgroup */

struct GroupRec { int64_t key[2]; uint32_t n_rows, nulls; };                        /* cryo_group_rec */
struct GroupCell { uint64_t n; int64_t min, max; uint64_t sum_lo; int64_t sum_hi; }; /* cryo_agg_cell */
static_assert(sizeof(GroupRec) == 24 && sizeof(GroupCell) == 40, "the records' layout is the header's");

/* a wave's matches in LDS.  meta: bits 0 .. 1 the group columns' null bits, bits 2 .. 5 set where aggregate column j has a
 * value.  order[s]: the match at place s of the contract's order, bit 16 set when it is a group's head */
struct GroupLds {
    int64_t key[kGroupMaxBy][kHeapMaxItems];
    int64_t val[kAggMaxCols][kHeapMaxItems];
    uint32_t meta[kHeapMaxItems];
    uint32_t order[kHeapMaxItems];
};
static_assert(sizeof(GroupLds) * kGroupWaves <= 65536u, "a workgroup's LDS stays within 64 KiB");

/* the wave's LDS writes are done before its next LDS reads */
__device__ inline void group_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace cryo
