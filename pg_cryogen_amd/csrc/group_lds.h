/*
 * group_lds.h -- what the grouped scan's two block kernels (group.hip: k_group_block; group_float.hip: k_groupf_block) share: the
 * records' layout, a wave's matches in LDS, the wave's barrier between its LDS writes and reads, and the two steps that lead up
 * to a kernel's own reduction: the matches into LDS (group_matches) and their ranks (group_rank).  group_bucket.hip's
 * k_groupb_block is a third user: it hands group_matches a step that maps the captured group values (GroupRawKeys: none).
 * group_text.hip's k_groupt_block keeps the layout (GroupLds inside its own, wider LDS) and the barrier and states steps 1 and 2
 * for keys that carry a byte string's words: group_matches and group_rank stay as they are for the three kernels above.
 */
#pragma once
#include "kernels.h"
#include "agg_cell.h"
#include "scan_sweep.h"

namespace cryo {

constexpr uint32_t kGroupMaxBy = 2u;
constexpr uint32_t kGroupSlots = kGroupMaxBy + kAggMaxCols; /* capture slots: the group columns, then the aggregate columns */
constexpr uint32_t kGroupWaves = 2u;                        /* blocks per workgroup */

struct GroupRec { int64_t key[2]; uint32_t n_rows, nulls; }; /* cryo_group_rec; a group's cells are AggCell (agg_cell.h) */
static_assert(sizeof(GroupRec) == 24 && sizeof(cryo_group_rec) == 24, "the record's layout is the header's");

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

/* group_matches' step between a turn's capture and its compaction: the kernels that group by the raw values pass this one, which
 * does nothing; group_bucket.hip passes the step that maps a group value to its bucket and turns an undecided match into a bad item */
struct GroupRawKeys { __device__ void operator()(WalkCaptureN<kGroupSlots> &, SweepItem &) const {} };

/* Step 1 of a block kernel: the sweep of scan_sweep.h over an opened block, with six capture slots (slots: the nby group columns,
 * then the aggregate columns) and the walk's BYTES and FLOATS as the kernel's.  The wave compacts the matches in position order
 * into L (ballot + popcount prefix): per match the two group values, the null bits and the captured aggregate values.  keys_of
 * sees every turn's capture and verdict first, the same call in all 64 lanes */
template <bool BYTES, bool FLOATS, class KEYS = GroupRawKeys>
__device__ inline void group_matches(GroupLds &L, const uint8_t *__restrict__ p, uint32_t B, uint32_t n, uint32_t upper, uint32_t lane,
                                     const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                                     uint32_t max_att, const AggCol *__restrict__ slots, uint32_t nby, uint32_t &n_match, uint32_t &n_bad,
                                     const KEYS keys_of = KEYS())
{
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t by_mask = (1u << nby) - 1u;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        WalkCaptureN<kGroupSlots> cap;
        SweepItem it = sweep_turn<true, kGroupSlots, BYTES, false, FLOATS>(p, B, n, upper, t0 + lane, atts, keys, nkeys, max_att, slots,
                                                                          kGroupSlots, &cap);
        keys_of(cap, it);
        const unsigned long long mm = __ballot(it.match);
        if (it.match) {
            const uint32_t at = n_match + (uint32_t)__popcll(mm & below); /* below n <= 290 */
#pragma unroll
            for (uint32_t j = 0; j < kGroupMaxBy; j++) L.key[j][at] = cap.v[j]; /* 0 when NULL or not a group column */
#pragma unroll
            for (uint32_t j = 0; j < kAggMaxCols; j++) L.val[j][at] = cap.v[kGroupMaxBy + j];
            L.meta[at] = (~cap.has & by_mask) | (cap.has & ~3u);
        }
        n_match += (uint32_t)__popcll(mm);
        n_bad += (uint32_t)__popcll(__ballot(it.bad));
    }
    group_wave_sync();
}

/* Step 2, the rank pass over the m matches in L: the place of match i is (matches with a smaller key) + (earlier matches with an
 * equal key), m uniform LDS reads per lane and turn (m <= 290).  The two counts add up to the match's place in the contract's
 * order -- a stable sort without a single exchange, so equal keys lie together in position order and the result does not depend
 * on timing -- and a match whose second count is 0 is its group's head.  A key is (null 1, value 1, null 2, value 2) with NULL
 * after every value; a NULL's value is 0, so equal null bits and equal values make equal keys.  A bitonic network over 512 padded
 * slots would need 45 compare-exchange steps with a wave barrier each and an index to break ties; the rank pass needs two
 * barriers in all */
__device__ inline void group_rank(GroupLds &L, uint32_t m, uint32_t lane)
{
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
}

} // namespace cryo
