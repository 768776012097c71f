/*
 * group_lds.h -- what the grouped scan's block kernels (group.hip: k_group_block; group_float.hip: k_groupf_block;
 * group_bucket.hip: k_groupb_block; group_text.hip: k_groupt_block) share: the records' layout, a wave's matches in LDS, the
 * wave's barrier between its LDS writes and reads, and a block kernel's three steps: the matches into LDS (group_matches), their
 * ranks (group_rank) and the reduction of every group's run into its record and cells (group_reduce).  The first three kernels
 * are one body (group_block) that differs in the walk's BYTES and FLOATS and in the step that maps the captured group values
 * (GroupRawKeys: none; group_bucket.hip: to bucket keys).  k_groupt_block keeps the layout (GroupLds inside its own, wider LDS)
 * and the barrier, states steps 1 and 2 for keys that carry a byte string's words, and hands group_reduce the step that writes
 * a group's key cells (GroupNoKeyCells: none).  And, for the host, the launch of such a kernel (group_launch), which the four
 * units' launchers share.
 */
#pragma once
#include "kernels.h"
#include "agg_cell.h"
#include "float_pair.h"
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
 * then the aggregate columns) and the walk's BYTES, FLOATS and LIKE as the kernel's.  The wave compacts the matches in position order
 * into L (ballot + popcount prefix): per match the two group values, the null bits and the captured aggregate values.  keys_of
 * sees every turn's capture and verdict first, the same call in all 64 lanes */
template <bool BYTES, bool FLOATS, bool LIKE = false, class KEYS = GroupRawKeys>
__device__ inline void group_matches(GroupLds &L, const uint8_t *__restrict__ p, uint32_t B, uint32_t n, uint32_t upper, uint32_t lane,
                                     const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                                     uint32_t max_att, const AggCol *__restrict__ slots, uint32_t nby, uint32_t &n_match, uint32_t &n_bad,
                                     const KEYS keys_of = KEYS())
{
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t by_mask = (1u << nby) - 1u;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        WalkCaptureN<kGroupSlots> cap;
        SweepItem it = sweep_turn<true, kGroupSlots, BYTES, false, FLOATS, false, LIKE>(p, B, n, upper, t0 + lane, atts, keys, nkeys, max_att,
                                                                                       slots, kGroupSlots, &cap);
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

/* group_reduce's step behind a group's aggregate cells: the kernels without a text group column pass this one, which does nothing;
 * group_text.hip passes the step that writes the key cells.  cell: the index of the group's first cell after the aggregate cells
 * within the block's row of the side area; first: the group's first match in L */
struct GroupNoKeyCells { __device__ void operator()(uint64_t, uint32_t) const {} };

/* Step 3, the reduction over the m ranked matches in L: one lane per group.  The heads are counted in sorted order with a ballot
 * prefix across the turns; the lane that holds a head walks its run in L.order up to the next head (a run has at most 290 values,
 * a block's) and reduces every aggregate column into the running state of agg_cell.h -- with FLOATS, by a uniform branch on the
 * column's type, a float column into the count, the minimum and maximum of the mapped values (float_map), three flag bits (+Inf,
 * -Inf, NaN seen) and the double-double pair over the finite values, started at (+0, +0) and taken in position order, the order
 * the run has; without FLOATS that branch is not compiled.  The lane writes the group's record to out_rec and its cells to
 * out_cell, cpg cells a group (the block's rows of the side area; out_cell is not touched when a group has no cell), and
 * key_cells follows.  The number of groups comes back, the same in all 64 lanes */
template <bool FLOATS, class KEYCELLS = GroupNoKeyCells>
__device__ inline uint32_t group_reduce(const GroupLds &L, uint32_t m, uint32_t lane, const AggCol *__restrict__ slots, uint32_t ncols,
                                        uint32_t cpg, GroupRec *__restrict__ out_rec, AggCell *__restrict__ out_cell,
                                        const KEYCELLS key_cells = KEYCELLS())
{
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t n_groups = 0;
    for (uint32_t t0 = 0; t0 < m; t0 += 64u) {
        const uint32_t s = t0 + lane;
        const uint32_t o = s < m ? L.order[s] : 0u;
        const bool head = (o >> 16) != 0u;
        const unsigned long long mh = __ballot(head);
        if (head) {
            const uint32_t g = n_groups + (uint32_t)__popcll(mh & below); /* below m <= n <= side_stride */
            const uint32_t first = o & 0xFFFFu;
            uint32_t rows = 0;
            uint32_t cn[kAggMaxCols], flags = 0; /* flags: three bits per float column */
            int64_t cmin[kAggMaxCols], cmax[kAggMaxCols];
            uint64_t ca[kAggMaxCols], cb[kAggMaxCols]; /* an integer column's sum halves; a float column's hi and lo bits */
#pragma unroll
            for (uint32_t j = 0; j < kAggMaxCols; j++) { cn[j] = 0; cmin[j] = INT64_MAX; cmax[j] = INT64_MIN; ca[j] = 0; cb[j] = 0; }
            for (uint32_t r = s;;) {
                const uint32_t i = L.order[r] & 0xFFFFu;
                const uint32_t has = L.meta[i] >> 2;
                rows++;
#pragma unroll
                for (uint32_t j = 0; j < kAggMaxCols; j++) {
                    if (j >= ncols || ((has >> j) & 1u) == 0) continue; /* a NULL adds nothing */
                    int64_t v = L.val[j][i];
                    cn[j]++;
                    const uint32_t type = FLOATS ? slots[kGroupMaxBy + j].type : 0u; /* uniform */
                    if (FLOATS && type >= kKeyFloat4) {
                        /* the run's values in position order into the pair; what is not finite into the flags alone */
                        const uint64_t b = float_bits(v, type == kKeyFloat4);
                        const uint32_t f = float_flag(b);
                        v = float_map(b);
                        flags |= f << (3u * j);
                        if (f == 0u) float_pair_take(b, ca[j], cb[j]);
                    } else cell_sum(v, ca[j], cb[j]);
                    cell_minmax(v, cmin[j], cmax[j]);
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
            const uint64_t cell = (uint64_t)g * cpg;
#pragma unroll
            for (uint32_t j = 0; j < kAggMaxCols; j++) {
                if (j >= ncols) continue; /* uniform */
                AggCell c;
                if (FLOATS && slots[kGroupMaxBy + j].type >= kKeyFloat4) /* uniform */
                    float_cell(c.w, cn[j], cmin[j], cmax[j], (flags >> (3u * j)) & 7u, float_pair_of(ca[j], cb[j]));
                else c = cell_int(cn[j], cmin[j], cmax[j], ca[j], cb[j]);
                out_cell[cell + j] = c;
            }
            key_cells(cell + ncols, first);
        }
        n_groups += (uint32_t)__popcll(mh);
    }
    return n_groups;
}

/* A block kernel on GroupLds, all of it: the wave's block opened (scan_sweep.h), steps 1 to 3 with the block's rows of the side
 * area, and the block's two rows of `blocks`.  The arguments are the kernel's own; keys_of is group_matches' */
template <bool BYTES, bool FLOATS, bool LIKE = false, class KEYS = GroupRawKeys>
__device__ inline void group_block(GroupLds &L, uint32_t k, uint32_t lane, const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B,
                                   const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts,
                                   const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ slots, uint32_t nby,
                                   uint32_t ncols, uint32_t max_att, uint32_t side_stride, uint4 *__restrict__ blocks,
                                   GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell, const KEYS keys_of = KEYS())
{
    uint32_t n_match = 0, n_bad = 0;
    const uint8_t *__restrict__ p;
    uint32_t n, upper;
    const uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    group_matches<BYTES, FLOATS, LIKE>(L, p, B, n, upper, lane, atts, keys, nkeys, max_att, slots, nby, n_match, n_bad, keys_of);
    group_rank(L, n_match, lane);
    const uint32_t n_groups = group_reduce<FLOATS>(L, n_match, lane, slots, ncols, ncols, side_rec + (uint64_t)k * side_stride,
                                                   side_cell + (uint64_t)k * side_stride * ncols);
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n, n_match, n_bad);
        blocks[2u * k + 1u] = make_uint4(n_groups, 0u, 0u, 0u); /* first_group: k_group_offsets */
    }
}

/* ---- the host's side: the block-kernel launch of the grouped scan (scan_sweep.h: scan_block_launch), one per parameter list.
 * Behind the slots the kernels on GroupLds take nby, ncols, max_att, the bucket kernels the bucket table first, and the text
 * kernels, of one wave per workgroup, the text mask behind ncols; all end alike ---- */
struct GroupBucket; /* group_bucket.hip */
inline hipError_t group_launch(ScanKernel<const AggCol *, uint32_t, uint32_t, uint32_t, uint32_t, uint4 *, GroupRec *, AggCell *> kernel, bool table,
                               const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    return scan_block_launch(kernel, kGroupWaves, table, c, d, (const AggCol *)g.d_slots, g.nby, g.ncols, d.max_att,
                             filter_side_stride(c.block_size), g.d_blocks, (GroupRec *)g.d_side_rec, (AggCell *)g.d_side_cell);
}
inline hipError_t group_launch(ScanKernel<const AggCol *, const GroupBucket *, uint32_t, uint32_t, uint32_t, uint32_t, uint4 *, GroupRec *, AggCell *> kernel,
                               bool table, const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    return scan_block_launch(kernel, kGroupWaves, table, c, d, (const AggCol *)g.d_slots, (const GroupBucket *)d.d_buckets, g.nby, g.ncols, d.max_att,
                             filter_side_stride(c.block_size), g.d_blocks, (GroupRec *)g.d_side_rec, (AggCell *)g.d_side_cell);
}
inline hipError_t group_launch(ScanKernel<const AggCol *, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint4 *, GroupRec *, AggCell *> kernel,
                               bool table, const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    return scan_block_launch(kernel, 1u, table, c, d, (const AggCol *)g.d_slots, g.nby, g.ncols, d.text, d.max_att,
                             filter_side_stride(c.block_size), g.d_blocks, (GroupRec *)g.d_side_rec, (AggCell *)g.d_side_cell);
}
static_assert(kGroupMaxBy == CRYO_GROUP_MAX_BY && kAggMaxCols == CRYO_AGG_MAX_COLS, "group_launch_ok's limits (kernels.h) are the kernels'");

} // namespace cryo
