/*
 * group_bucket.hip -- the grouped scan's block kernels for descriptors whose group columns go through a bucket
 * (CRYO_GROUP_BUCKETS; include/cryo_codec.h: "Bucketed group columns").  Every other descriptor runs group.hip's k_group_block or
 * group_float.hip's k_groupf_block; k_group_offsets and k_group_copy serve all three.
 *   k_groupb_block<FLOATS>  k_group_block<true> (FLOATS false: integer cells alone) or k_groupf_block (FLOATS true: a float key or
 *                   a float aggregate column) with one more step.  The sweep and the capture are group_matches' (group_lds.h);
 *                   between a turn's capture and its compaction into LDS the step GroupBucketKeys maps each captured, non-NULL
 *                   group value to its bucket's key (bucket_key) and turns a match whose key is undecided into a bad item.  So
 *                   the match count, the compaction, the rank pass and the reduction run on bucket keys as they run on raw values,
 *                   and an undecided tuple is in n_bad, in no group and in no cell.  Always the walk instantiation that knows key
 *                   tables and the truth table (the AND table from the host when the caller gave none): two kernels, not four.
 *                   The body is group_block<true, FLOATS> (group_lds.h), the other two kernels' with the step handed on.
 * The bucket table (d_buckets): kGroupMaxBy entries of 24 bytes, cryo_bucket with -- for a list of boundaries -- n rewritten to the
 * number of distinct boundaries and value to the device address of the library's own copy: ascending as signed 64-bit integers,
 * duplicate-free, 8-byte aligned (cryo_codec.cpp, bucket_table_fill).  It is read at addresses that depend on loop counters only.
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "group_lds.h"

namespace cryo {

constexpr uint32_t kBucketNone = 0u, kBucketWidth = 1u; /* CRYO_BUCKET_NONE, _WIDTH; the third kind is CRYO_BUCKET_BOUNDS */
constexpr uint32_t kBucketInfinite = 1u;                /* CRYO_BUCKET_INFINITE */

struct GroupBucket { uint8_t kind, flags; uint16_t rsv; uint32_t n; int64_t origin, value; }; /* cryo_bucket, staged */
static_assert(sizeof(GroupBucket) == 24 && sizeof(cryo_bucket) == 24, "the bucket's layout is the header's");

/* o + w * floor((v - o) / w) for w >= 1 without wider arithmetic: the distance of v from o is exact in 64 unsigned bits on either
 * side of o, r is (v - o) mod w in [0, w), and the key v - r lies below INT64_MIN exactly when r exceeds v's distance from
 * INT64_MIN.  False: the key is not representable.  w is the same in all lanes; the division is the compiler's */
__device__ inline bool bucket_width(int64_t o, uint64_t w, int64_t v, int64_t &key)
{
    const bool up = v >= o;
    const uint64_t d = up ? (uint64_t)v - (uint64_t)o : (uint64_t)o - (uint64_t)v;
    const uint64_t m = d % w;
    const uint64_t r = up || m == 0u ? m : w - m;
    key = (int64_t)((uint64_t)v - r);
    return r <= (uint64_t)v - (uint64_t)INT64_MIN;
}

/* The greatest of the n >= 1 boundaries at set that is <= v: walk_set_has' search (filter_walk.h) with its last step turned from
 * "equal" into "not above".  Up to kSetLinear boundaries are read one per trip at addresses that depend on the trip alone; the
 * list ascends, so the last one not above v stays.  A longer list is searched: after ceil(log2 n) trips set[lo] is that boundary
 * or, when every boundary is above v, the first.  The trip count is n's, every index is below n, and a lane that is not `on`
 * loads nothing in the search.  False: v lies below every boundary */
__device__ inline bool bucket_bounds(const int64_t *__restrict__ set, uint32_t n, int64_t v, bool on, int64_t &key)
{
    if (n <= kSetLinear) { /* uniform */
        bool hit = false;
        for (uint32_t i = 0; i < n; i++) {
            const int64_t m = set[i]; /* uniform */
            if (m <= v) { key = m; hit = true; }
        }
        return hit;
    }
    uint32_t lo = 0;
    for (uint32_t len = n; len > 1u;) {
        const uint32_t half = len >> 1;
        if (on && set[lo + half] <= v) lo += half;
        len -= half;
    }
    const int64_t m = on ? set[lo] : 0;
    key = m;
    return m <= v;
}

/* The key of the non-NULL value v of a group column of integer type `type` under bucket b (kind not kBucketNone); false: it is
 * undecided.  Under kBucketInfinite the type's two extremes are their own buckets, and a key that equals an extreme without the
 * value being one is undecided.  Every branch on b and type is uniform */
__device__ inline bool bucket_key(const GroupBucket b, uint32_t type, int64_t v, bool on, int64_t &key)
{
    bool ok;
    key = v;
    if (b.kind == kBucketWidth) ok = bucket_width(b.origin, (uint64_t)b.value, v, key);
    else /* CRYO_BUCKET_BOUNDS: the host lets no other kind through */
        ok = bucket_bounds(reinterpret_cast<const int64_t *>(b.value), b.n, v, on, key);
    if (b.flags & kBucketInfinite) {
        const int64_t lo = type == 1u ? INT16_MIN : type == 2u ? INT32_MIN : INT64_MIN; /* CRYO_KEY_INT2, _INT4, _INT8 */
        const int64_t hi = type == 1u ? INT16_MAX : type == 2u ? INT32_MAX : INT64_MAX;
        if (v == lo || v == hi) { key = v; ok = true; }
        else if (key == lo || key == hi) ok = false;
    }
    return ok;
}

/* group_matches' step for bucketed group columns: slots[j] and bk[j] describe group column j < nby */
struct GroupBucketKeys {
    const GroupBucket *__restrict__ bk;
    const AggCol *__restrict__ slots;
    uint32_t nby;
    __device__ void operator()(WalkCaptureN<kGroupSlots> &cap, SweepItem &it) const
    {
        bool undecided = false;
#pragma unroll
        for (uint32_t j = 0; j < kGroupMaxBy; j++) {
            if (j >= nby) continue; /* uniform */
            const GroupBucket b = bk[j]; /* uniform */
            if (b.kind == kBucketNone) continue;
            const bool on = it.match && ((cap.has >> j) & 1u) != 0; /* a NULL stays the NULL group */
            int64_t key;
            const bool ok = bucket_key(b, slots[j].type, on ? cap.v[j] : 0, on, key);
            if (on) {
                cap.v[j] = key;
                undecided = undecided || !ok;
            }
        }
        if (undecided) {
            it.verdict = kFilterUndecided;
            it.match = false;
            it.bad = true;
        }
    }
};

#ifndef CRYO_LIKE_UNIT
template <bool FLOATS>
__global__ void __launch_bounds__(64 * kGroupWaves)
k_groupb_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
               const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
               const AggCol *__restrict__ slots, const GroupBucket *__restrict__ buckets, uint32_t nby, uint32_t ncols, uint32_t max_att,
               uint32_t side_stride, uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
    uint32_t k, lane;
    GroupLds &L = lds[sweep_wave(kGroupWaves, k, lane)];
    if (k >= cnt) return;
    /* the matches' group values mapped to bucket keys on their way into LDS */
    group_block<true, FLOATS>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, max_att, side_stride, blocks,
                              side_rec, side_cell, GroupBucketKeys{buckets, slots, nby});
}

hipError_t launch_groupb_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    return group_launch(d.floats ? k_groupb_block<true> : k_groupb_block<false>, true, c, d, g);
}

#else /* CRYO_LIKE_UNIT */
/* k_groupb_block<true> whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like): a kernel of its
 * own name, so that k_groupb_block stays the code it was.  Built from this source compiled a second time with CRYO_LIKE_UNIT
 * (group_bucket_like.o) */
__global__ void __launch_bounds__(64 * kGroupWaves)
k_groupbl_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
                const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                const AggCol *__restrict__ slots, const GroupBucket *__restrict__ buckets, uint32_t nby, uint32_t ncols, uint32_t max_att,
                uint32_t side_stride, uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
    uint32_t k, lane;
    GroupLds &L = lds[sweep_wave(kGroupWaves, k, lane)];
    if (k >= cnt) return;
    group_block<true, true, true>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, max_att, side_stride,
                                  blocks, side_rec, side_cell, GroupBucketKeys{buckets, slots, nby});
}

hipError_t launch_groupbl_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g) { return group_launch(k_groupbl_block, true, c, d, g); }
#endif

} // namespace cryo
