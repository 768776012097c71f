/*
 * group_float.hip -- the grouped scan's block kernel for descriptors with a float key or a float aggregate column
 * (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8; include/cryo_codec.h: "A float column's cell", "The reduction").  Every other descriptor runs
 * group.hip's k_group_block; k_group_offsets and k_group_copy serve both.
 *   k_groupf_block  k_group_block with the walk's FLOATS parameter set and the truth table's verdict path (the AND table from the
 *                   host when the caller gave none): the same LDS layout -- a captured value is its raw 64-bit word, a float4's
 *                   32 bits sign-extended --, the same rank pass over the integer group columns, the same side area.  Only
 *                   step 3 differs, per aggregate column by a uniform branch on its type: the head lane that walks its run
 *                   reduces an integer column as k_group_block does, cell byte for byte, and a float column into the count, the
 *                   minimum and maximum of the mapped values (float_map), three flag bits (+Inf, -Inf, NaN seen) and the
 *                   double-double pair over the finite values, started at (+0, +0) and taken in position order -- the order the
 *                   run has, equal keys lying in position order.
 *                   The sweep and the rank pass are stated again here, not shared with k_group_block as a template: that kernel's
 *                   two instantiations stay the text and the registers they were, and this one's run state differs throughout.
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "float_pair.h"
#include "group_lds.h"

namespace cryo {

struct GroupWords { uint64_t w[5]; }; /* cryo_agg_cell and cryo_agg_cell_f alike */
static_assert(sizeof(GroupWords) == 40, "the cell's layout is the header's");

__global__ void __launch_bounds__(64 * kGroupWaves)
k_groupf_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
               const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
               const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t side_stride,
               uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, GroupWords *__restrict__ side_cell)
{
    __shared__ GroupLds lds[kGroupWaves];
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
                    walk_tuple<true, kGroupSlots, true, false, true>(p + src, len, live, atts, keys, nkeys, max_att, slots, kGroupSlots, &cap,
                                                                     WalkKeys<true>());
                if (live) verdict = walked;
                const bool match = verdict == 0u,
                           bad = verdict == kFilterItem || verdict == kFilterTuple || verdict == kFilterUndecided;
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
            GroupWords *out_cell = side_cell + (uint64_t)k * side_stride * ncols;
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
                            const uint32_t type = slots[kGroupMaxBy + j].type; /* uniform */
                            int64_t v = L.val[j][i];
                            cn[j]++;
                            if (type >= kKeyFloat4) {
                                /* the run's values in position order into the pair; what is not finite into the flags alone */
                                const uint64_t b = float_bits(v, type == kKeyFloat4);
                                const uint32_t f = float_flag(b);
                                v = float_map(b);
                                flags |= f << (3u * j);
                                if (f == 0u) {
                                    FloatPair x, y;
                                    x.hi = __longlong_as_double((long long)ca[j]);
                                    x.lo = __longlong_as_double((long long)cb[j]);
                                    y.hi = __longlong_as_double((long long)b);
                                    y.lo = 0.0;
                                    x = float_pair_add(x, y);
                                    ca[j] = (uint64_t)__double_as_longlong(x.hi);
                                    cb[j] = (uint64_t)__double_as_longlong(x.lo);
                                }
                            } else {
                                ca[j] += (uint64_t)v & 0xFFFFFFFFull;
                                cb[j] += (uint64_t)(v >> 32); /* arithmetic: v = (v >> 32) * 2^32 + (v & 0xFFFFFFFF) */
                            }
                            cmin[j] = v < cmin[j] ? v : cmin[j];
                            cmax[j] = v > cmax[j] ? v : cmax[j];
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
                        GroupWords c;
                        if (slots[kGroupMaxBy + j].type >= kKeyFloat4) { /* uniform */
                            FloatPair x;
                            x.hi = __longlong_as_double((long long)ca[j]);
                            x.lo = __longlong_as_double((long long)cb[j]);
                            float_cell(c.w, cn[j], cmin[j], cmax[j], (flags >> (3u * j)) & 7u, x);
                        } else {
                            /* sum = chi * 2^32 + clo as a 128-bit two's-complement number, as in agg.hip */
                            const int64_t chi = (int64_t)cb[j];
                            const uint64_t low = (uint64_t)chi << 32;
                            c.w[0] = cn[j];
                            c.w[1] = cn[j] ? (uint64_t)cmin[j] : 0u;
                            c.w[2] = cn[j] ? (uint64_t)cmax[j] : 0u;
                            c.w[3] = low + ca[j];
                            c.w[4] = (uint64_t)((chi >> 32) + (c.w[3] < low ? 1 : 0));
                        }
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

hipError_t launch_groupf_block(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                               const int32_t *d_dec_status, const void *d_atts, const void *d_keys, uint32_t nkeys, const void *d_slots,
                               uint32_t nby, uint32_t ncols, uint32_t max_att, uint32_t truth, uint32_t side_stride, uint4 *d_blocks,
                               void *d_side_rec, void *d_side_cell)
{
    /* the arguments are launch_group's, which checked them; the one verdict path needs a table */
    if (truth == 0u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_groupf_block, dim3((cnt + kGroupWaves - 1u) / kGroupWaves), dim3(64 * kGroupWaves), 0, s, d_dec, dec_stride,
                       block_size, cnt, d_dec_status, (const FilterAtt *)d_atts, (const FilterKey *)d_keys, nkeys | truth << 16,
                       (const AggCol *)d_slots, nby, ncols, max_att, side_stride, d_blocks, (GroupRec *)d_side_rec,
                       (GroupWords *)d_side_cell);
    return hipGetLastError();
}

} // namespace cryo
