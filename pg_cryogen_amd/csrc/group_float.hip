/*
 * group_float.hip -- the grouped scan's block kernel for descriptors with a float key or a float aggregate column
 * (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8; include/cryo_codec.h: "A float column's cell", "The reduction").  Every other descriptor runs
 * group.hip's k_group_block; k_group_offsets and k_group_copy serve both.
 *   k_groupf_block  k_group_block with the walk's FLOATS parameter set and the truth table's verdict path (the AND table from the
 *                   host when the caller gave none): the same LDS layout -- a captured value is its raw 64-bit word, a float4's
 *                   32 bits sign-extended --, the same steps 1 and 2 over the integer group columns (group_lds.h), the same side
 *                   area.  Only step 3 differs, per aggregate column by a uniform branch on its type: the head lane that walks
 *                   its run reduces an integer column as k_group_block does, cell byte for byte, and a float column into the
 *                   count, the minimum and maximum of the mapped values (float_map), three flag bits (+Inf, -Inf, NaN seen) and
 *                   the double-double pair over the finite values, started at (+0, +0) and taken in position order -- the order
 *                   the run has, equal keys lying in position order.
 *                   Step 3's frame -- the head's lane, its walk along the run, the record -- is stated in both kernels: what
 *                   differs sits in the innermost loop, and this kernel's run state (88 vector registers against 62) differs
 *                   throughout, so sharing the frame would take a callable for the column step.
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "float_pair.h"
#include "group_lds.h"

namespace cryo {

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
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t n_match = 0, n_bad = 0, n_groups = 0;
    const uint8_t *__restrict__ p;
    uint32_t n, upper;
    const uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    /* 1. the matches into LDS in position order, 2. their ranks: group_lds.h */
    group_matches<true, true>(L, p, B, n, upper, lane, atts, keys, nkeys, max_att, slots, nby, n_match, n_bad);
    const uint32_t m = n_match;
    group_rank(L, m, lane);
    /* 3. one lane per group: the head's lane walks the run up to the next head */
    GroupRec *out_rec = side_rec + (uint64_t)k * side_stride;
    AggCell *out_cell = side_cell + (uint64_t)k * side_stride * ncols;
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
#pragma unroll
            for (uint32_t j = 0; j < kAggMaxCols; j++) {
                if (j >= ncols) continue; /* uniform */
                AggCell c;
                if (slots[kGroupMaxBy + j].type >= kKeyFloat4) /* uniform */
                    float_cell(c.w, cn[j], cmin[j], cmax[j], (flags >> (3u * j)) & 7u, float_pair_of(ca[j], cb[j]));
                else c = cell_int(cn[j], cmin[j], cmax[j], ca[j], cb[j]);
                out_cell[(uint64_t)g * ncols + j] = c;
            }
        }
        n_groups += (uint32_t)__popcll(mh);
    }
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n, n_match, n_bad);
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
                       (AggCell *)d_side_cell);
    return hipGetLastError();
}

} // namespace cryo
