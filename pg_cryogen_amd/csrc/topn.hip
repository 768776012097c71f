/*
 * topn.hip -- the device side of the ordered scan (cryo_codec_topn_batch / _blocks, include/cryo_codec.h: "ordering a scan").
 *
 * The host (cryo_codec.cpp, topn_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); these kernels look into every heap tuple of the decoded chunk as the projection does, rank each block's matches
 * by one or two order columns and let only the first `limit` of them leave the device, as the projection's row with a 24-byte
 * record that carries the compared keys:
 *   k_topn_block    one wave per block, two blocks per workgroup.  1. The sweep of scan_sweep.h, whose walk runs over the columns
 *                   1 .. max(highest key, projected, order column) with ten capture slots: the two order columns, then the eight
 *                   projected ones.  The wave ballots the turn's matches; a lane's rank among them, in position order, is where
 *                   its row goes in the block's share of a side area in handle workspace (the register assembly of
 *                   k_project_block, a copy: sharing it through a header would put project.hip's pinned resource figures at
 *                   risk) and where its two keys and its meta word go in LDS.  A key is the sign-extended value or, for a
 *                   float column, its float_map image, 0 when NULL; the meta word holds the position, the projected columns'
 *                   null bits and per order column a class (0 NULLs first, 1 a value, 2 NULLs last) that is compared before
 *                   the key.  2. The rank pass, in the manner of group_rank (group_lds.h): the place of a match is (matches
 *                   that sort before it) + (earlier matches that tie), m uniform LDS reads per lane and turn, no exchange, and
 *                   stable.  DESC is the bitwise complement of a key (~v reverses the signed order without overflow; -v does
 *                   not exist for INT64_MIN), applied to both sides of a compare by an exclusive or with a uniform mask.
 *                   3. Place s < min(limit, m) writes its record and the side-area index of its row; lane 0 the block row.
 *                   A descriptor with a byte-string key, a set key or a truth table runs k_topn_block<true>, one with a float
 *                   scan key k_topnf_block (the walk's FLOATS); a float ORDER column needs neither: it is mapped here, after
 *                   the capture.
 *   k_topn_offsets  one workgroup per chunk: the tiled scan of heap_block.h (offsets_of_rows, k_group_offsets' too) over n_rows,
 *                   from the running total the chunk before left in device memory; it writes row_first.
 *   k_topn_copy     a grid stride over the blocks: block k's records to row_first of the call's output, and its kept rows
 *                   gathered through the order list to the same places, 8 bytes per access, cut off at row_cap.
 * Every device write is a vector store in plain C++.  LDS: 24 bytes per possible match and wave.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "group_lds.h"

namespace cryo {

constexpr uint32_t kTopnMaxBy = 2u;   /* CRYO_ORDER_MAX_BY */
constexpr uint32_t kTopnMaxCols = 8u; /* CRYO_PROJECT_MAX_COLS */
constexpr uint32_t kTopnSlots = kTopnMaxBy + kTopnMaxCols; /* capture slots: the order columns, then the projected columns */
constexpr uint32_t kTopnWaves = 2u;   /* blocks per workgroup */
/* what the block kernel needs of the descriptors after the walk rides in two arguments, not in loads from the staged table that
 * the compiler would hoist over the item loop and keep in scalar registers the walk has none to spare of: ord_bits and row_map,
 * with the kOrd* bits, as topn_pack (kernels.h) packs them from the host's copy of the table */
static_assert(kTopnMaxBy == CRYO_ORDER_MAX_BY && kTopnMaxCols == CRYO_PROJECT_MAX_COLS, "topn_launch_ok's limits (kernels.h) are the kernels'");

struct TopnRec { int64_t key[2]; uint16_t pos, key_nulls; uint32_t nulls; }; /* cryo_topn_rec */
static_assert(sizeof(TopnRec) == 24 && sizeof(cryo_topn_rec) == 24, "the record's layout is the header's");

/* a wave's matches in LDS, in position order.  key: what the record reports (before the direction).  meta: bits 0 .. 8 the
 * position (1 .. 290), bits 9 .. 10 and 11 .. 12 the classes of order column 1 and 2, bits 16 .. 23 the projected columns' null
 * bits.  order[s]: the match at place s */
struct TopnLds {
    int64_t key[kTopnMaxBy][kHeapMaxItems];
    uint32_t meta[kHeapMaxItems];
    uint32_t order[kHeapMaxItems];
};
static_assert(sizeof(TopnLds) * kTopnWaves <= 32480u, "a workgroup's LDS stays within k_group_block's");

/* The staged table (TopnLaunch's rule, kernels.h): entries 0 .. 1 the order columns {att, type, flags, 0}, entries 2 .. 9 the projection's
 * column table {att, width, offset within the row, 0}; unused entries all zero.  The walk reads it as AggCol and looks at att */

template <bool BYTES, bool FLOATS, bool LIKE = false>
__device__ inline void topn_block_body(TopnLds &L, uint32_t k, uint32_t lane, const uint8_t *__restrict__ dec, uint64_t dec_stride,
                                       uint32_t B, const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts,
                                       const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ slots,
                                       uint32_t ord_bits, uint64_t row_map, uint32_t limit, uint32_t max_att, uint32_t row_words,
                                       uint32_t side_stride, uint4 *__restrict__ blocks, TopnRec *__restrict__ side_rec,
                                       uint2 *__restrict__ side_rows, uint32_t *__restrict__ side_ord)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t col_mask = (ord_bits >> 16) & 0xFFu;
    uint32_t n_match = 0, n_bad = 0;
    const uint8_t *__restrict__ p;
    uint32_t n, upper; /* lower <= B: n <= side_stride */
    const uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    uint2 *out_rows = side_rows + (uint64_t)k * side_stride * row_words;
    /* 1. rows to the side area and keys to LDS, both in position order */
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        const uint32_t i = t0 + lane;
        WalkCaptureN<kTopnSlots> cap;
        const SweepItem it = sweep_turn<true, kTopnSlots, BYTES, true, FLOATS, false, LIKE>(p, B, n, upper, i, atts, keys, nkeys, max_att,
                                                                                            slots, kTopnSlots, &cap);
        const unsigned long long mm = __ballot(it.match);
        /* no instruction: the three stay what they are, but the compiler may not know it, so that it keeps them alone over the
         * walk and not the several dozen compares and shifts it would derive from them once and for all turns */
        asm volatile("" : "+s"(ord_bits), "+s"(row_map), "+s"(row_words));
        if (it.match) {
            const uint32_t at = n_match + (uint32_t)__popcll(mm & below); /* below n <= side_stride <= 290 */
            uint32_t meta = (i + 1u) | ((~(cap.has >> kTopnMaxBy) & col_mask) << 16);
#pragma unroll
            for (uint32_t j = 0; j < kTopnMaxBy; j++) {
                const uint32_t ob = ord_bits >> (8u * j); /* uniform */
                const bool has = ((cap.has >> j) & 1u) != 0; /* never of a column the descriptor does not have: its att is 0 */
                int64_t v = cap.v[j];
                if (ob & kOrdFloat) /* uniform */
                    v = float_map(float_bits(v, (ob & kOrdFloat4) != 0u));
                L.key[j][at] = has ? v : 0;
                /* a column the descriptor does not have is one value: class 1, key 0 */
                const uint32_t cls = (has || !(ob & kOrdPresent)) ? 1u : (ob & kOrdNullsFirst) ? 0u : 2u;
                meta |= cls << (9u + 2u * j);
            }
            L.meta[at] = meta;
            /* the row in registers, as k_project_block's: a captured value is sign-extended and 0 when NULL, so its low w_j
             * bytes are the column's and shifting them to o_j touches no other column (o_j is a multiple of w_j) */
            uint64_t word[kTopnMaxCols];
#pragma unroll
            for (uint32_t q = 0; q < kTopnMaxCols; q++) word[q] = 0;
#pragma unroll
            for (uint32_t j = 0; j < kTopnMaxCols; j++) {
                /* uniform; a column the descriptor does not have captured 0 and places nothing */
                const uint32_t cm = (uint32_t)(row_map >> (8u * j)) & 0xFFu;
                const uint32_t w = 1u << (cm >> 6), o = cm & 63u;
                const int64_t cv = cap.v[kTopnMaxBy + j];
                const uint64_t bits = w >= 8u ? (uint64_t)cv : (uint64_t)cv & ((1ull << (8u * w)) - 1ull);
                const uint64_t placed = bits << (8u * (o & 7u));
#pragma unroll
                for (uint32_t q = 0; q < kTopnMaxCols; q++)
                    if ((o >> 3) == q) word[q] |= placed; /* uniform: the register is picked by a scalar compare */
            }
            uint2 *row = out_rows + (uint64_t)at * row_words;
            /* one scalar branch on the row's length, 1 .. 8 words, and the stores from the last word down */
#define CRYO_ROW_WORD(q) row[q] = make_uint2((uint32_t)word[q], (uint32_t)(word[q] >> 32))
            switch (row_words) {
            case 0: break;
            default: CRYO_ROW_WORD(7); [[fallthrough]];
            case 7: CRYO_ROW_WORD(6); [[fallthrough]];
            case 6: CRYO_ROW_WORD(5); [[fallthrough]];
            case 5: CRYO_ROW_WORD(4); [[fallthrough]];
            case 4: CRYO_ROW_WORD(3); [[fallthrough]];
            case 3: CRYO_ROW_WORD(2); [[fallthrough]];
            case 2: CRYO_ROW_WORD(1); [[fallthrough]];
            case 1: CRYO_ROW_WORD(0);
            }
#undef CRYO_ROW_WORD
        }
        n_match += (uint32_t)__popcll(mm);
        n_bad += (uint32_t)__popcll(__ballot(it.bad));
    }
    group_wave_sync();
    /* 2. the rank pass: (class 1, key 1, class 2, key 2) under the directions, ties by position */
    const uint32_t m = n_match;
    const int64_t d0 = (ord_bits & kOrdDesc) ? -1 : 0, d1 = ((ord_bits >> 8) & kOrdDesc) ? -1 : 0; /* uniform */
    for (uint32_t t0 = 0; t0 < m; t0 += 64u) {
        const uint32_t i = t0 + lane;
        const bool on = i < m;
        const uint32_t me = on ? i : 0u;
        const int64_t k0 = L.key[0][me] ^ d0, k1 = L.key[1][me] ^ d1;
        const uint32_t kc = (L.meta[me] >> 9) & 15u;
        uint32_t before = 0;
        for (uint32_t j = 0; j < m; j++) { /* uniform addresses: one LDS read serves the wave */
            const int64_t a0 = L.key[0][j] ^ d0, a1 = L.key[1][j] ^ d1;
            const uint32_t ac = (L.meta[j] >> 9) & 15u;
            const bool lt0 = (ac & 3u) != (kc & 3u) ? (ac & 3u) < (kc & 3u) : a0 < k0;
            const bool eq0 = (ac & 3u) == (kc & 3u) && a0 == k0;
            const bool lt1 = (ac >> 2) != (kc >> 2) ? (ac >> 2) < (kc >> 2) : a1 < k1;
            const bool eq1 = (ac >> 2) == (kc >> 2) && a1 == k1;
            before += (lt0 || (eq0 && (lt1 || (eq1 && j < i)))) ? 1u : 0u;
        }
        if (on) L.order[before] = i; /* a permutation of 0 .. m - 1 */
    }
    group_wave_sync();
    /* 3. the kept places: the record and the side-area index of the row */
    const uint32_t kept = m < limit ? m : limit;
    TopnRec *out_rec = side_rec + (uint64_t)k * side_stride;
    uint32_t *out_ord = side_ord + (uint64_t)k * side_stride;
    for (uint32_t t0 = 0; t0 < kept; t0 += 64u) {
        const uint32_t s = t0 + lane;
        if (s >= kept) continue;
        const uint32_t i = L.order[s], meta = L.meta[i];
        TopnRec rec;
        rec.key[0] = L.key[0][i];
        rec.key[1] = L.key[1][i];
        rec.pos = (uint16_t)(meta & 0x1FFu);
        rec.key_nulls = (uint16_t)((((meta >> 9) & 3u) != 1u ? 1u : 0u) | (((meta >> 11) & 3u) != 1u ? 2u : 0u));
        rec.nulls = (meta >> 16) & 0xFFu;
        out_rec[s] = rec;
        out_ord[s] = i;
    }
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n, n_match, n_bad);
        blocks[2u * k + 1u] = make_uint4(kept, 0u, 0u, 0u); /* row_first: k_topn_offsets */
    }
}

/* the host's side: the block-kernel launch of both units (scan_sweep.h: scan_block_launch), with the two packed arguments */
template <class K> inline hipError_t topn_launch(K kernel, bool table, const ScanChunk &c, const ScanDesc &d, const TopnLaunch &t)
{
    uint32_t ord_bits;
    uint64_t row_map;
    if (!topn_pack(t, ord_bits, row_map)) return hipErrorInvalidValue;
    return scan_block_launch(kernel, kTopnWaves, table, c, d, (const AggCol *)t.d_slots, ord_bits, row_map, t.limit, d.max_att, t.row_bytes / 8u,
                             filter_side_stride(c.block_size), t.d_blocks, (TopnRec *)t.d_side_rec, (uint2 *)t.d_side_rows,
                             (uint32_t *)t.d_side_ord);
}

#ifndef CRYO_LIKE_UNIT
template <bool BYTES>
__global__ void __launch_bounds__(64 * kTopnWaves)
k_topn_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
             const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ slots,
             uint32_t ord_bits, uint64_t row_map, uint32_t limit, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
             uint4 *__restrict__ blocks, TopnRec *__restrict__ side_rec, uint2 *__restrict__ side_rows, uint32_t *__restrict__ side_ord)
{
    __shared__ TopnLds lds[kTopnWaves];
    uint32_t k, lane;
    TopnLds &L = lds[sweep_wave(kTopnWaves, k, lane)];
    if (k >= cnt) return;
    topn_block_body<BYTES, false>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, ord_bits, row_map, limit, max_att,
                                  row_words, side_stride, blocks, side_rec, side_rows, side_ord);
}

/* k_topn_block<true> whose walk also maps the columns of float scan keys */
__global__ void __launch_bounds__(64 * kTopnWaves)
k_topnf_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
              const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ slots,
              uint32_t ord_bits, uint64_t row_map, uint32_t limit, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
              uint4 *__restrict__ blocks, TopnRec *__restrict__ side_rec, uint2 *__restrict__ side_rows, uint32_t *__restrict__ side_ord)
{
    __shared__ TopnLds lds[kTopnWaves];
    uint32_t k, lane;
    TopnLds &L = lds[sweep_wave(kTopnWaves, k, lane)];
    if (k >= cnt) return;
    topn_block_body<true, true>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, ord_bits, row_map, limit, max_att,
                                row_words, side_stride, blocks, side_rec, side_rows, side_ord);
}

/* row_first of every row of the chunk: the kept rows before block k, counted from the call's start; *running: the total before
 * the chunk in, after it out */
__global__ void __launch_bounds__(256)
k_topn_offsets(uint32_t cnt, uint64_t *__restrict__ running, uint4 *__restrict__ blocks)
{
    __shared__ uint64_t wave_sum[4];
    offsets_of_rows(cnt, running, blocks, wave_sum);
}

/* records (3 words each) of the chunk's blocks from the side area to their places within the call, and the kept rows (row_words
 * words each) gathered through the order list: row s of block k is the side area's row side_ord[s] */
__global__ void __launch_bounds__(256)
k_topn_copy(uint32_t cnt, uint32_t side_stride, uint32_t row_words, const uint4 *__restrict__ blocks,
            const uint64_t *__restrict__ side_rec, const uint2 *__restrict__ side_rows, const uint32_t *__restrict__ side_ord,
            uint64_t *__restrict__ rec, uint2 *__restrict__ rows, uint64_t row_cap)
{
    for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
        const uint4 place = blocks[2u * k + 1u];
        const uint64_t first = (uint64_t)place.z | (uint64_t)place.w << 32;
        uint32_t nrow = place.x < side_stride ? place.x : side_stride;
        if (first >= row_cap) continue;
        if (row_cap - first < nrow) nrow = (uint32_t)(row_cap - first); /* nothing at or beyond row_cap */
        const uint64_t *sr = side_rec + (uint64_t)k * side_stride * 3u;
        for (uint32_t w = threadIdx.x; w < nrow * 3u; w += 256u) rec[first * 3u + w] = sr[w];
        const uint2 *sw = side_rows + (uint64_t)k * side_stride * row_words;
        const uint32_t *so = side_ord + (uint64_t)k * side_stride;
        for (uint32_t w = threadIdx.x; w < nrow * row_words; w += 256u) {
            const uint32_t s = w / row_words, q = w - s * row_words;
            const uint32_t from = so[s];
            if (from < side_stride) rows[first * row_words + w] = sw[(uint64_t)from * row_words + q]; /* a match index: below m */
        }
    }
}

hipError_t launch_topn(const ScanChunk &c, const ScanDesc &d, const TopnLaunch &t)
{
    if (c.cnt == 0) return hipSuccess;
    if (!topn_launch_ok(c, d, t)) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    switch (scan_route(d.truth, d.floats, d.like)) {
    case kRouteLike: e = launch_topnl_block(c, d, t); break; /* a pattern key: the kernel of this source's second unit */
    case kRouteFloat: e = topn_launch(k_topnf_block, true, c, d, t); break;
    case kRouteTable: e = topn_launch(k_topn_block<true>, true, c, d, t); break;
    case kRoutePlain: e = topn_launch(k_topn_block<false>, false, c, d, t); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_topn_offsets, dim3(1), dim3(256), 0, c.stream, c.cnt, t.d_running, t.d_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_topn_copy, dim3(scan_copy_grid(c.cus, c.cnt)), dim3(256), 0, c.stream, c.cnt, filter_side_stride(c.block_size),
                       t.row_bytes / 8u, (const uint4 *)t.d_blocks, (const uint64_t *)t.d_side_rec, (const uint2 *)t.d_side_rows,
                       (const uint32_t *)t.d_side_ord, (uint64_t *)t.d_rec, (uint2 *)t.d_rows, t.row_cap);
    return hipGetLastError();
}

#else /* CRYO_LIKE_UNIT */
/* k_topnf_block whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like): a kernel of its own
 * name, as k_filterl_match is, built from this source compiled a second time with CRYO_LIKE_UNIT (topn_like.o): this unit
 * holds its three block kernels and no other */
__global__ void __launch_bounds__(64 * kTopnWaves)
k_topnl_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
              const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ slots,
              uint32_t ord_bits, uint64_t row_map, uint32_t limit, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
              uint4 *__restrict__ blocks, TopnRec *__restrict__ side_rec, uint2 *__restrict__ side_rows, uint32_t *__restrict__ side_ord)
{
    __shared__ TopnLds lds[kTopnWaves];
    uint32_t k, lane;
    TopnLds &L = lds[sweep_wave(kTopnWaves, k, lane)];
    if (k >= cnt) return;
    topn_block_body<true, true, true>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, ord_bits, row_map, limit,
                                      max_att, row_words, side_stride, blocks, side_rec, side_rows, side_ord);
}

hipError_t launch_topnl_block(const ScanChunk &c, const ScanDesc &d, const TopnLaunch &t) { return topn_launch(k_topnl_block, true, c, d, t); }
#endif

} // namespace cryo
