/*
 * group_text.hip -- the grouped scan's block kernels for descriptors with a byte-string group column (CRYO_GROUP_TEXT with a group
 * column of type CRYO_KEY_BYTES; include/cryo_codec.h: "Text group columns").  Every other descriptor runs group.hip's
 * k_group_block, group_float.hip's k_groupf_block or group_bucket.hip's k_groupb_block; k_group_offsets and k_group_copy serve all
 * four, with the cells of a group (the aggregate cells, then a key cell per text group column) where the others have ncols.
 *   k_groupt_block<FLOATS>  one wave per block and per workgroup (the wave's LDS is 34 800 bytes: GroupLds and four 64-bit words
 *                   per match and group column).  Always the walk instantiation that knows key tables and the truth table (the
 *                   AND table from the host when the caller gave none), with the walk's TEXT parameter: a text group column's
 *                   capture slot notes where the payload lies in the tuple, and the walk loads none of it.
 *                     1. the sweep; per turn a lane reads its match's payload bytewise, never past its length (at most
 *                        kTextMax bytes, inside the bytes the walk has proven to lie in the tuple), into four big-endian words,
 *                        zero-padded: unsigned word compares then give memcmp's order, and the length -- the column's key in
 *                        GroupLds, as the record reports it -- settles "ab" < "ab\0".  A match whose payload is not in line or
 *                        is longer than kTextMax becomes a bad item before the compaction, as an undecided bucket does.
 *                     2. group_rank's pass (group_lds.h) on the key (null, words .., length | integer value) per column:
 *                        uniform LDS reads of match j, a per-lane compare, less + same_before, heads marked.  An integer column
 *                        has no words: a uniform branch.
 *                     3. group_reduce (group_lds.h), every block kernel's, on the GroupLds inside and with the cells of a group
 *                        as its stride; behind a group's aggregate cells it calls GroupTextKeyCells, which writes one key cell
 *                        per text column in column order: the words back in memory order, the length, 0.  A NULL's words and
 *                        length are 0, so its cell is all zero.
 * Every device write is a vector store in plain C++.  No scratch, no global atomics.
 */
#include "kernels.h"
#include "group_lds.h"

namespace cryo {

constexpr uint32_t kTextMax = 32u;  /* CRYO_GROUP_TEXT_MAX */
constexpr uint32_t kTextWords = kTextMax / 8u;

struct GroupTextLds {
    GroupLds g;                                              /* key[j]: a text column's length */
    uint64_t word[kGroupMaxBy][kTextWords][kHeapMaxItems];   /* all zero for an integer column and for a NULL */
};
static_assert(sizeof(cryo_group_key) == sizeof(AggCell) && CRYO_GROUP_TEXT_MAX == kTextMax, "a key cell has a cell's room");
static_assert(sizeof(GroupTextLds) <= 65536u, "a workgroup's LDS stays within 64 KiB");

/* Step 1: group_matches with the text columns' bytes.  text: bit j set when group column j is a byte string */
template <bool FLOATS, bool LIKE>
__device__ inline void groupt_matches(GroupTextLds &L, const uint8_t *__restrict__ p, uint32_t B, uint32_t n, uint32_t upper, uint32_t lane,
                                      const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                                      uint32_t max_att, const AggCol *__restrict__ slots, uint32_t nby, uint32_t text, uint32_t &n_match,
                                      uint32_t &n_bad)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t by_mask = (1u << nby) - 1u;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        WalkCaptureN<kGroupSlots> cap;
        SweepItem it = sweep_turn<true, kGroupSlots, true, false, FLOATS, true, LIKE>(p, B, n, upper, t0 + lane, atts, keys, nkeys, max_att,
                                                                                      slots, kGroupSlots, &cap);
        /* what the slots of the text columns noted: a match whose payload is away or too long is undecided */
        uint32_t at[kGroupMaxBy], len[kGroupMaxBy];
        bool undecided = false;
#pragma unroll
        for (uint32_t j = 0; j < kGroupMaxBy; j++) {
            at[j] = len[j] = 0;
            if (((text >> j) & 1u) == 0) continue; /* uniform */
            const bool on = it.match && ((cap.has >> j) & 1u) != 0; /* a NULL stays the NULL group: no byte, length 0 */
            const int64_t note = cap.v[j];
            const uint32_t n_bytes = (uint32_t)((uint64_t)note >> 32);
            const bool inl = on && note != kWalkTextAway && n_bytes <= kTextMax;
            undecided = undecided || (on && !inl);
            at[j] = inl ? (uint32_t)note : 0u;
            len[j] = inl ? n_bytes : 0u;
            cap.v[j] = (int64_t)len[j];
        }
        if (undecided) {
            it.verdict = kFilterUndecided;
            it.match = false;
            it.bad = true;
        }
        const unsigned long long mm = __ballot(it.match);
        const uint32_t to = n_match + (uint32_t)__popcll(mm & below); /* a match's: below n <= 290 */
        if (it.match) {
#pragma unroll
            for (uint32_t j = 0; j < kGroupMaxBy; j++) L.g.key[j][to] = cap.v[j]; /* 0 when NULL or not a group column */
#pragma unroll
            for (uint32_t j = 0; j < kAggMaxCols; j++) L.g.val[j][to] = cap.v[kGroupMaxBy + j];
            L.g.meta[to] = (~cap.has & by_mask) | (cap.has & ~3u);
        }
        /* the payloads, a word per trip, straight to the match's place.  A match's tuple is good: the walk has seen
         * [at, at + len) lie inside it; every other lane has length 0 and loads nothing */
#pragma unroll
        for (uint32_t j = 0; j < kGroupMaxBy; j++) {
            if (((text >> j) & 1u) == 0) continue; /* uniform */
            const uint8_t *__restrict__ b = p + it.src + at[j];
            const uint32_t n_bytes = it.match ? len[j] : 0u;
#pragma unroll 1
            for (uint32_t q = 0; q < kTextWords; q++) {
                uint64_t x = 0;
#pragma unroll
                for (uint32_t r = 0; r < 8u; r++) {
                    const uint32_t i = 8u * q + r;
                    const uint32_t c = i < n_bytes ? b[i] : 0u;
                    x = x << 8 | c;
                }
                if (it.match) L.word[j][q][to] = x;
            }
        }
        n_match += (uint32_t)__popcll(mm);
        n_bad += (uint32_t)__popcll(__ballot(it.bad));
    }
    group_wave_sync();
}

/* one column's part of a compare: (a, k) are the column's words or its key; lt and eq carry the compare so far */
template <class T> __device__ inline void groupt_step(T a, T k, bool &lt, bool &eq)
{
    lt = lt || (eq && a < k);
    eq = eq && a == k;
}

/* Step 2: group_rank on keys with words.  The place of match i is (matches with a smaller key) + (earlier matches with an equal
 * key); a column's key is (null, word 0 .. 3 unsigned, key signed), NULL after every value, a NULL's words and key 0 */
__device__ inline void groupt_rank(GroupTextLds &L, uint32_t m, uint32_t lane, uint32_t text)
{
    for (uint32_t t0 = 0; t0 < m; t0 += 64u) {
        const uint32_t i = t0 + lane;
        const bool on = i < m;
        const uint32_t me = on ? i : 0u;
        int64_t kk[kGroupMaxBy];
        uint64_t kw[kGroupMaxBy][kTextWords];
#pragma unroll
        for (uint32_t c = 0; c < kGroupMaxBy; c++) {
            kk[c] = L.g.key[c][me];
#pragma unroll
            for (uint32_t q = 0; q < kTextWords; q++) kw[c][q] = ((text >> c) & 1u) ? L.word[c][q][me] : 0u;
        }
        const uint32_t kn = L.g.meta[me] & 3u;
        uint32_t less = 0, same_before = 0;
        for (uint32_t j = 0; j < m; j++) { /* uniform addresses: one LDS read serves the wave */
            const uint32_t an = L.g.meta[j] & 3u;
            bool lt = false, eq = true; /* over the columns so far */
#pragma unroll
            for (uint32_t c = 0; c < kGroupMaxBy; c++) {
                const uint32_t bit = 1u << c;
                bool clt = false, ceq = true;
                if ((text >> c) & 1u) { /* uniform */
#pragma unroll
                    for (uint32_t q = 0; q < kTextWords; q++) groupt_step<uint64_t>(L.word[c][q][j], kw[c][q], clt, ceq);
                }
                groupt_step<int64_t>(L.g.key[c][j], kk[c], clt, ceq);
                if ((an & bit) != (kn & bit)) { clt = (an & bit) == 0u; ceq = false; }
                lt = lt || (eq && clt);
                eq = eq && ceq;
            }
            less += lt ? 1u : 0u;
            same_before += (eq && j < i) ? 1u : 0u;
        }
        if (on) L.g.order[less + same_before] = i | (same_before == 0u ? 1u << 16 : 0u); /* a permutation of 0 .. m - 1 */
    }
    group_wave_sync();
}

/* bytes 0 .. 7 of a big-endian word back in memory order for a little-endian store */
__device__ inline uint64_t groupt_swap(uint64_t x) { return __builtin_bswap64(x); }

/* group_reduce's step for text group columns: behind a group's aggregate cells one key cell per text column in column order */
struct GroupTextKeyCells {
    const GroupTextLds &L;
    AggCell *__restrict__ out_cell;
    uint32_t text;
    __device__ void operator()(uint64_t cell, uint32_t first) const
    {
#pragma unroll
        for (uint32_t j = 0; j < kGroupMaxBy; j++) {
            if (((text >> j) & 1u) == 0) continue; /* uniform */
            AggCell c; /* cryo_group_key: bytes[32], len, rsv */
#pragma unroll
            for (uint32_t q = 0; q < kTextWords; q++) c.w[q] = groupt_swap(L.word[j][q][first]);
            c.w[4] = (uint64_t)(uint32_t)L.g.key[j][first];
            out_cell[cell] = c;
            cell++;
        }
    }
};

/* the body of k_groupt_block and -- LIKE -- of k_grouptl_block */
template <bool FLOATS, bool LIKE>
__device__ inline void groupt_block_body(GroupTextLds &L, uint32_t k, uint32_t lane, const uint8_t *__restrict__ dec, uint64_t dec_stride,
                                         uint32_t B, const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts,
                                         const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ slots, uint32_t nby,
                                         uint32_t ncols, uint32_t text, uint32_t max_att, uint32_t side_stride, uint4 *__restrict__ blocks,
                                         GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    uint32_t n_match = 0, n_bad = 0;
    const uint8_t *__restrict__ p;
    uint32_t n, upper;
    const uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    const uint32_t cpg = ncols + (uint32_t)__popc(text); /* a group's cells: the aggregate cells, then the key cells */
    /* 1. the matches and their text keys into LDS in position order, 2. their ranks, 3. group_reduce with the key cells */
    groupt_matches<FLOATS, LIKE>(L, p, B, n, upper, lane, atts, keys, nkeys, max_att, slots, nby, text, n_match, n_bad);
    groupt_rank(L, n_match, lane, text);
    AggCell *out_cell = side_cell + (uint64_t)k * side_stride * cpg;
    const uint32_t n_groups = group_reduce<FLOATS>(L.g, n_match, lane, slots, ncols, cpg, side_rec + (uint64_t)k * side_stride, out_cell,
                                                   GroupTextKeyCells{L, out_cell, text});
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n, n_match, n_bad);
        blocks[2u * k + 1u] = make_uint4(n_groups, 0u, 0u, 0u); /* first_group: k_group_offsets */
    }
}

#ifndef CRYO_LIKE_UNIT
template <bool FLOATS>
__global__ void __launch_bounds__(64)
k_groupt_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
               const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
               const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t text, uint32_t max_att,
               uint32_t side_stride, uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupTextLds lds[1];
    uint32_t k, lane;
    GroupTextLds &L = lds[sweep_wave(1u, k, lane)];
    if (k >= cnt) return;
    groupt_block_body<FLOATS, false>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, text, max_att,
                                     side_stride, blocks, side_rec, side_cell);
}

hipError_t launch_groupt_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    return group_launch(d.floats ? k_groupt_block<true> : k_groupt_block<false>, true, c, d, g);
}

#else /* CRYO_LIKE_UNIT */
/* k_groupt_block<true> whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like): a kernel of its
 * own name, so that k_groupt_block stays the code it was.  Built from this source compiled a second time with CRYO_LIKE_UNIT
 * (group_text_like.o) */
__global__ void __launch_bounds__(64)
k_grouptl_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
                const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                const AggCol *__restrict__ slots, uint32_t nby, uint32_t ncols, uint32_t text, uint32_t max_att,
                uint32_t side_stride, uint4 *__restrict__ blocks, GroupRec *__restrict__ side_rec, AggCell *__restrict__ side_cell)
{
    __shared__ GroupTextLds lds[1];
    uint32_t k, lane;
    GroupTextLds &L = lds[sweep_wave(1u, k, lane)];
    if (k >= cnt) return;
    groupt_block_body<true, true>(L, k, lane, dec, dec_stride, B, dec_status, atts, keys, nkeys, slots, nby, ncols, text, max_att,
                                  side_stride, blocks, side_rec, side_cell);
}

hipError_t launch_grouptl_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g) { return group_launch(k_grouptl_block, true, c, d, g); }
#endif

} // namespace cryo
