/*
 * filter_walk.h -- the walk over one heap tuple that the scan filter (filter.hip), the scan aggregate (agg.hip), the grouped
 * scan (group.hip) and the projection (project.hip, eight capture slots) share: the TUPLE rule, the column walk and the key tests of include/cryo_codec.h ("filtering a scan"), and --
 * for the aggregate and the grouping -- the capture of column values as the walk passes them ("aggregating a scan", "grouping a
 * scan").  One statement of the walk: the filter instantiates it without capture, and the capture costs it nothing (the same
 * registers, no scratch).  The number of capture slots is a template parameter: four for the aggregate, six for the grouping (two
 * group columns and four aggregate columns).  Byte-string keys (CRYO_KEY_BYTES) are a second instantiation, chosen by the host when
 * a descriptor has one: a descriptor of integer keys and null tests alone runs the code it ran before those keys existed.  Set keys
 * (CRYO_OP_IN, CRYO_OP_NOT_IN) live in that second instantiation too: the host chooses it when a descriptor has either kind.
 * So does the truth table (CRYO_FILTER_TRUTH): the second instantiation keeps, per tuple, the mask of keys that are true and the
 * mask of keys that are undecided, and reads the verdict off a 16-bit table that rides in the high half of its nkeys argument --
 * the caller's under the flag, the AND table from the host otherwise, so that it has one verdict path.
 * Float keys (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8) are a further template parameter, FLOATS, of the walk: the kernels of float
 * descriptors (k_filterf_match, k_projectf_block, k_aggf_block, k_groupf_block) set it, every other instantiation is textually
 * what it was.  With it a loaded column value is mapped onto the signed integer whose order is the float order (float_map)
 * when the key's type is a float type; the host has mapped the key's constant the same way, so the compare is filter_compare's.
 * Pattern keys (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE) are the last parameter, LIKE: the kernels of descriptors with such a key set it
 * (k_filterl_match, k_aggl_block, k_groupl_block, k_groupbl_block, k_grouptl_block, k_projectl_block, k_topnl_block, each in a
 * unit of its own), and the walk then matches the noted payloads against the library's compiled patterns (walk_like).
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cryo {

constexpr uint32_t kFilterStream = 1, kFilterHeader = 2, kFilterItem = 3, kFilterOverlap = 7, kFilterTuple = 8; /* statuses */
constexpr uint32_t kFilterUndecided = 9;       /* a status too: a byte-string key met a value whose bytes are not in the tuple */
constexpr uint32_t kFilterNoMatch = 0xFFFFu;  /* inside the kernels only: a good tuple that fails a key */
constexpr uint32_t kKeyBytes = 16u;           /* CRYO_KEY_BYTES */
constexpr uint32_t kWalkNoBytes = 0xFFFFFFFFu; /* inside the walk only: the payload length of a varlena without in-line bytes */
constexpr int64_t kWalkTextAway = -1;           /* a TEXT capture: the varlena's bytes are not in the tuple (no place is negative) */
constexpr uint32_t kOpLt = 1, kOpLe = 2, kOpEq = 3, kOpGe = 4, kOpGt = 5, kOpNe = 6, kOpIsNull = 7, kOpNotNull = 8;
constexpr uint32_t kOpIn = 9, kOpNotIn = 10;  /* set keys: rsv the members, value their address in the key table */
constexpr uint32_t kOpLike = 11, kOpNotLike = 12; /* pattern keys: value the address of the compiled pattern in the key table */
constexpr uint32_t kLikeTextMax = 2048u;      /* CRYO_LIKE_TEXT_MAX: a longer payload leaves a pattern key undecided */
constexpr uint32_t kLikeNone = 0xFFFFFFFFu;   /* inside walk_like only: no position */
constexpr uint32_t kLikeUtf8 = 1u << 29, kLikeHead = 1u << 30, kLikeTail = 1u << 31; /* in a compiled pattern's segment word */
constexpr uint32_t kLikeAny = 0x100u;         /* a pattern element that is no literal byte: any one character */
constexpr uint32_t kSetLinear = 8u;           /* sets up to this size are scanned, larger ones searched; where the scan stops paying
                                                 is not measured: tools/set_key_cost.py reports both sides of this figure */
constexpr uint32_t kAggMaxCols = 4u;
constexpr uint32_t kKeyFloat4 = 8u, kKeyFloat8 = 9u; /* CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8 */
constexpr uint64_t kFloatNan = 0x7FF8000000000000ull; /* the canonical NaN a float cell reports */

struct FilterAtt { int16_t attlen; uint8_t attalign, rsv; };                           /* cryo_att */
struct FilterKey { uint16_t att; uint8_t type, op; uint32_t rsv; int64_t value; };    /* cryo_scan_key */
struct AggCol { uint16_t att; uint8_t type, rsv; uint32_t rsv2; };                     /* cryo_agg_col */
static_assert(sizeof(FilterAtt) == 4 && sizeof(FilterKey) == 16 && sizeof(AggCol) == 8, "the descriptor's layout is the header's");

/* what the walk captured of a tuple: v[j] the value of captured column j, valid when bit j of `has` is set (the column is not
 * NULL).  Only a tuple whose verdict is 0 has a capture worth reading.  SLOTS: how many columns a kernel captures at most. */
template <uint32_t SLOTS> struct WalkCaptureN { int64_t v[SLOTS]; uint32_t has; };
using WalkCapture = WalkCaptureN<kAggMaxCols>; /* the aggregate's */
template <class T> struct WalkPlain { using type = T; }; /* keeps SLOTS out of deduction: the filter passes a null capture */
template <bool BYTES> struct WalkKeys {};                /* a tag: whether the keys may hold a CRYO_KEY_BYTES entry or a set key */

/* what the walk notes of key k's test on a tuple: without BYTES the keys are ANDed into pass; with BYTES bit k of t says that
 * key k is true, and the truth table decides at the end */
template <bool BYTES> __device__ inline void walk_note(bool &pass, uint32_t &t, uint32_t k, bool hit)
{
    if (BYTES) t |= hit ? 1u << k : 0u;
    else pass = pass && hit;
}

__device__ inline bool filter_compare(uint32_t op, int64_t v, int64_t k)
{
    switch (op) {
    case kOpLt: return v < k;
    case kOpLe: return v <= k;
    case kOpEq: return v == k;
    case kOpGe: return v >= k;
    case kOpGt: return v > k;
    case kOpNe: return v != k;
    default: return false; /* the host lets no other op through */
    }
}

/* The bits of the IEEE double that equals the IEEE single of bits f, in integer arithmetic: exact for every value, a subnormal
 * included, whatever the wave's denormal mode; a NaN keeps its sign and its payload's high bits */
__device__ inline uint64_t float4_widen(uint32_t f)
{
    const uint64_t sign = (uint64_t)(f >> 31) << 63;
    uint32_t e = (f >> 23) & 0xFFu, m = f & 0x7FFFFFu;
    if (e == 255u) return sign | 0x7FF0000000000000ull | (uint64_t)m << 29;
    if (e == 0u) {
        if (m == 0u) return sign;
        const uint32_t sh = (uint32_t)__clz((int)m) - 8u; /* 1 .. 23: the leading one goes to bit 23 */
        m = (m << sh) & 0x7FFFFFu;
        return sign | (uint64_t)(897u - sh) << 52 | (uint64_t)m << 29; /* 2^(-126 - sh): 1023 - 126 - sh */
    }
    return sign | (uint64_t)(e + 896u) << 52 | (uint64_t)m << 29; /* 1023 - 127 */
}

/* The signed integer whose order is the float order of the double of bits b (PostgreSQL's float8_cmp_internal: -Inf < finite <
 * +Inf < NaN, all NaNs equal, -0 = +0): a NaN INT64_MAX, a zero 0, else b with its low 63 bits flipped when negative.  Its own
 * inverse apart from those two cases (float_unmap) */
__device__ inline int64_t float_map(uint64_t b)
{
    const uint64_t mag = b & 0x7FFFFFFFFFFFFFFFull;
    if (mag > 0x7FF0000000000000ull) return INT64_MAX;
    if (mag == 0u) return 0;
    return (int64_t)(b ^ ((uint64_t)((int64_t)b >> 63) & 0x7FFFFFFFFFFFFFFFull));
}

/* the double bits of a mapped value, canonical: the NaN kFloatNan, the zero +0 */
__device__ inline uint64_t float_unmap(int64_t m)
{
    if (m == INT64_MAX) return kFloatNan;
    return (uint64_t)m ^ ((uint64_t)(m >> 63) & 0x7FFFFFFFFFFFFFFFull);
}

/* the double bits of a column value as walk_value loaded it: a float4's 32 bits, sign-extended, are widened */
__device__ inline uint64_t float_bits(int64_t raw, bool is_float4)
{
    return is_float4 ? float4_widen((uint32_t)raw) : (uint64_t)raw;
}

/* the signed integer of attlen 2, 4 or 8 bytes at p, which is aligned to attlen */
__device__ inline int64_t walk_value(const uint8_t *__restrict__ p, int32_t attlen)
{
    if (attlen == 2) return *reinterpret_cast<const int16_t *>(p);
    if (attlen == 4) return *reinterpret_cast<const int32_t *>(p);
    return *reinterpret_cast<const int64_t *>(p);
}

/* the same with attlen 1 as well: the projection's load (project.hip), whose columns may be one byte wide.  A load of its own:
 * a fourth width in walk_value costs the aggregate's and the grouping's kernels two scalar registers each */
__device__ inline int64_t walk_value_narrow(const uint8_t *__restrict__ p, int32_t attlen)
{
    if (attlen == 1) return *reinterpret_cast<const int8_t *>(p);
    return walk_value(p, attlen);
}

/* A number with the sign of (payload, constant) in the order of the byte-string keys: memcmp over the shorter length on unsigned bytes, then the
 * lengths.  p: the plen payload bytes, anywhere; kc: the constant's n bytes, 8-byte aligned and zero-padded to a multiple of 8 (the
 * host's copy), read a word per trip at addresses that depend on the trip alone -- a uniform load -- and the trip count is n's.
 * The payload is read bytewise and never past plen: its pad up to MAXALIGN is not the column's.  A lane that is not `on`, whose
 * sign is known already, or -- by_len: the op is = or <> -- whose length differs from n loads nothing. */
__device__ inline int32_t walk_bytes_sign(const uint8_t *__restrict__ p, uint32_t plen, bool on, const uint64_t *__restrict__ kc,
                                          uint32_t n, bool by_len)
{
    uint32_t m = plen < n ? plen : n; /* the bytes memcmp looks at */
    if (!on || (by_len && plen != n)) m = 0;
    int32_t c = 0;
    for (uint32_t w = 0; w < n; w += 8u) {
        const uint64_t kw = kc[w >> 3]; /* uniform */
        if (c != 0 || w >= m) continue;
        const uint32_t r = m - w; /* 1 .. : the bytes of this word that count */
#pragma unroll
        for (uint32_t j = 0; j < 8u; j++) {
            if (j >= r) continue;
            const int32_t d = (int32_t)p[w + j] - (int32_t)((uint32_t)(kw >> (8u * j)) & 0xFFu);
            c = c != 0 ? c : d; /* the first byte that differs decides */
        }
    }
    if (c == 0) c = plen < n ? -1 : plen > n ? 1 : 0;
    return c;
}

/* Whether v is among the n >= 1 members at set: distinct, ascending as signed 64-bit integers, 8-byte aligned (the host's copy).
 * Up to kSetLinear members are read one per trip at addresses that depend on the trip alone -- uniform loads, as the byte-string
 * constant's words.  A larger set is searched: [lo, lo + len) always holds the last member <= v if there is one, lo + len <= n,
 * and a trip halves len (rounding up) with one 8-byte load per lane at lo + len / 2 < lo + len; after ceil(log2 n) trips len is 1
 * and set[lo] is that member or, when every member is above v, the first.  Either way the trip count is n's, the same in every
 * lane, every index is below n, and a lane that is not `on` loads nothing. */
__device__ inline bool walk_set_has(const int64_t *__restrict__ set, uint32_t n, int64_t v, bool on)
{
    if (n <= kSetLinear) { /* uniform */
        bool hit = false;
        for (uint32_t i = 0; i < n; i++) {
            const int64_t m = set[i]; /* uniform */
            hit = hit || m == v;
        }
        return on && hit;
    }
    uint32_t lo = 0;
    for (uint32_t len = n; len > 1u;) {
        const uint32_t half = len >> 1;
        if (on && set[lo + half] <= v) lo += half;
        len -= half;
    }
    return on && set[lo] == v;
}

/* One character on from s < plen in the plen bytes at p: one byte and every byte behind it whose top two bits are 10 under the mask cont --
 * 0xC0: the bytes 10xxxxxx, the UTF-8 rule; 0: none, a character is a byte.  Nothing at or past plen is read */
__device__ inline uint32_t like_next(const uint8_t *__restrict__ p, uint32_t plen, uint32_t s, uint32_t cont)
{
    s++;
    while (s < plen && (p[s] & cont) >> 6 == 2u) s++;
    return s;
}

/* Whether the plen payload bytes at p match the compiled pattern at prog (the host's copy, key_table_fill: 32-bit words, the
 * first 8-byte aligned).  A pattern is its segments -- the stretches between its unescaped '%' -- in order, then a word 0.  A
 * segment is one word and its elements: the word holds the element count ne in bits 0-15, the first element in bits 16-24,
 * kLikeUtf8 (the character rule), kLikeHead (the segment is matched at the payload's start and nowhere else) and kLikeTail (it
 * must end at the payload's end); the elements follow two a word, 16 bits each: a literal byte, or kLikeAny for any one
 * character.  '%' alone has no segment; the empty pattern has one without elements, head and tail.  Greedy by segments, no
 * backtracking: a head segment is matched at the payload's start; every other segment at its leftmost character start at or
 * after the end of the one before; a tail segment is searched the same way, and the start from which it ends exactly at plen is
 * the one accepted.  The segment and the element loops run on uniform counters and read the program with uniform loads; the
 * search for a start is per lane and runs while any lane still searches: at most plen + 1 starts a segment, so a wave does at
 * most (plen + 1) times the pattern's elements element steps whatever the data -- with kLikeTextMax the bound is 2 049 x 256.
 * The payload is read bytewise and never at or past plen; a lane that is not `on` or has failed loads nothing. */
__device__ inline bool walk_like(const uint8_t *__restrict__ p, uint32_t plen, bool on, const uint32_t *__restrict__ prog)
{
    uint32_t pos = on ? 0u : kLikeNone, w = 0; /* pos: where the segment before ended, kLikeNone in a lane that is out; w: the segment's word, uniform */
#pragma nounroll
    for (uint32_t sh = prog[0]; sh != 0u; sh = prog[w]) { /* uniform */
        const uint32_t ne = sh & 0xFFFFu, first = (sh >> 16) & 0x1FFu;
        const uint32_t cont = (sh & kLikeUtf8) ? 0xC0u : 0u, lit = (first & kLikeAny) ? 0u : 0xFFu; /* masks; 0: that test is off */
        uint32_t s = pos; /* the start this lane tries next; kLikeNone: it searches no more */
        pos = kLikeNone;  /* until a start matches */
        for (bool again = false; __ballot(s != kLikeNone) != 0; again = true) {
            if (again) { /* uniform.  On to the next character start, and to one whose byte can be the segment's first */
                while (s < plen) {
                    const uint32_t b = p[s];
                    if ((b & cont) >> 6 != 2u && (b & lit) == (first & lit)) break;
                    s++;
                }
            }
            if (s != kLikeNone && plen - s < ne) s = kLikeNone; /* s <= plen; an element takes a byte at least: no later start fits either */
            uint32_t q = s; /* kLikeNone: an element did not match */
#pragma nounroll
            for (uint32_t e = 0; e < ne; e++) {
                const uint32_t el = (prog[w + 1u + (e >> 1)] >> (16u * (e & 1u))) & 0xFFFFu; /* uniform */
                if (q >= plen) q = kLikeNone; /* kLikeNone is above every plen */
                else if (el & kLikeAny) q = like_next(p, plen, q, cont);
                else q = p[q] == el ? q + 1u : kLikeNone;
            }
            if (s == kLikeNone) continue;
            if (q != kLikeNone && (!(sh & kLikeTail) || q == plen)) { pos = q; s = kLikeNone; }
            else s = (sh & kLikeHead) || s >= plen ? kLikeNone : s + 1u;
        }
        w += 1u + ((ne + 1u) >> 1);
    }
    return pos != kLikeNone;
}

/* The verdict on one tuple of len bytes at t (8-byte aligned): 0 a match, kFilterNoMatch, kFilterTuple or -- BYTES alone --
 * kFilterUndecided.  `live` is false in
 * lanes without a tuple: they make the same trips and load nothing.  Invariant of the walk: hoff + o <= len.  CAPTURE: the walk
 * also notes the value of each of the ncols <= SLOTS columns cols[] names (their att <= max_att, attlen the type's size and
 * attalign at least that: the aggregate's argument rule; an att of 0 names no column) in *cap; cols is read at addresses that
 * depend on the loop counters only.  BYTES: a key of type kKeyBytes compares the column's in-line payload with the rsv bytes at
 * value (walk_bytes_sign), and a key of op kOpIn / kOpNotIn tests the column's value against the rsv sorted members at value
 * (walk_set_has); without BYTES no key has that type or those ops.  BYTES again: nkeys is the key count in its low half and the
 * truth table W in its high half (kernels.h, scan_nkeys_arg, packs them; bit m of W: a match when exactly the keys of mask m are true; monotone, the host's rule), and
 * the verdict on a good tuple with t the keys that are true and u those that are undecided is a match if W[t], no match if not
 * W[t | u], undecided otherwise; without BYTES nkeys is the count alone and the keys are ANDed.  NARROW: a captured column may have attlen 1 (the projection's
 * argument rule: attlen 1, 2, 4 or 8 and attalign at least that).  FLOATS (with BYTES alone): a comparison key of type kKeyFloat4 or
 * kKeyFloat8 holds its constant mapped (float_map, the host's rewrite) and the column's value is mapped before the compare;
 * a capture stays the raw bits.  TEXT (with BYTES alone; k_groupt_block's, group_text.hip): a captured column of type kKeyBytes is
 * a varlena, and its slot notes where the payload lies instead of a value: the payload's offset from t in the low half and its
 * length in the high half, or kWalkTextAway when the bytes are not in the tuple; the walk itself loads none of them.  LIKE (with
 * BYTES alone; the kernels of descriptors with a pattern key, k_filterl_match and its six siblings): a key of op kOpLike /
 * kOpNotLike matches the in-line payload of its column, of up to kLikeTextMax bytes, against the compiled pattern at value
 * (walk_like); an external, a compressed and a longer payload leave the key undecided, as a byte-string compare's.  The column
 * loop only notes where the payload lies; the match runs behind it, where the loop's scalar state is dead -- inside it the
 * matcher's own made the compiler spill.  Without LIKE no key has those ops, and every instantiation is textually what it was. */
template <bool CAPTURE, uint32_t SLOTS = kAggMaxCols, bool BYTES = false, bool NARROW = false, bool FLOATS = false, bool TEXT = false,
          bool LIKE = false>
__device__ inline uint32_t walk_tuple(const uint8_t *__restrict__ t, uint32_t len, bool live, const FilterAtt *__restrict__ atts,
                                      const FilterKey *__restrict__ keys, uint32_t nkeys, uint32_t max_att,
                                      const AggCol *__restrict__ cols, uint32_t ncols,
                                      typename WalkPlain<WalkCaptureN<SLOTS>>::type *cap, WalkKeys<BYTES> = WalkKeys<false>())
{
    uint32_t tnatts = 0, hoff = 0, tmask = 0, umask = 0; /* tmask, umask: BYTES alone */
    bool hasnull = false, bad = false, pass = true;
    const uint32_t truth = BYTES ? nkeys >> 16 : 0u; /* uniform */
    uint32_t like_at[4], like_len[4]; /* LIKE alone: where the payload of pattern key k lies from t, and its length or kLikeNone */
    if (LIKE) {
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) { like_at[j] = 0; like_len[j] = kLikeNone; }
    }
    if (BYTES) nkeys &= 0xFFFFu;
    if (live) {
        if (len < 23u) bad = true;
        else {
            tnatts = *reinterpret_cast<const uint16_t *>(t + 18) & 0x07FFu;
            hasnull = (*reinterpret_cast<const uint16_t *>(t + 20) & 1u) != 0;
            hoff = t[22];
            const uint32_t need = (23u + (hasnull ? (tnatts + 7u) >> 3 : 0u) + 7u) & ~7u;
            if ((hoff & 7u) != 0 || hoff < need || hoff > len) bad = true;
        }
    }
    uint32_t pos = hoff; /* hoff + o; alignment counts from hoff, a multiple of 8, so aligning pos aligns o */
    for (uint32_t col = 1; col <= max_att; col++) {
        const FilterAtt a = atts[col - 1u]; /* uniform */
        const uint32_t al = a.attalign - 1u;
        const bool on = live && !bad;
        bool isnull = true;
        if (on && col <= tnatts) /* the bitmap's byte lies below hoff: the TUPLE rule */
            isnull = hasnull && ((t[23u + ((col - 1u) >> 3)] >> ((col - 1u) & 7u)) & 1u) == 0;
        const bool here = on && !isnull;
        uint32_t size = 0, head = 0; /* head: the varlena's header bytes, kWalkNoBytes when its bytes are not in the tuple */
        if (a.attlen > 0) {
            if (here) {
                size = (uint32_t)a.attlen;
                pos = (pos + al) & ~al;
                if (pos > len || size > len - pos) bad = true;
            }
        } else if (here) {
            if (pos >= len) bad = true;
            else {
                if (t[pos] == 0) pos = (pos + al) & ~al; /* a pad byte: the header is aligned (att_align_pointer) */
                if (pos >= len) bad = true;
                else {
                    const uint32_t b = t[pos];
                    if (b == 1u) { /* external: 18 bytes when on-disk TOAST */
                        if (len - pos < 2u || t[pos + 1u] != 18u) bad = true;
                        else size = 18u;
                        if (BYTES) head = kWalkNoBytes;
                    } else if (b & 1u) {
                        size = b >> 1;
                        if (BYTES) head = 1u;
                    } else if (len - pos < 4u) bad = true;
                    else {
                        size = (b | (uint32_t)t[pos + 1u] << 8 | (uint32_t)t[pos + 2u] << 16 | (uint32_t)t[pos + 3u] << 24) >> 2;
                        if (size < 4u) bad = true;
                        if (BYTES) head = (b & 2u) ? kWalkNoBytes : 4u; /* bit 1 of an even header: compressed in line */
                    }
                    if (!bad && size > len - pos) bad = true;
                }
            }
        }
        const bool val = here && !bad;
        for (uint32_t k = 0; k < nkeys; k++) {
            const FilterKey key = keys[k]; /* uniform */
            if (key.att != col) continue;
            if (key.op == kOpIsNull) walk_note<BYTES>(pass, tmask, k, isnull);
            else if (key.op == kOpNotNull) walk_note<BYTES>(pass, tmask, k, !isnull);
            else if (LIKE && key.op >= kOpLike) { /* uniform.  The column is a varlena (the argument rule), as for a byte-string compare */
                const bool can = val && head != kWalkNoBytes && size - head <= kLikeTextMax;
                if (val && !can) umask |= 1u << k; /* external, compressed in line, or too long to search here */
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++) { /* unrolled: both stay in registers */
                    if (j != k) continue; /* uniform */
                    like_at[j] = pos + head;
                    like_len[j] = can ? size - head : kLikeNone;
                }
            } else if (BYTES && key.op >= kOpIn) {
                /* the column rule is the comparison key's: the same load.  Never undecided; false on a NULL column */
                const int64_t v = val ? walk_value(t + pos, a.attlen) : 0;
                const bool in = walk_set_has(reinterpret_cast<const int64_t *>(key.value), key.rsv, v, val);
                walk_note<BYTES>(pass, tmask, k, val && in == (key.op == kOpIn));
            } else if (BYTES && key.type == kKeyBytes) {
                /* the column is a varlena (the argument rule) and [pos, pos + size) lies below len */
                const bool inl = val && head != kWalkNoBytes;
                const int32_t c = walk_bytes_sign(t + pos + (inl ? head : 0u), inl ? size - head : 0u, inl,
                                                  reinterpret_cast<const uint64_t *>(key.value), key.rsv,
                                                  key.op == kOpEq || key.op == kOpNe);
                if (val && !inl) umask |= 1u << k; /* neither true nor false */
                else walk_note<BYTES>(pass, tmask, k, val && filter_compare(key.op, c, 0));
            } else {
                /* attlen is the key type's size and pos a multiple of it: the argument rule */
                int64_t v = val ? walk_value(t + pos, a.attlen) : 0;
                if (FLOATS && key.type >= kKeyFloat4 && key.type <= kKeyFloat8) /* uniform */
                    v = float_map(float_bits(v, key.type == kKeyFloat4));
                walk_note<BYTES>(pass, tmask, k, val && filter_compare(key.op, v, key.value));
            }
        }
        if (CAPTURE) {
#pragma unroll
            for (uint32_t j = 0; j < SLOTS; j++) { /* unrolled: v[j] stays in registers */
                if (j >= ncols || cols[j].att != col) continue; /* uniform */
                if (TEXT && cols[j].type == kKeyBytes) { /* uniform; [pos, pos + size) lies below len and head <= size */
                    cap->v[j] = !val ? 0 : head == kWalkNoBytes ? kWalkTextAway : (int64_t)((uint64_t)(pos + head) | (uint64_t)(size - head) << 32);
                    if (val) cap->has |= 1u << j;
                    continue;
                }
                /* as for a key: the column's [pos, pos + attlen) lies below len, aligned by the aggregate's argument rule */
                cap->v[j] = !val ? 0 : NARROW ? walk_value_narrow(t + pos, a.attlen) : walk_value(t + pos, a.attlen);
                if (val) cap->has |= 1u << j;
            }
        }
        if (val) pos += size;
    }
    if (LIKE) { /* the pattern keys, now that the walk's own state is done with: what they note is walk_note's */
        for (uint32_t k = 0; k < nkeys; k++) {
            const uint32_t op = keys[k].op; /* uniform */
            if (op < kOpLike) continue;
            uint32_t at = 0, plen = kLikeNone;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++)
                if (j == k) { at = like_at[j]; plen = like_len[j]; } /* uniform */
            const bool can = plen != kLikeNone; /* a good tuple, the column not NULL, its payload in the tuple and within the cap */
            const bool hit = walk_like(t + (can ? at : 0u), can ? plen : 0u, can, reinterpret_cast<const uint32_t *>(keys[k].value));
            if (can && hit == (op == kOpLike)) tmask |= 1u << k;
        }
    }
    if (BYTES) /* tmask and umask are below 16: both shifts stay within the table's 16 bits */
        return bad ? kFilterTuple : ((truth >> tmask) & 1u) ? 0u : ((truth >> (tmask | umask)) & 1u) ? kFilterUndecided : kFilterNoMatch;
    return bad ? kFilterTuple : !pass ? kFilterNoMatch : 0u;
}

} // namespace cryo
