/*
 * filter.h -- a sequential scan with scan keys evaluated on the GPU (include/cryo_codec.h, cryo_codec_filter_batch: the rules of
 * a block, of a tuple and of a key, and what is not supported).
 *
 * The reference accepts scan keys in cryo_beginscan and ignores them (pg_cryogen.c:185-211): every block is decoded in full on
 * the host side of PCIe and the executor drops the tuples that fail the qual.  The walk below reads the relation in
 * sequential-scan order (scan_iterator.h) as cryo_check_relation does, reassembles each chain with cryo_stage_read_chain, hands
 * the readable ones, batched by method, to the codec's filter_blocks -- thousands of blocks per call -- and gets back only the
 * tuples that pass the keys, 8 bytes per match and 32 bytes per block.  It touches neither the decompressed-block cache nor the
 * device pool.  Visibility stays with the caller: every tuple comes with its chain's created_xid (FrozenTransactionId for a
 * frozen block), nothing is filtered by it.
 *
 * Where it does not pay: wide rows at high selectivity (almost the whole block comes back, plus the records), and one block per
 * call (a device round trip per block; the host cache serves a second scan of a small relation for free).
 */
#ifndef CRYO_FILTER_H
#define CRYO_FILTER_H

#include <string.h>

#include "walk.h"
#include "cryo_codec.h"

/* data: the tuple's len bytes, zero up to MAXALIGN(len), at a MAXALIGNed address; valid during the callback only */
typedef struct {
    BlockNumber block;
    uint16 pos;
    TransactionId created_xid;
    const char *data;
    uint32 len;
} CryoFilteredTuple;

/* reason: a block's status (CRYO_FETCH_STREAM, CRYO_FETCH_HEADER, CRYO_FETCH_OVERLAP: detail 0), a bad item's
 * (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE, or CRYO_FILTER_UNDECIDED -- a byte-string key met a compressed or external value, the
 * caller fetches the tuple and rechecks it: detail = its position), or one of check.h's host-side reasons (CRYO_CHECK_CHAIN: detail =
 * the CryoError of cryo_stage_read_chain; CRYO_CHECK_METHOD: detail = the method the first page names) */
typedef CryoWalkReport CryoFilterReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 items;        /* items of the blocks the codec looked into */
    uint64 matches;      /* tuples that passed every key (delivered, unless CRYO_FILTER_COUNT_ONLY) */
    uint64 bad;          /* bad items (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE) and undecided ones (CRYO_FILTER_UNDECIDED) */
    uint64 reports;      /* reports made */
    uint64 codec_calls;  /* filter_blocks calls */
    uint64 bytes_back;   /* what the calls brought back: the block table, records and packed tuples */
} CryoFilterTotals;

/* a window of the walk -- one codec call per method present -- takes at most this many chains, or this many compressed bytes,
 * whichever comes first */
#define CRYO_FILTER_WINDOW_BLOCKS 4096
#define CRYO_FILTER_WINDOW_BYTES ((Size)256 << 20)
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_filter_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Scans the relation (nblocks read once) with the descriptor *f (host arrays; include/cryo_codec.h).  Matches are delivered
 * through tuple(arg, t) in block order, then position order.  Every bad block, every bad item and every chain that cannot be read
 * is reported through report(arg, r) -- in the same order, between the tuples -- and the walk goes on.  With
 * CRYO_FILTER_COUNT_ONLY in f->flags no tuple is delivered and bad items are counted, not reported one by one (count(*): the
 * totals carry items, matches and bad).  *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0),
 * CRYO_E_UNSUPPORTED when the bound codec has no filter_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a null
 * relation or descriptor; a descriptor the codec refuses), CRYO_E_NOMEM, or the codec's error (the walk stops there; what was
 * delivered stands). */
int cryo_filter_scan(CryoRel *rel, const cryo_filter *f,
                     void (*tuple)(void *arg, const CryoFilteredTuple *t),
                     void (*report)(void *arg, const CryoFilterReport *r), void *arg, CryoFilterTotals *totals);

/* The truth table of a WHERE clause in disjunctive normal form, for f->rsv under CRYO_FILTER_TRUTH (include/cryo_codec.h,
 * "Truth table"): terms[i] is a mask of the keys that are ANDed in term i (bit k: keys[k]) and the nterms terms are ORed --
 * A AND B AND (C OR D) over keys A, B, C, D is {0x7, 0xB}.  Bit m of the result is set when some term lies within m, so the
 * table is monotone by construction: binders build their tables here.  Returns 0 -- no table, the codec refuses it -- for no
 * term, a null array, an empty term, a term with a bit at or beyond nkeys, or nkeys outside 1 .. CRYO_FILTER_MAX_KEYS.  The four
 * walks (this one, aggregate.h, group.h, project.h) pass flags and rsv of the descriptor through untouched. */
/* A float key (include/cryo_codec.h, "Float keys"): column att of type CRYO_KEY_FLOAT4 or CRYO_KEY_FLOAT8 compared by op
 * (CRYO_OP_LT .. CRYO_OP_NE) with the double x -- a float4 constant widened by the caller's cast */
static inline cryo_scan_key cryo_filter_float_key(uint16_t att, uint8_t type, uint8_t op, double x)
{
    cryo_scan_key k = {att, type, op, 0, 0};
    memcpy(&k.value, &x, sizeof k.value);
    return k;
}

/* What the codec would hold against the n bytes at pattern as the pattern of a CRYO_OP_LIKE / CRYO_OP_NOT_LIKE key
 * (include/cryo_codec.h, "Pattern keys"), so that the binder raises PostgreSQL's own error, or keeps the qual to itself, before
 * any call: 0 -- nothing; CRYO_LIKE_CHECK_LENGTH -- n is above CRYO_KEY_BYTES_MAX, or n > 0 and pattern is null;
 * CRYO_LIKE_CHECK_ESCAPE -- the last byte is an unescaped '\' ("LIKE pattern must not end with escape character").  The
 * ESCAPE character has been rewritten to '\' by then.  In the header, as cryo_filter_truth_dnf is: a binder needs no codec for it. */
#define CRYO_LIKE_CHECK_LENGTH 1
#define CRYO_LIKE_CHECK_ESCAPE 2
static inline int cryo_filter_like_check(const void *pattern, uint32_t n)
{
    const uint8_t *p = (const uint8_t *)pattern;
    uint32_t i;
    if (n > CRYO_KEY_BYTES_MAX || (n > 0 && !p)) return CRYO_LIKE_CHECK_LENGTH;
    for (i = 0; i < n; i++)
        if (p[i] == '\\' && ++i == n) return CRYO_LIKE_CHECK_ESCAPE; /* the byte behind an escape is skipped, whatever it is */
    return 0;
}

static inline uint32_t cryo_filter_truth_dnf(const uint32_t *terms, uint32_t nterms, uint32_t nkeys)
{
    uint32_t w = 0, i, m;
    if (!terms || nterms == 0 || nkeys == 0 || nkeys > CRYO_FILTER_MAX_KEYS) return 0;
    for (i = 0; i < nterms; i++)
        if (terms[i] == 0 || (terms[i] >> nkeys) != 0) return 0;
    for (m = 0; m < (1u << nkeys); m++)
        for (i = 0; i < nterms; i++)
            if ((terms[i] & m) == terms[i]) w |= 1u << m;
    return w;
}

#endif
