/*
 * topn.h -- a sequential scan whose keys are tested, whose matches are ranked per block and whose SELECT list is picked on the GPU
 * (include/cryo_codec.h, cryo_codec_topn_batch: the rules of a block, of a tuple, of a key, of the order and of a row, and what is
 * not supported), and the merge that makes a query's answer of the blocks a snapshot sees.
 *
 * SELECT id, ts, revenue FROM t WHERE app_id IN (3, 17) AND ts >= a ORDER BY ts DESC LIMIT 100 through project.h brings every
 * match back and leaves the host to sort them.  The walk below is cryo_project_scan's (project.h) with an order: the relation is
 * read in sequential-scan order (scan_iterator.h), chains reassembled with cryo_stage_read_chain, the readable ones batched by
 * method in the filter's windows and handed to the codec's topn_blocks; 32 bytes per block and 24 + row_bytes bytes per KEPT row
 * come back, at most min(limit, 290) rows per block.  It touches neither the decompressed-block cache nor the device pool.
 * Visibility stays with the caller: a block is the unit of visibility, every block's kept rows come with its chain's created_xid
 * (FrozenTransactionId for a frozen block), nothing is filtered by it, and the caller adds the blocks its snapshot sees to a
 * CryoTopnMerge -- the first `limit` rows of every visible block, merged, are exactly the query's first `limit` rows.
 *
 * Where it does not pay: a limit near the matches a block has (every match comes back anyway, with 16 bytes more each than
 * through project.h), and one block per call.  Text, bytea or bucketed order columns, more than two order columns, WITH TIES and
 * DISTINCT ON go through project.h or filter.h; OFFSET is the caller's: it asks for LIMIT + OFFSET and drops the first rows.
 */
#ifndef CRYO_TOPN_H
#define CRYO_TOPN_H

#include "walk.h"
#include "cryo_codec.h"

/* a block's kept rows in rank order: rec[r] belongs to the row at rows + r * row_bytes (the layout of include/cryo_codec.h, at a
 * MAXALIGNed address); valid during the callback only.  n_bad > 0: bad or undecided items were in no ranking -- the call lists
 * none of them, the caller reads such a block through filter.h (the aggregate's rule) */
typedef struct {
    BlockNumber block;
    TransactionId created_xid;
    uint32 n_items, n_match, n_bad, n_rows;
    const cryo_topn_rec *rec;
    const char *rows;
    uint32 row_bytes;
} CryoTopnBlock;

/* reason and detail as CryoAggReport's: an unreadable chain, CRYO_FETCH_STREAM, CRYO_FETCH_HEADER */
typedef CryoWalkReport CryoTopnReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 items;        /* items of the blocks the codec looked into */
    uint64 matches;      /* tuples that passed every key, counted in full */
    uint64 bad;          /* bad items (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE) and undecided ones (CRYO_FILTER_UNDECIDED) */
    uint64 reports;      /* reports made */
    uint64 codec_calls;  /* topn_blocks calls */
    uint64 bytes_back;   /* what the calls brought back: the block table, records and rows */
    uint64 rows;         /* kept rows delivered */
} CryoTopnTotals;

/* a window of the walk -- one codec call per method present -- is the filter's (CRYO_FILTER_WINDOW_BLOCKS / _BYTES, filter.h) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_topn_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Scans the relation (nblocks read once) with the descriptors *f, *ord and *prj (host arrays; include/cryo_codec.h).  Every block
 * the codec looked into is delivered through block_cb(arg, b) in block order, with its kept rows.  Every bad block and every chain
 * that cannot be read is reported through report(arg, r) -- in the same order, between the blocks -- and the walk goes on.
 * *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0), CRYO_E_UNSUPPORTED when the bound codec has no
 * topn_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a null relation or descriptor; descriptors the codec
 * refuses), CRYO_E_NOMEM, or the codec's error (the walk stops there; what was delivered stands). */
int cryo_topn_scan(CryoRel *rel, const cryo_filter *f, const cryo_order *ord, const cryo_project *prj,
                   void (*block_cb)(void *arg, const CryoTopnBlock *b),
                   void (*report)(void *arg, const CryoTopnReport *r), void *arg, CryoTopnTotals *totals);

/* ---- the merge: the counterpart of cryo_agg_cell_f_combine for this call ----
 * Holds at most `limit` rows, ordered by the descriptor over the records' key / key_nulls: integer compares and the flags, nothing
 * else.  Ties across blocks go to the block added earlier, then to the block's own order, so the result does not depend on how the
 * relation was cut into windows.  `limit` is the query's (LIMIT + OFFSET) and may exceed 290. */
typedef struct {
    cryo_order_col by[CRYO_ORDER_MAX_BY];
    uint32 nby, limit, row_bytes;
    uint32 n;             /* rows held */
    cryo_topn_rec *rec;   /* n records in order */
    char *rows;           /* their rows */
} CryoTopnMerge;

/* CRYO_E_ARG: a null pointer, nby outside 1 .. 2, limit 0, an unknown flag, row_bytes 0 or no multiple of 8.  Only by[].flags of
 * the order are looked at */
int cryo_topn_merge_init(CryoTopnMerge *m, const cryo_order *ord, uint32 limit, uint32 row_bytes);
/* one block's n kept rows in the block's order (what block_cb got).  CRYO_E_NOMEM: *m is what it was */
int cryo_topn_merge_add(CryoTopnMerge *m, const cryo_topn_rec *rec, const void *rows, uint32 n);
/* the rows held, in order; *rec and *rows (either may be NULL) point into *m and hold until the next add or the free */
uint32 cryo_topn_merge_finish(const CryoTopnMerge *m, const cryo_topn_rec **rec, const void **rows);
void cryo_topn_merge_free(CryoTopnMerge *m);
/* the order of two records under the descriptor held in *m: below 0, 0, above 0 */
int cryo_topn_merge_compare(const CryoTopnMerge *m, const cryo_topn_rec *a, const cryo_topn_rec *b);

#endif
