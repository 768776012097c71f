/*
 * group.h -- a sequential scan whose keys are tested and whose matches are grouped by one or two integer columns on the GPU, one
 * set of partial groups per block (include/cryo_codec.h, cryo_codec_group_batch: the rules of a block, of a tuple, of a key, of a
 * group and of a cell, and what is not supported).
 *
 * SELECT app_id, country, count(*), sum(revenue) FROM t WHERE ts >= a AND ts < b GROUP BY app_id, country through filter.h brings
 * every matching tuple back and leaves the grouping to the host.  The walk below is cryo_aggregate_scan's (aggregate.h) with
 * groups: the relation is read in sequential-scan order (scan_iterator.h), chains reassembled with cryo_stage_read_chain, the
 * readable ones batched by method in the aggregate's windows and handed to the codec's group_blocks; 32 bytes per block and 24 + 40
 * * ncols bytes per group and block come back.  It touches neither the decompressed-block cache nor the device pool.
 *
 * Visibility stays with the caller, and the block is the unit that makes that exact: a cryo block is written by one transaction,
 * so every block's groups come with its chain's created_xid (FrozenTransactionId for a frozen block) and the caller merges the
 * groups of the blocks its snapshot sees.
 *
 * The totals hold counters only -- there are no combined cells here, unlike CryoAggTotals: the same key may come back from
 * every block, so merging the groups across blocks needs a hash table on (key, nulls), and that is the caller's job (cells merge
 * as aggregate.h's do: n and the 128-bit sums added with carry, min and max over the cells with n > 0; n_rows are added).
 *
 * Where it does not pay: one block per call, and high cardinality -- a block of 290 distinct groups returns 64 + 40 * ncols bytes
 * per tuple, more than the filter returns for a narrow tuple.  More than two group columns, non-integer keys and HAVING go
 * through filter.h -- a text or bytea group column of short in-line values does not: CRYO_GROUP_TEXT (include/cryo_codec.h, "Text
 * group columns"; a block with n_bad > 0 holds values that are no key and is read again through filter.h).  An aggregate column may be a float column (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8): its cell is a cryo_agg_cell_f, and
 * the cells of one key from several blocks combine in block order with cryo_agg_cell_f_combine (aggregate.h).
 */
#ifndef CRYO_GROUP_H
#define CRYO_GROUP_H

#include "walk.h"
#include "cryo_codec.h"

/* one block's groups: recs n_groups records in the contract's order (ascending, NULLS LAST), cells n_groups * ncols cells (group
 * g's at g * ncols; NULL when ncols == 0); both valid during the callback only.  Under CRYO_GROUP_TEXT a group has ncols + ntext
 * cells (ntext: the group columns of type CRYO_KEY_BYTES): group g's aggregate cells at g * (ncols + ntext), and behind them, at
 * g * (ncols + ntext) + ncols, one cryo_group_key per text group column in column order, read through a cast -- the key's bytes
 * and its length, all zero for a NULL; cells is NULL when ncols + ntext == 0.  n_bad > 0: the block holds damaged items or --
 * under a byte-string key -- undecided ones, which are in no group -- cryo_filter_scan lists them */
typedef struct {
    BlockNumber block;
    TransactionId created_xid;
    uint32 n_items, n_match, n_bad, n_groups;
    const cryo_group_rec *recs;
    const cryo_agg_cell *cells;
} CryoGroupBlock;

/* reason and detail as CryoAggReport's */
typedef CryoWalkReport CryoGroupReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 items;        /* items of the blocks the codec looked into */
    uint64 matches;      /* tuples that passed every key */
    uint64 bad;          /* bad items (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE) and undecided ones (CRYO_FILTER_UNDECIDED) */
    uint64 reports;      /* reports made */
    uint64 codec_calls;  /* group_blocks calls */
    uint64 bytes_back;   /* what the calls brought back: rows, records and cells, a text group column's key cells included */
    uint64 groups;       /* per-block groups delivered (the same key counts once per block it occurs in) */
} CryoGroupTotals;

/* a window of the walk -- one codec call per method present -- is the aggregate's */
#define CRYO_GROUP_WINDOW_BLOCKS 4096
#define CRYO_GROUP_WINDOW_BYTES ((Size)256 << 20)
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_group_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Scans the relation (nblocks read once) with the descriptors *f, *grp and *agg (host arrays; agg may be NULL: no aggregate
 * column; include/cryo_codec.h).  Every block the codec could look into (status 0) is handed to block_cb(arg, b) in block order.
 * Every block it could not (STREAM, HEADER) and every chain that cannot be read is reported through report(arg, r) -- in the same
 * order, between the blocks -- and the walk goes on.  *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0),
 * CRYO_E_UNSUPPORTED when the bound codec has no group_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a null
 * relation or descriptor; descriptors the codec refuses), CRYO_E_NOMEM, or the codec's error (the walk stops there; what was
 * delivered stands). */
int cryo_group_scan(CryoRel *rel, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                    void (*block_cb)(void *arg, const CryoGroupBlock *b),
                    void (*report)(void *arg, const CryoGroupReport *r), void *arg, CryoGroupTotals *totals);

#endif
