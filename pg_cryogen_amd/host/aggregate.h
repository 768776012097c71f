/*
 * aggregate.h -- a sequential scan whose keys are tested and whose integer columns are reduced on the GPU, one partial aggregate
 * per block (include/cryo_codec.h, cryo_codec_agg_batch: the rules of a block, of a tuple, of a key and of a cell, and what is not
 * supported).
 *
 * SELECT sum(x), min(ts), max(ts), count(x) FROM t WHERE ts >= a AND ts < b through filter.h brings every matching tuple back
 * and leaves the adding up to the host.  The walk below reads the relation as cryo_filter_scan does -- sequential-scan order
 * (scan_iterator.h), chains reassembled with cryo_stage_read_chain, the readable ones batched by method in the filter's windows --
 * hands them to the codec's agg_blocks and gets back 16 bytes per block and 40 bytes per block and aggregate column.  It touches
 * neither the decompressed-block cache nor the device pool.
 *
 * Visibility stays with the caller, and the block is the unit that makes that exact: a cryo block is written by one transaction,
 * so every block's partial comes with its chain's created_xid (FrozenTransactionId for a frozen block) and the caller adds up the
 * blocks its snapshot sees.  The totals' combined cells are the answer for a relation whose blocks are all visible.
 *
 * Where it does not pay: one block per call (a device round trip per block), and aggregates this codec does not reduce (float and
 * numeric columns, expressions) -- those go through filter.h.  GROUP BY on one or two integer columns is group.h's.
 */
#ifndef CRYO_AGGREGATE_H
#define CRYO_AGGREGATE_H

#include "check.h"
#include "cryo_codec.h"

/* one block's partial aggregate; cells: ncols cells in the order of the aggregate descriptor, valid during the callback only.
 * n_bad > 0: the block holds damaged items or -- under a byte-string key -- undecided ones, which are in no cell --
 * cryo_filter_scan lists them */
typedef struct {
    BlockNumber block;
    TransactionId created_xid;
    uint32 n_items, n_match, n_bad;
    const cryo_agg_cell *cells;
} CryoAggBlock;

/* reason: a block's status (CRYO_FETCH_STREAM, CRYO_FETCH_HEADER: detail 0) or one of check.h's host-side reasons
 * (CRYO_CHECK_CHAIN: detail = the CryoError of cryo_stage_read_chain; CRYO_CHECK_METHOD: detail = the method the first page
 * names) */
typedef struct {
    BlockNumber block;
    uint32 reason, detail;
} CryoAggReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 items;        /* items of the blocks the codec looked into */
    uint64 matches;      /* tuples that passed every key */
    uint64 bad;          /* bad items (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE) and undecided ones (CRYO_FILTER_UNDECIDED) */
    uint64 reports;      /* reports made */
    uint64 codec_calls;  /* agg_blocks calls */
    uint64 bytes_back;   /* what the calls brought back: rows and cells */
    /* the cells of all blocks with status 0 combined, whatever their xid: n and the 128-bit sums added (with carry), min and max
     * over the cells with n > 0 (0 when there is none); entries ncols .. 3 are zero */
    cryo_agg_cell cells[CRYO_AGG_MAX_COLS];
} CryoAggTotals;

/* a window of the walk -- one codec call per method present -- is the filter's: at most this many chains, or this many
 * compressed bytes, whichever comes first */
#define CRYO_AGG_WINDOW_BLOCKS 4096
#define CRYO_AGG_WINDOW_BYTES ((Size)256 << 20)
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_aggregate_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Scans the relation (nblocks read once) with the descriptors *f and *agg (host arrays; include/cryo_codec.h).  Every block the
 * codec could look into (status 0) is handed to block_cb(arg, b) in block order.  Every block it could not (STREAM, HEADER) and
 * every chain that cannot be read is reported through report(arg, r) -- in the same order, between the blocks -- and the walk
 * goes on.  *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0), CRYO_E_UNSUPPORTED when the bound codec has no
 * agg_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a null relation or descriptor; descriptors the codec refuses),
 * CRYO_E_NOMEM, or the codec's error (the walk stops there; what was delivered stands). */
int cryo_aggregate_scan(CryoRel *rel, const cryo_filter *f, const cryo_agg *agg,
                        void (*block_cb)(void *arg, const CryoAggBlock *b),
                        void (*report)(void *arg, const CryoAggReport *r), void *arg, CryoAggTotals *totals);

#endif
