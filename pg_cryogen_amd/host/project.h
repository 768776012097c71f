/*
 * project.h -- a sequential scan whose keys are tested and whose SELECT list is picked on the GPU (include/cryo_codec.h,
 * cryo_codec_project_batch: the rules of a block, of a tuple, of a key and of a row, and what is not supported).
 *
 * SELECT id, ts, revenue FROM t WHERE ts >= a AND ts < b through filter.h brings every matching tuple back whole and leaves the
 * host to deform it a second time.  The walk below is cryo_filter_scan's (filter.h) with rows: the relation is read in
 * sequential-scan order (scan_iterator.h), chains reassembled with cryo_stage_read_chain, the readable ones batched by method in
 * the filter's windows and handed to the codec's project_blocks; 32 bytes per block and 8 + row_bytes bytes per match come back,
 * whatever the tuple's width.  It touches neither the decompressed-block cache nor the device pool.  Visibility stays with the
 * caller: every row comes with its chain's created_xid (FrozenTransactionId for a frozen block), nothing is filtered by it.
 *
 * Where it does not pay: one block per call, and a SELECT list that names most of a narrow tuple (the row is then as long as
 * the tuple).  Varlena columns, fixed columns wider than 8 bytes (uuid, name), expressions and more than 8 columns go through
 * filter.h; there is no combined project-and-aggregate call.
 */
#ifndef CRYO_PROJECT_H
#define CRYO_PROJECT_H

#include "walk.h"
#include "cryo_codec.h"

/* data: the row's row_bytes bytes in the layout of include/cryo_codec.h (CRYO_PROJECT_COL_OFFSET / CRYO_PROJECT_ROW_BYTES), at a MAXALIGNed address;
 * bit j of nulls: projected column j is NULL (and zero in the row); valid during the callback only */
typedef struct {
    BlockNumber block;
    uint16 pos;
    TransactionId created_xid;
    uint32 nulls;
    const char *data;
    uint32 row_bytes;
} CryoProjectedRow;

/* reason and detail as CryoFilterReport's (OVERLAP does not occur) */
typedef CryoWalkReport CryoProjectReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 items;        /* items of the blocks the codec looked into */
    uint64 matches;      /* tuples that passed every key: rows delivered */
    uint64 bad;          /* bad items (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE) and undecided ones (CRYO_FILTER_UNDECIDED) */
    uint64 reports;      /* reports made */
    uint64 codec_calls;  /* project_blocks calls */
    uint64 bytes_back;   /* what the calls brought back: the block table, records and rows */
} CryoProjectTotals;

/* a window of the walk -- one codec call per method present -- is the filter's (CRYO_FILTER_WINDOW_BLOCKS / _BYTES, filter.h) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_project_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Scans the relation (nblocks read once) with the descriptors *f and *prj (host arrays; include/cryo_codec.h).  The rows of the
 * matches are delivered through row_cb(arg, r) in block order, then position order.  Every bad block, every bad item and every
 * chain that cannot be read is reported through report(arg, r) -- in the same order, between the rows -- and the walk goes on.
 * *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0), CRYO_E_UNSUPPORTED when the bound codec has no
 * project_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a null relation or descriptor; descriptors the codec
 * refuses), CRYO_E_NOMEM, or the codec's error (the walk stops there; what was delivered stands). */
int cryo_project_scan(CryoRel *rel, const cryo_filter *f, const cryo_project *prj,
                      void (*row_cb)(void *arg, const CryoProjectedRow *r),
                      void (*report)(void *arg, const CryoProjectReport *r), void *arg, CryoProjectTotals *totals);

#endif
