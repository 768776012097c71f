/*
 * walk.h -- what the host walks share: reading and sorting a stored block, the sequential walk of a relation, and the window
 * that collects blocks for one codec call per method.
 *
 * cryo_check_relation (check.h) uses the relation walk and batches by itself; cryo_fetch_tuples (fetch.h) reads the pages it is
 * given and uses the window; cryo_recompress_relation, cryo_filter_scan, cryo_aggregate_scan, cryo_group_scan and
 * cryo_project_scan use both (cryo_walk_windowed).  What is left in their files is what is particular to each: its buffers, its
 * codec call, and how the rows that come back turn into callbacks and totals.
 */
#ifndef CRYO_WALK_H
#define CRYO_WALK_H

#include "check.h"

/* ---- a block, read and sorted ---- */

/* One chain as the walks see it.  Either its stream can go to a codec call (method COMP_LZ4 or COMP_ZSTD, comp and csize), or it
 * was not read (method -1) and reason, detail say why: CRYO_CHECK_CHAIN and the CryoError of cryo_stage_read_chain, or
 * CRYO_CHECK_METHOD and the method the first page names (that stream is dropped; csize keeps its length) */
typedef struct {
    BlockNumber block;     /* first page of the chain */
    uint32 npages;         /* pages of the chain that were read (a chain that broke off keeps the pages it did read) */
    TransactionId xid;     /* created_xid, or FrozenTransactionId for a frozen block */
    int method;
    char *comp;            /* malloc'd; its holder frees it */
    uint32 csize;
    uint32 reason, detail;
    size_t at;             /* its slot within the codec call of its method (cryo_window_gather) */
    const void *tag;       /* the caller's: cryo_fetch_tuples ties an entry to its CryoFetchPage */
} CryoWalkBlock;

/* pages the longest chain of a block can have: the scratch cryo_walk_read and cryo_stage_write_chain need */
uint32 cryo_walk_max_chain(void);

/* Reads the chain that starts at `block` into *b (the caller owns b->comp) and returns what cryo_stage_read_chain returned, so
 * that CRYO_ERR_EMPTY_BLOCK and CRYO_ERR_WRONG_STARTING_BLOCK stay the caller's to count.  chain[0 .. b->npages) are the pages. */
CryoError cryo_walk_read(CryoRel *rel, BlockNumber block, BlockNumber *chain, uint32 max_chain, CryoWalkBlock *b);

/* Walks the relation in sequential-scan order (scan_iterator.h; nblocks read once): new pages are counted in *empty_pages and
 * skipped, every other block start is counted in *blocks, its continuation pages leave the iterator, and it is handed to
 * visit(arg, b), which owns b->comp.  Stops at the first nonzero return and returns it; else CRYO_OK, or CRYO_E_NOMEM. */
typedef int (*CryoWalkVisit)(void *arg, CryoWalkBlock *b);
int cryo_walk_relation(CryoRel *rel, CryoWalkVisit visit, void *arg, uint64 *blocks, uint64 *empty_pages);

/* ---- the window ---- */

typedef struct {
    int blocks;            /* a window takes at most this many entries, */
    Size bytes;            /* or this many compressed bytes, whichever comes first */
} CryoWindowLimits;

typedef struct CryoWindow CryoWindow;
/* the window's codec calls and what follows from them, entries 0 .. n - 1 in order; the window is cleared after it, whatever
 * it returns */
typedef int (*CryoWindowFlush)(void *arg, CryoWindow *w);
struct CryoWindow {
    CryoWalkBlock *e;
    int n;
    Size bytes;            /* of the streams held */
    /* one codec call: the streams of one method */
    const void **src;
    uint32_t *src_size;
    CryoWindowLimits limits;
    CryoWindowFlush flush;
    void *arg;
};

/* CRYO_OK or CRYO_E_NOMEM; cryo_window_finish and cryo_window_free are safe after either */
int cryo_window_init(CryoWindow *w, CryoWindowLimits limits, CryoWindowFlush flush, void *arg);
/* Takes *b over.  A chain that was read and would take a window that is not empty past its byte limit flushes the window first
 * (so a single stream over the limit travels alone; the chain of an unknown method was read and is weighed like any other);
 * an entry that was not read takes a slot and adds no bytes; a window that holds limits.blocks entries is flushed.  After a
 * failed flush nothing more is flushed: *b is freed, the status returned. */
int cryo_window_add(CryoWindow *w, CryoWalkBlock *b);
/* the last flush, made only if rc is CRYO_OK; what is left is freed.  Returns rc, or the flush's status */
int cryo_window_finish(CryoWindow *w, int rc);
void cryo_window_free(CryoWindow *w);
/* the window's streams of `method` into src[] and src_size[], in entry order, each entry's slot into its `at`; returns how many */
size_t cryo_window_gather(CryoWindow *w, int method);

/* cryo_walk_relation into a window: init, an add per block, finish, free */
int cryo_walk_windowed(CryoRel *rel, CryoWindowLimits limits, CryoWindowFlush flush, void *arg, uint64 *blocks,
                       uint64 *empty_pages);

#ifdef CRYO_HOST_TEST_HOOKS
/* behind the cryo_*_set_window hooks: a value above 0 and below its maximum lowers that limit, any other restores it */
CryoWindowLimits cryo_window_limits(int blocks, Size bytes, int max_blocks, Size max_bytes);
#endif

/* ---- small parts ---- */

/* the report of the fetch and of the four scans (their headers name it CryoFetchReport, CryoFilterReport, ...) */
typedef struct {
    BlockNumber block;
    uint32 reason, detail;
} CryoWalkReport;
/* fills one and hands it to report, if there is one; counting it is the caller's */
void cryo_walk_say(void (*report)(void *, const CryoWalkReport *), void *arg, BlockNumber block, uint32 reason, uint32 detail);

/* a worst case as untouched virtual memory: only the used part is ever written.  NULL when it cannot be had; release takes NULL */
void *cryo_walk_reserve(size_t bytes);
void cryo_walk_release(void *p, size_t bytes);

#endif
