/*
 * fetch.h -- fetching tuples of a relation by TID on the GPU (include/cryo_codec.h, cryo_codec_fetch_batch: the rules of a
 * request and what they do not check).
 *
 * A bitmap heap scan hands the access method one page of TIDs after the other (TBMIterateResult: a block number, ntuples
 * offsets, or ntuples < 0 for a lossy page, of which every tuple is wanted); the reference reads and decodes the whole block
 * for each (pg_cryogen.c:412-509).  The walk below takes the pages of a scan in one go: it reassembles each chain with
 * cryo_stage_read_chain, hands the readable ones, batched by method, to the codec's fetch_blocks -- thousands of blocks per
 * call -- and gets back only the tuples asked for and 16 bytes per request.  It touches neither the decompressed-block cache
 * nor the device pool.  Visibility stays with the caller: every tuple comes with its chain's created_xid (FrozenTransactionId
 * for a frozen block), nothing is filtered.
 *
 * Where it does not pay: a call for one TID is a whole device round trip for one tuple, and the host cache serves a second
 * fetch from the same block for free; a lossy page of wide rows returns almost the whole block.
 */
#ifndef CRYO_FETCH_H
#define CRYO_FETCH_H

#include "walk.h"

/* one page of a TID bitmap: TBMIterateResult's fields */
typedef struct {
    BlockNumber block;     /* first page of a chain, as a TID's block number is */
    int32_t ntuples;       /* -1: lossy, every tuple of the block */
    const uint16 *offsets; /* ntuples 1-based item positions, ascending and distinct */
} CryoFetchPage;

/* data: the tuple's len bytes, zero up to MAXALIGN(len), at a MAXALIGNed address; valid during the callback only */
typedef struct {
    BlockNumber block;
    uint16 pos;
    TransactionId created_xid;
    const char *data;
    uint32 len;
} CryoFetchedTuple;

/* reason: a cryo_fetch_status (detail: the position asked for; for CRYO_FETCH_STREAM, _HEADER and _BADREQ, which hold for the
 * whole block, one report per page with the first position asked for), or one of check.h's host-side reasons (CRYO_CHECK_CHAIN:
 * detail = the CryoError of cryo_stage_read_chain; CRYO_CHECK_METHOD: detail = the method the first page names) */
typedef CryoWalkReport CryoFetchReport;

typedef struct {
    uint64 pages;            /* pages handed in */
    uint64 not_block_starts; /* of them: not the first page of a chain, or new (empty) pages -- skipped, as a scan skips them */
    uint64 blocks;           /* chains sent to the codec */
    uint64 tuples;           /* tuples delivered */
    uint64 bad;              /* reports */
    uint64 codec_calls;      /* fetch_blocks calls */
    uint64 bytes_back;       /* what the calls brought back: packed tuples and 16 bytes per request */
} CryoFetchTotals;

/* a codec call per method takes at most this many chains, or this many compressed bytes, whichever comes first */
#define CRYO_FETCH_WINDOW_BLOCKS 4096
#define CRYO_FETCH_WINDOW_BYTES ((Size)256 << 20)
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_fetch_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Fetches the tuples the pages name.  Pages come in ascending block order, as a TID bitmap iterates; tuples are delivered
 * through tuple(arg, t) in page order, then position order.  A lossy page asks for positions 1 .. 290 and delivers up to the first
 * position the block does not have.  A page with ntuples == 0 is counted and nothing else.  A request the codec refuses and a
 * chain that cannot be read are reported through report(arg, r) -- in page order too, between the tuples -- and the walk goes
 * on.  *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0), CRYO_E_UNSUPPORTED when the bound codec has no
 * fetch_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a page with ntuples > 0 and no offsets), CRYO_E_NOMEM, or
 * the codec's error (the walk stops there; what was delivered stands). */
int cryo_fetch_tuples(CryoRel *rel, const CryoFetchPage *pages, size_t npages,
                      void (*tuple)(void *arg, const CryoFetchedTuple *t),
                      void (*report)(void *arg, const CryoFetchReport *r), void *arg, CryoFetchTotals *totals);

#endif
