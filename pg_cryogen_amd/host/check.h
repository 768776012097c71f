/*
 * check.h -- checking every stored block of a relation on the GPU (include/cryo_codec.h, cryo_codec_check_batch: the layout
 * rules of a decoded cryo block and what they do not see).
 *
 * The walk reads the relation in sequential-scan order (scan_iterator.h), reassembles each chain with cryo_stage_read_chain
 * and hands the readable ones, batched by method, to the codec's check_blocks: thousands of blocks per call, and only 8 bytes
 * per block come back.  Unlike a sequential scan, which stops with an ERROR at the first bad block, the walk goes on past every
 * bad block and reports each one.  It does not touch the decompressed-block cache or the device pool.
 */
#ifndef CRYO_CHECK_H
#define CRYO_CHECK_H

#include "staging.h"

/* reasons a report may carry: cryo_check_reason (CRYO_CHECK_STREAM .. CRYO_CHECK_NONZERO) and two found on the host */
enum {
    CRYO_CHECK_CHAIN = 16, /* the chain cannot be read: offset = the CryoError of cryo_stage_read_chain */
    CRYO_CHECK_METHOD = 17 /* the first page names a method that is neither LZ4 nor zstd: offset = that value */
};

typedef struct {
    BlockNumber block;   /* first page of the chain */
    uint32 reason, offset;
    uint32 npages;       /* pages of the chain the walk read */
} CryoCheckReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 bad;          /* reports */
    uint64 codec_calls;  /* check_blocks calls */
} CryoCheckTotals;

/* Walks the relation (nblocks read once), reports every bad block in ascending block order through report(arg, r), fills
 * *totals (may be NULL).  Returns CRYO_OK (0), CRYO_E_UNSUPPORTED when the bound codec has no check_blocks, CRYO_E_NODEV when
 * no codec can be bound, CRYO_E_NOMEM, or the codec's error (the walk stops there; what was reported stands). */
int cryo_check_relation(CryoRel *rel, void (*report)(void *arg, const CryoCheckReport *r), void *arg,
                        CryoCheckTotals *totals);

#endif
