/*
 * recompress.h -- rewriting a cryo relation with another codec on the GPU: what relation_copy_for_cluster / VACUUM FULL would
 * call (the reference leaves both NOT_IMPLEMENTED, pg_cryogen.c:968-985, 1320, so a block keeps the codec it was written with
 * for good).
 *
 * The walk reads `src` in sequential-scan order as check.h does (cryo_stage_read_chain, continuation pages excluded from the
 * iterator) and collects the chains it meets into a window of at most CRYO_RECOMPRESS_WINDOW_BLOCKS chains or
 * CRYO_RECOMPRESS_WINDOW_BYTES compressed bytes.  A full window (and the last one) is handed to the codec's recode_blocks, ONE
 * call per source method present in it (cryo_multi_recode_blocks: the streams go up, are decoded, encoded again and packed on
 * the device, and only the new streams come back -- no uncompressed byte crosses PCIe), and then written into `dst` in the
 * order the walk met the chains: cryo_stage_write_chain on pages obtained through dst->ops->extend.  `dst` is a fresh relation
 * that already has its metapage (block 0).
 *
 * Every block written carries compression_method = the target method and the xid the read of its source reports: the
 * created_xid of its source first page (FrozenTransactionId where src's visibility map has the block all-frozen).
 * Nothing is lost silently:
 *   - a block whose chain reads but whose stream the decoders reject, or whose new stream fails write verification
 *     (pg_cryogen.gpu_verify_writes), is copied VERBATIM -- the same bytes under the same method field -- and reported with
 *     CRYO_CHECK_STREAM (offset 0xFFFFFFFF: rejected by the decoders; else the codec's status of the block as uint32);
 *   - a chain that cannot be read is reported with CRYO_CHECK_CHAIN and skipped, a first page with an unknown method with
 *     CRYO_CHECK_METHOD (offsets as in check.h); their pages are not copied.
 * The encode options are the backend's GUCs already set on the binding (segment size and strategy, verification, checksums).
 * It does not touch the decompressed-block cache or the device pool of `src`.  Not done here: the visibility map of `dst`,
 * writing a metapage, WAL beyond what dst->ops does per page, swapping the relations.
 */
#ifndef CRYO_RECOMPRESS_H
#define CRYO_RECOMPRESS_H

#include "check.h"

#define CRYO_RECOMPRESS_WINDOW_BLOCKS 4096
#define CRYO_RECOMPRESS_WINDOW_BYTES ((Size)256 << 20)
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_recompress_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

typedef struct {
    uint64 blocks;       /* chains the walk took for a block start: recoded + verbatim + skipped */
    uint64 recoded;      /* written with the target method */
    uint64 verbatim;     /* copied as they were (reported) */
    uint64 skipped;      /* unreadable chain or unknown method (reported, not copied) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 bytes_in;     /* compressed bytes of the chains read (recoded + verbatim) */
    uint64 bytes_out;    /* compressed bytes written to dst */
    uint64 pages_in;     /* pages of the chains read (recoded + verbatim) */
    uint64 pages_out;    /* pages written to dst */
    uint64 codec_calls;  /* recode_blocks calls */
} CryoRecompressTotals;

/* moved(arg, old_first, new_first, old_npages, new_npages): once per block written to dst, in the order written (TIDs carry
 * the first page's number: a caller rebuilding indexes needs this map).  report(arg, r): once per block not recoded, in walk
 * order, r->block a page of src.  Both may be NULL, as may totals.  Returns CRYO_OK, CRYO_E_ARG (an unknown target method),
 * CRYO_E_UNSUPPORTED when the bound codec has no recode_blocks (dst untouched), CRYO_E_NODEV when no codec can be bound,
 * CRYO_E_NOMEM, or the codec's error (the walk stops there; what was written and reported stands). */
int cryo_recompress_relation(CryoRel *src, CryoRel *dst, CompressionMethod method, int param,
                             void (*moved)(void *arg, BlockNumber old_first, BlockNumber new_first, uint32 old_npages,
                                           uint32 new_npages),
                             void (*report)(void *arg, const CryoCheckReport *r), void *arg, CryoRecompressTotals *totals);

#endif
