/* walk.c -- see walk.h */
#include "walk.h"
#include "cryo_codec.h"
#include "scan_iterator.h"

#include <string.h>
#include <sys/mman.h>

uint32 cryo_walk_max_chain(void)
{
    const Size ba = cryo_host_codec_bound(COMP_LZ4, cryo_blcksz), bb = cryo_host_codec_bound(COMP_ZSTD, cryo_blcksz);
    return (uint32)cryo_pages_needed(ba > bb ? ba : bb);
}

CryoError cryo_walk_read(CryoRel *rel, BlockNumber block, BlockNumber *chain, uint32 max_chain, CryoWalkBlock *b)
{
    char *comp = NULL;
    Size csize = 0;
    CompressionMethod sm = COMP_LZ4;
    TransactionId xid = 0;
    uint32 nb = 0;
    const CryoError err = cryo_stage_read_chain(rel, block, &comp, &csize, &sm, &xid, chain, max_chain, &nb);

    memset(b, 0, sizeof *b);
    b->block = block;
    b->npages = nb;
    b->xid = xid;
    b->method = -1;
    b->csize = (uint32)csize;
    if (err != CRYO_ERR_SUCCESS) {
        b->reason = CRYO_CHECK_CHAIN; b->detail = (uint32)err;
    } else if (sm != COMP_LZ4 && sm != COMP_ZSTD) {
        free(comp);
        b->reason = CRYO_CHECK_METHOD; b->detail = (uint32)sm;
    } else {
        b->method = (int)sm; b->comp = comp;
    }
    return err;
}

int cryo_walk_relation(CryoRel *rel, CryoWalkVisit visit, void *arg, uint64 *blocks, uint64 *empty_pages)
{
    const uint32 max_chain = cryo_walk_max_chain();
    const BlockNumber nblocks = rel->ops->nblocks(rel->handle);
    SeqScanIterator *iter = cryo_seqscan_iter_create();
    BlockNumber *chain = malloc((size_t)max_chain * sizeof *chain);
    int rc = iter && chain ? CRYO_OK : CRYO_E_NOMEM;

    while (rc == CRYO_OK) {
        const BlockNumber at = cryo_seqscan_iter_next(iter);
        CryoWalkBlock b;
        uint32 q;
        if (!BlockNumberIsValid(at) || at >= nblocks) break;
        if (cryo_walk_read(rel, at, chain, max_chain, &b) == CRYO_ERR_EMPTY_BLOCK) { (*empty_pages)++; continue; }
        (*blocks)++;
        /* the chain's continuation pages are not block starts (a chain that broke off keeps the pages it did read) */
        for (q = 1; q < b.npages; q++) cryo_seqscan_iter_exclude(iter, chain[q], true);
        rc = visit(arg, &b);
    }
    free(chain);
    if (iter) cryo_seqscan_iter_free(iter);
    return rc;
}

static void window_clear(CryoWindow *w)
{
    int i;
    for (i = 0; i < w->n; i++) free(w->e[i].comp);
    w->n = 0;
    w->bytes = 0;
}

static int window_flush(CryoWindow *w)
{
    const int rc = w->n ? w->flush(w->arg, w) : CRYO_OK;
    window_clear(w);
    return rc;
}

int cryo_window_init(CryoWindow *w, CryoWindowLimits limits, CryoWindowFlush flush, void *arg)
{
    memset(w, 0, sizeof *w);
    w->limits = limits;
    w->flush = flush;
    w->arg = arg;
    w->e = malloc((size_t)limits.blocks * sizeof *w->e);
    w->src = malloc((size_t)limits.blocks * sizeof *w->src);
    w->src_size = malloc((size_t)limits.blocks * sizeof *w->src_size);
    return w->e && w->src && w->src_size ? CRYO_OK : CRYO_E_NOMEM;
}

int cryo_window_add(CryoWindow *w, CryoWalkBlock *b)
{
    /* every chain that was read is weighed, the one of an unknown method too, which then adds nothing */
    int rc = b->csize && w->n > 0 && w->bytes + b->csize > w->limits.bytes ? window_flush(w) : CRYO_OK;
    if (rc != CRYO_OK) { free(b->comp); return rc; }
    w->e[w->n++] = *b;
    if (b->method >= 0) w->bytes += b->csize;
    if (w->n == w->limits.blocks) rc = window_flush(w);
    return rc;
}

int cryo_window_finish(CryoWindow *w, int rc)
{
    if (rc == CRYO_OK && w->e) rc = window_flush(w);
    if (w->e) window_clear(w);
    return rc;
}

void cryo_window_free(CryoWindow *w)
{
    free(w->e); free(w->src); free(w->src_size);
    memset(w, 0, sizeof *w);
}

size_t cryo_window_gather(CryoWindow *w, int method)
{
    size_t k = 0;
    int i;
    for (i = 0; i < w->n; i++) {
        CryoWalkBlock *e = &w->e[i];
        if (e->method != method) continue;
        w->src[k] = e->comp;
        w->src_size[k] = e->csize;
        e->at = k++;
    }
    return k;
}

static int add_visit(void *w, CryoWalkBlock *b) { return cryo_window_add(w, b); }

int cryo_walk_windowed(CryoRel *rel, CryoWindowLimits limits, CryoWindowFlush flush, void *arg, uint64 *blocks,
                       uint64 *empty_pages)
{
    CryoWindow w;
    int rc = cryo_window_init(&w, limits, flush, arg);
    if (rc == CRYO_OK) rc = cryo_walk_relation(rel, add_visit, &w, blocks, empty_pages);
    rc = cryo_window_finish(&w, rc);
    cryo_window_free(&w);
    return rc;
}

#ifdef CRYO_HOST_TEST_HOOKS
CryoWindowLimits cryo_window_limits(int blocks, Size bytes, int max_blocks, Size max_bytes)
{
    CryoWindowLimits l;
    l.blocks = blocks > 0 && blocks < max_blocks ? blocks : max_blocks;
    l.bytes = bytes > 0 && bytes < max_bytes ? bytes : max_bytes;
    return l;
}
#endif

void cryo_walk_say(void (*report)(void *, const CryoWalkReport *), void *arg, BlockNumber block, uint32 reason, uint32 detail)
{
    CryoWalkReport r;
    r.block = block;
    r.reason = reason;
    r.detail = detail;
    if (report) report(arg, &r);
}

void *cryo_walk_reserve(size_t bytes)
{
    void *p = mmap(NULL, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    return p == MAP_FAILED ? NULL : p;
}

void cryo_walk_release(void *p, size_t bytes)
{
    if (p) munmap(p, bytes);
}
