/* recompress.c -- see recompress.h */
#include "recompress.h"
#include "cryo_codec.h"
#include "scan_iterator.h"

#include <sys/mman.h>

typedef struct {
    BlockNumber block;   /* first page in src */
    uint32 npages;       /* pages of the chain the walk read */
    int method;          /* source method; -1: not read (reason, offset say why), skipped */
    TransactionId xid;
    char *comp;          /* the source stream */
    uint32 csize;
    uint32 reason, offset; /* of its report, when it is not recoded */
    /* from the codec call of its method: status CRYO_OK = its new stream is out_size bytes at out_off of that call's area */
    int32_t status;
    uint32_t out_size;
    uint64_t out_off;
} Entry;

typedef struct {
    Entry *e;
    int n;
    Size bytes;
    /* one codec call: the streams of one method, and where its results go */
    const void **src;
    uint32_t *src_size, *out_size;
    uint64_t *out_off;
    int32_t *status;
    int *at;             /* entry index of call slot k */
} Window;

typedef struct {
    CryoRel *dst;
    CompressionMethod method;
    int param;
    void (*moved)(void *, BlockNumber, BlockNumber, uint32, uint32);
    void (*report)(void *, const CryoCheckReport *);
    void *arg;
    BlockNumber *chain;
    int max_chain;
    Size slot;           /* align16(bound of the target method) */
    CryoRecompressTotals t;
} Job;

static void window_clear(Window *w)
{
    int i;
    for (i = 0; i < w->n; i++) free(w->e[i].comp);
    w->n = 0;
    w->bytes = 0;
}

static int write_block(Job *j, const Entry *e, CompressionMethod method, const char *bytes, Size size)
{
    const BlockNumber first = j->dst->ops->extend(j->dst->handle);
    int np = 0;
    if (cryo_stage_write_chain(j->dst, first, method, e->xid, bytes, size, j->chain, j->max_chain, &np) != 0) return CRYO_E_HIP;
    j->t.bytes_out += size;
    j->t.pages_out += (uint64)np;
    if (j->moved) j->moved(j->arg, e->block, first, e->npages, (uint32)np);
    return CRYO_OK;
}

static void say(Job *j, const Entry *e, uint32 reason, uint32 offset)
{
    CryoCheckReport r;
    r.block = e->block;
    r.reason = reason;
    r.offset = offset;
    r.npages = e->npages;
    if (j->report) j->report(j->arg, &r);
}

/* the window's codec calls (one per source method present), then its blocks into dst in walk order */
static int window_flush(const CryoCodecOps *ops, Job *j, Window *w)
{
    /* the worst case of the packed area, as untouched virtual memory: only the packed part is ever written.  A binding over G
     * GPUs cuts it into G regions of ceil(n / G) slots */
    const int gpus = cryo_gpu_count_guc < 1 ? 1 : (cryo_gpu_count_guc > 64 ? 64 : cryo_gpu_count_guc);
    const Size cap = ((Size)w->n + (Size)gpus) * j->slot;
    char *packed[2] = {NULL, NULL};
    int m, i, rc = CRYO_OK;

    if (w->n == 0) return CRYO_OK;
    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        int k = 0;
        for (i = 0; i < w->n; i++)
            if (w->e[i].method == m) {
                w->src[k] = w->e[i].comp;
                w->src_size[k] = w->e[i].csize;
                w->at[k] = i;
                k++;
            }
        if (k == 0) continue;
        packed[m] = mmap(NULL, cap, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (packed[m] == MAP_FAILED) { packed[m] = NULL; rc = CRYO_E_NOMEM; break; }
        rc = ops->recode_blocks(ops->ctx, m, w->src, w->src_size, (size_t)k, cryo_blcksz, (int)j->method, j->param, packed[m], cap,
                                w->out_off, w->out_size, w->status);
        j->t.codec_calls++;
        for (i = 0; rc == CRYO_OK && i < k; i++) {
            Entry *e = &w->e[w->at[i]];
            e->status = w->status[i];
            e->out_size = w->out_size[i];
            e->out_off = w->out_off[i];
            if (e->status == CRYO_OK && (e->out_size == 0 || e->out_off + e->out_size > cap)) rc = CRYO_E_HIP; /* not a packing */
        }
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        Entry *e = &w->e[i];
        if (e->method < 0) {                       /* never read: reported and skipped */
            j->t.skipped++;
            say(j, e, e->reason, e->offset);
            continue;
        }
        j->t.bytes_in += e->csize;
        j->t.pages_in += e->npages;
        if (e->status == CRYO_OK) {
            rc = write_block(j, e, j->method, packed[e->method] + e->out_off, e->out_size);
            if (rc == CRYO_OK) j->t.recoded++;
        } else {                                   /* the decoders reject it, or it failed verification: as it was */
            rc = write_block(j, e, (CompressionMethod)e->method, e->comp, e->csize);
            if (rc == CRYO_OK) {
                j->t.verbatim++;
                say(j, e, CRYO_CHECK_STREAM, e->status == CRYO_E_CORRUPT ? 0xFFFFFFFFu : (uint32)e->status);
            }
        }
    }
    for (m = 0; m < 2; m++)
        if (packed[m]) munmap(packed[m], cap);
    window_clear(w);
    return rc;
}

int cryo_recompress_relation(CryoRel *src, CryoRel *dst, CompressionMethod method, int param,
                             void (*moved)(void *arg, BlockNumber old_first, BlockNumber new_first, uint32 old_npages,
                                           uint32 new_npages),
                             void (*report)(void *arg, const CryoCheckReport *r), void *arg, CryoRecompressTotals *totals)
{
    const CryoCodecOps *ops;
    const Size ba = cryo_host_codec_bound(COMP_LZ4, cryo_blcksz), bb = cryo_host_codec_bound(COMP_ZSTD, cryo_blcksz);
    const uint32 max_chain = (uint32)cryo_pages_needed(ba > bb ? ba : bb);
    const int W = CRYO_RECOMPRESS_WINDOW_BLOCKS;
    BlockNumber nblocks;
    Job j;
    Window w;
    SeqScanIterator *iter = NULL;
    int rc = CRYO_OK;

    memset(&j, 0, sizeof j);
    memset(&w, 0, sizeof w);
    if (totals) *totals = j.t;
    if (method != COMP_LZ4 && method != COMP_ZSTD) return CRYO_E_ARG;
    ops = cryo_host_codec_ops();
    if (!ops) return CRYO_E_NODEV;
    if (!ops->recode_blocks) return CRYO_E_UNSUPPORTED;
    nblocks = src->ops->nblocks(src->handle);
    j.dst = dst; j.method = method; j.param = param; j.moved = moved; j.report = report; j.arg = arg;
    j.max_chain = (int)max_chain;
    j.slot = ((method == COMP_LZ4 ? ba : bb) + 15) & ~(Size)15;
    j.chain = malloc((size_t)max_chain * sizeof *j.chain);
    iter = cryo_seqscan_iter_create();
    w.e = malloc((size_t)W * sizeof *w.e);
    w.src = malloc((size_t)W * sizeof *w.src);
    w.src_size = malloc((size_t)W * sizeof *w.src_size);
    w.out_size = malloc((size_t)W * sizeof *w.out_size);
    w.out_off = malloc((size_t)W * sizeof *w.out_off);
    w.status = malloc((size_t)W * sizeof *w.status);
    w.at = malloc((size_t)W * sizeof *w.at);
    if (!j.chain || !iter || !w.e || !w.src || !w.src_size || !w.out_size || !w.out_off || !w.status || !w.at) rc = CRYO_E_NOMEM;

    while (rc == CRYO_OK) {
        const BlockNumber b = cryo_seqscan_iter_next(iter);
        char *comp = NULL;
        Size csize = 0;
        CompressionMethod sm = COMP_LZ4;
        TransactionId xid = 0;
        uint32 nb = 0, k;
        CryoError err;
        Entry *e;
        if (!BlockNumberIsValid(b) || b >= nblocks) break;
        err = cryo_stage_read_chain(src, b, &comp, &csize, &sm, &xid, j.chain, max_chain, &nb);
        if (err == CRYO_ERR_EMPTY_BLOCK) { j.t.empty_pages++; continue; }
        j.t.blocks++;
        /* the chain's continuation pages are not block starts (a chain that broke off keeps the pages it did read) */
        for (k = 1; k < nb; k++) cryo_seqscan_iter_exclude(iter, j.chain[k], true);
        if (err == CRYO_ERR_SUCCESS && w.n > 0 && w.bytes + csize > CRYO_RECOMPRESS_WINDOW_BYTES) rc = window_flush(ops, &j, &w);
        if (rc != CRYO_OK) { free(comp); break; }
        e = &w.e[w.n++];
        memset(e, 0, sizeof *e);
        e->block = b;
        e->npages = nb;
        e->xid = xid;
        if (err != CRYO_ERR_SUCCESS) {
            e->method = -1; e->reason = CRYO_CHECK_CHAIN; e->offset = (uint32)err;
        } else if (sm != COMP_LZ4 && sm != COMP_ZSTD) {
            free(comp);
            e->method = -1; e->reason = CRYO_CHECK_METHOD; e->offset = (uint32)sm;
        } else {
            e->method = (int)sm; e->comp = comp; e->csize = (uint32)csize;
            w.bytes += csize;
        }
        if (w.n == W) rc = window_flush(ops, &j, &w);
    }
    if (rc == CRYO_OK && w.e) rc = window_flush(ops, &j, &w);
    if (w.e) window_clear(&w);
    if (totals) *totals = j.t;
    free(w.e); free(w.src); free(w.src_size); free(w.out_size); free(w.out_off); free(w.status); free(w.at);
    free(j.chain);
    cryo_seqscan_iter_free(iter);
    return rc;
}
