/* recompress.c -- see recompress.h */
#include "recompress.h"
#include "cryo_codec.h"
#include "walk.h"

#include <string.h>

static CryoWindowLimits window = {CRYO_RECOMPRESS_WINDOW_BLOCKS, CRYO_RECOMPRESS_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_recompress_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_RECOMPRESS_WINDOW_BLOCKS, CRYO_RECOMPRESS_WINDOW_BYTES);
}
#endif

/* what a codec call says of its stream k: status CRYO_OK = the new stream is out_size bytes at out_off of that call's area */
typedef struct {
    int32_t *status;
    uint32_t *out_size;
    uint64_t *out_off;
} Recoded;

typedef struct {
    const CryoCodecOps *ops;
    CryoRel *dst;
    CompressionMethod method;
    int param;
    void (*moved)(void *, BlockNumber, BlockNumber, uint32, uint32);
    void (*report)(void *, const CryoCheckReport *);
    void *arg;
    BlockNumber *chain;  /* of the chain being written */
    int max_chain;
    Size slot;           /* align16(bound of the target method) */
    Recoded out[2];      /* per source method, by the entry's slot in that call */
    CryoRecompressTotals t;
} Job;

static int write_block(Job *j, const CryoWalkBlock *e, CompressionMethod method, const char *bytes, Size size)
{
    const BlockNumber first = j->dst->ops->extend(j->dst->handle);
    int np = 0;
    if (cryo_stage_write_chain(j->dst, first, method, e->xid, bytes, size, j->chain, j->max_chain, &np) != 0) return CRYO_E_HIP;
    j->t.bytes_out += size;
    j->t.pages_out += (uint64)np;
    if (j->moved) j->moved(j->arg, e->block, first, e->npages, (uint32)np);
    return CRYO_OK;
}

static void say(Job *j, const CryoWalkBlock *e, uint32 reason, uint32 offset)
{
    CryoCheckReport r;
    r.block = e->block;
    r.reason = reason;
    r.offset = offset;
    r.npages = e->npages;
    if (j->report) j->report(j->arg, &r);
}

/* the window's codec calls (one per source method present), then its blocks into dst in walk order */
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    /* the worst case of the packed area, as untouched virtual memory: only the packed part is ever written.  A binding over G
     * GPUs cuts it into G regions of ceil(n / G) slots */
    const int gpus = cryo_gpu_count_guc < 1 ? 1 : (cryo_gpu_count_guc > 64 ? 64 : cryo_gpu_count_guc);
    const Size cap = ((Size)w->n + (Size)gpus) * j->slot;
    char *packed[2] = {NULL, NULL};
    int m, i, rc = CRYO_OK;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const Recoded *o = &j->out[m];
        const size_t k = cryo_window_gather(w, m);
        size_t s;
        if (k == 0) continue;
        packed[m] = cryo_walk_reserve(cap);
        if (!packed[m]) { rc = CRYO_E_NOMEM; break; }
        rc = j->ops->recode_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, (int)j->method, j->param, packed[m], cap,
                                   o->out_off, o->out_size, o->status);
        j->t.codec_calls++;
        for (s = 0; rc == CRYO_OK && s < k; s++)
            if (o->status[s] == CRYO_OK && (o->out_size[s] == 0 || o->out_off[s] + o->out_size[s] > cap)) rc = CRYO_E_HIP; /* not a packing */
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
        const Recoded *o;
        int32_t status;
        if (e->method < 0) {                       /* never read: reported and skipped */
            j->t.skipped++;
            say(j, e, e->reason, e->detail);
            continue;
        }
        j->t.bytes_in += e->csize;
        j->t.pages_in += e->npages;
        o = &j->out[e->method];
        status = o->status[e->at];
        if (status == CRYO_OK) {
            rc = write_block(j, e, j->method, packed[e->method] + o->out_off[e->at], o->out_size[e->at]);
            if (rc == CRYO_OK) j->t.recoded++;
        } else {                                   /* the decoders reject it, or it failed verification: as it was */
            rc = write_block(j, e, (CompressionMethod)e->method, e->comp, e->csize);
            if (rc == CRYO_OK) {
                j->t.verbatim++;
                say(j, e, CRYO_CHECK_STREAM, status == CRYO_E_CORRUPT ? 0xFFFFFFFFu : (uint32)status);
            }
        }
    }
    for (m = 0; m < 2; m++) cryo_walk_release(packed[m], cap);
    return rc;
}

int cryo_recompress_relation(CryoRel *src, CryoRel *dst, CompressionMethod method, int param,
                             void (*moved)(void *arg, BlockNumber old_first, BlockNumber new_first, uint32 old_npages,
                                           uint32 new_npages),
                             void (*report)(void *arg, const CryoCheckReport *r), void *arg, CryoRecompressTotals *totals)
{
    const CryoWindowLimits limits = window;
    const size_t W = (size_t)limits.blocks;
    Job j;
    int m, rc = CRYO_OK;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (method != COMP_LZ4 && method != COMP_ZSTD) return CRYO_E_ARG;
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    if (!j.ops->recode_blocks) return CRYO_E_UNSUPPORTED;
    j.dst = dst; j.method = method; j.param = param; j.moved = moved; j.report = report; j.arg = arg;
    j.max_chain = (int)cryo_walk_max_chain();
    j.slot = (cryo_host_codec_bound(method, cryo_blcksz) + 15) & ~(Size)15;
    j.chain = malloc((size_t)j.max_chain * sizeof *j.chain);
    if (!j.chain) rc = CRYO_E_NOMEM;
    for (m = 0; m < 2; m++) {
        j.out[m].status = malloc(W * sizeof *j.out[m].status);
        j.out[m].out_size = malloc(W * sizeof *j.out[m].out_size);
        j.out[m].out_off = malloc(W * sizeof *j.out[m].out_off);
        if (!j.out[m].status || !j.out[m].out_size || !j.out[m].out_off) rc = CRYO_E_NOMEM;
    }
    if (rc == CRYO_OK) rc = cryo_walk_windowed(src, limits, window_flush, &j, &j.t.blocks, &j.t.empty_pages);
    if (totals) *totals = j.t;
    for (m = 0; m < 2; m++) {
        free(j.out[m].status); free(j.out[m].out_size); free(j.out[m].out_off);
    }
    free(j.chain);
    return rc;
}
