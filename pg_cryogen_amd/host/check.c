/* check.c -- see check.h */
#include "check.h"
#include "cryo_codec.h"
#include "scan_iterator.h"

/* a codec call per method takes at most this many blocks, or this many compressed bytes, whichever comes first */
#define CHECK_BATCH_BLOCKS 4096
#define CHECK_BATCH_BYTES ((Size)256 << 20)

typedef struct {
    char **comp;
    uint32_t *size;
    BlockNumber *block;
    uint32 *npages;
    int n;
    Size bytes;
} CheckBatch;

typedef struct {
    CryoCheckReport *r;
    size_t n, cap;
} ReportList;

static int add_report(ReportList *l, BlockNumber block, uint32 reason, uint32 offset, uint32 npages)
{
    if (l->n == l->cap) {
        const size_t cap = l->cap ? l->cap * 2 : 64;
        CryoCheckReport *r = realloc(l->r, cap * sizeof *r);
        if (!r) return CRYO_E_NOMEM;
        l->r = r;
        l->cap = cap;
    }
    l->r[l->n].block = block;
    l->r[l->n].reason = reason;
    l->r[l->n].offset = offset;
    l->r[l->n].npages = npages;
    l->n++;
    return CRYO_OK;
}

static int cmp_report(const void *a, const void *b)
{
    const BlockNumber x = ((const CryoCheckReport *)a)->block, y = ((const CryoCheckReport *)b)->block;
    return x < y ? -1 : x > y;
}

static void batch_clear(CheckBatch *b)
{
    int i;
    for (i = 0; i < b->n; i++) free(b->comp[i]);
    b->n = 0;
    b->bytes = 0;
}

/* one codec call over the batch; its bad blocks go to the list */
static int batch_flush(const CryoCodecOps *ops, int method, CheckBatch *b, uint32_t *res, ReportList *l, CryoCheckTotals *t)
{
    int i, rc;
    if (b->n == 0) return CRYO_OK;
    rc = ops->check_blocks(ops->ctx, method, (const void *const *)b->comp, b->size, (size_t)b->n, cryo_blcksz, res);
    t->codec_calls++;
    for (i = 0; rc == CRYO_OK && i < b->n; i++)
        if (res[2 * i] != CRYO_CHECK_OK) rc = add_report(l, b->block[i], res[2 * i], res[2 * i + 1], b->npages[i]);
    batch_clear(b);
    return rc;
}

int cryo_check_relation(CryoRel *rel, void (*report)(void *arg, const CryoCheckReport *r), void *arg,
                        CryoCheckTotals *totals)
{
    const CryoCodecOps *ops = cryo_host_codec_ops();
    const Size ba = cryo_host_codec_bound(COMP_LZ4, cryo_blcksz), bb = cryo_host_codec_bound(COMP_ZSTD, cryo_blcksz);
    const uint32 max_chain = (uint32)cryo_pages_needed(ba > bb ? ba : bb);
    const BlockNumber nblocks = rel->ops->nblocks(rel->handle);
    CryoCheckTotals t = {0, 0, 0, 0};
    CheckBatch batch[2];
    ReportList list = {NULL, 0, 0};
    SeqScanIterator *iter = NULL;
    BlockNumber *chain = NULL;
    uint32_t *res = NULL;
    int m, rc = CRYO_OK;
    size_t i;

    if (totals) *totals = t;
    if (!ops) return CRYO_E_NODEV;
    if (!ops->check_blocks) return CRYO_E_UNSUPPORTED;
    memset(batch, 0, sizeof batch);
    iter = cryo_seqscan_iter_create();
    chain = malloc((size_t)max_chain * sizeof *chain);
    res = malloc((size_t)CHECK_BATCH_BLOCKS * 2 * sizeof *res);
    for (m = 0; m < 2; m++) {
        batch[m].comp = malloc(CHECK_BATCH_BLOCKS * sizeof *batch[m].comp);
        batch[m].size = malloc(CHECK_BATCH_BLOCKS * sizeof *batch[m].size);
        batch[m].block = malloc(CHECK_BATCH_BLOCKS * sizeof *batch[m].block);
        batch[m].npages = malloc(CHECK_BATCH_BLOCKS * sizeof *batch[m].npages);
        if (!batch[m].comp || !batch[m].size || !batch[m].block || !batch[m].npages) rc = CRYO_E_NOMEM;
    }
    if (!iter || !chain || !res) rc = CRYO_E_NOMEM;

    while (rc == CRYO_OK) {
        const BlockNumber b = cryo_seqscan_iter_next(iter);
        char *comp = NULL;
        Size csize = 0;
        CompressionMethod method = COMP_LZ4;
        TransactionId xid = 0;
        uint32 nb = 0, j;
        CryoError err;
        if (!BlockNumberIsValid(b) || b >= nblocks) break;
        err = cryo_stage_read_chain(rel, b, &comp, &csize, &method, &xid, chain, max_chain, &nb);
        if (err == CRYO_ERR_EMPTY_BLOCK) { t.empty_pages++; continue; }
        t.blocks++;
        /* the chain's continuation pages are not block starts (a chain that broke off keeps the pages it did read) */
        for (j = 1; j < nb; j++) cryo_seqscan_iter_exclude(iter, chain[j], true);
        if (err != CRYO_ERR_SUCCESS) { rc = add_report(&list, b, CRYO_CHECK_CHAIN, (uint32)err, nb); continue; }
        if (method != COMP_LZ4 && method != COMP_ZSTD) {
            free(comp);
            rc = add_report(&list, b, CRYO_CHECK_METHOD, (uint32)method, nb);
            continue;
        }
        {
            CheckBatch *bt = &batch[method];
            if (bt->n > 0 && bt->bytes + csize > CHECK_BATCH_BYTES) rc = batch_flush(ops, (int)method, bt, res, &list, &t);
            bt->comp[bt->n] = comp;
            bt->size[bt->n] = (uint32_t)csize;
            bt->block[bt->n] = b;
            bt->npages[bt->n] = nb;
            bt->n++;
            bt->bytes += csize;
            if (rc == CRYO_OK && bt->n == CHECK_BATCH_BLOCKS) rc = batch_flush(ops, (int)method, bt, res, &list, &t);
        }
    }
    for (m = 0; m < 2; m++) {
        if (rc == CRYO_OK && batch[m].comp) rc = batch_flush(ops, m, &batch[m], res, &list, &t);
        if (batch[m].comp) batch_clear(&batch[m]);
        free(batch[m].comp); free(batch[m].size); free(batch[m].block); free(batch[m].npages);
    }
    /* the walk meets blocks in ascending order, the batches answer later: the reports are sorted before they go out */
    if (list.n) qsort(list.r, list.n, sizeof *list.r, cmp_report);
    t.bad = list.n;
    if (report)
        for (i = 0; i < list.n; i++) report(arg, &list.r[i]);
    if (totals) *totals = t;
    free(list.r);
    free(res);
    free(chain);
    cryo_seqscan_iter_free(iter);
    return rc;
}
