/* check.c -- see check.h */
#include "check.h"
#include "cryo_codec.h"
#include "walk.h"

#include <string.h>

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

typedef struct {
    const CryoCodecOps *ops;
    CheckBatch batch[2];
    uint32_t *res;
    ReportList list;
    CryoCheckTotals t;
} Check;

/* a block of the walk: one that was not read is a report, a stream joins the batch of its method */
static int visit(void *arg, CryoWalkBlock *b)
{
    Check *c = arg;
    CheckBatch *bt;
    int rc = CRYO_OK;
    if (b->method < 0) return add_report(&c->list, b->block, b->reason, b->detail, b->npages);
    bt = &c->batch[b->method];
    if (bt->n > 0 && bt->bytes + b->csize > CHECK_BATCH_BYTES) rc = batch_flush(c->ops, b->method, bt, c->res, &c->list, &c->t);
    bt->comp[bt->n] = b->comp;
    bt->size[bt->n] = b->csize;
    bt->block[bt->n] = b->block;
    bt->npages[bt->n] = b->npages;
    bt->n++;
    bt->bytes += b->csize;
    if (rc == CRYO_OK && bt->n == CHECK_BATCH_BLOCKS) rc = batch_flush(c->ops, b->method, bt, c->res, &c->list, &c->t);
    return rc;
}

int cryo_check_relation(CryoRel *rel, void (*report)(void *arg, const CryoCheckReport *r), void *arg,
                        CryoCheckTotals *totals)
{
    Check c;
    int m, rc = CRYO_OK;
    size_t i;

    memset(&c, 0, sizeof c);
    if (totals) *totals = c.t;
    c.ops = cryo_host_codec_ops();
    if (!c.ops) return CRYO_E_NODEV;
    if (!c.ops->check_blocks) return CRYO_E_UNSUPPORTED;
    c.res = malloc((size_t)CHECK_BATCH_BLOCKS * 2 * sizeof *c.res);
    if (!c.res) rc = CRYO_E_NOMEM;
    for (m = 0; m < 2; m++) {
        CheckBatch *bt = &c.batch[m];
        bt->comp = malloc(CHECK_BATCH_BLOCKS * sizeof *bt->comp);
        bt->size = malloc(CHECK_BATCH_BLOCKS * sizeof *bt->size);
        bt->block = malloc(CHECK_BATCH_BLOCKS * sizeof *bt->block);
        bt->npages = malloc(CHECK_BATCH_BLOCKS * sizeof *bt->npages);
        if (!bt->comp || !bt->size || !bt->block || !bt->npages) rc = CRYO_E_NOMEM;
    }
    if (rc == CRYO_OK) rc = cryo_walk_relation(rel, visit, &c, &c.t.blocks, &c.t.empty_pages);
    for (m = 0; m < 2; m++) {
        CheckBatch *bt = &c.batch[m];
        if (rc == CRYO_OK) rc = batch_flush(c.ops, m, bt, c.res, &c.list, &c.t);
        if (bt->comp) batch_clear(bt);
        free(bt->comp); free(bt->size); free(bt->block); free(bt->npages);
    }
    /* the walk meets blocks in ascending order, the batches answer later: the reports are sorted before they go out */
    if (c.list.n) qsort(c.list.r, c.list.n, sizeof *c.list.r, cmp_report);
    c.t.bad = c.list.n;
    if (report)
        for (i = 0; i < c.list.n; i++) report(arg, &c.list.r[i]);
    if (totals) *totals = c.t;
    free(c.list.r);
    free(c.res);
    return rc;
}
