/* aggregate.c -- see aggregate.h */
#include "aggregate.h"
#include "scan_iterator.h"

static int window_blocks = CRYO_AGG_WINDOW_BLOCKS;
static Size window_bytes = CRYO_AGG_WINDOW_BYTES;
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_aggregate_set_window(int blocks, Size bytes)
{
    window_blocks = blocks > 0 && blocks < CRYO_AGG_WINDOW_BLOCKS ? blocks : CRYO_AGG_WINDOW_BLOCKS;
    window_bytes = bytes > 0 && bytes < CRYO_AGG_WINDOW_BYTES ? bytes : CRYO_AGG_WINDOW_BYTES;
}
#endif

typedef struct {
    BlockNumber block;
    int method;            /* -1: not read (reason, detail say why) */
    TransactionId xid;
    char *comp;
    uint32 csize;
    uint32 reason, detail;
    size_t at;             /* its place within the codec call of its method */
} Entry;

typedef struct {
    Entry *e;
    int n;
    Size bytes;
    /* one codec call: the streams of one method */
    const void **src;
    uint32_t *src_size;
} Window;

typedef struct {
    const cryo_filter *f;
    const cryo_agg *agg;
    void (*block_cb)(void *, const CryoAggBlock *);
    void (*report)(void *, const CryoAggReport *);
    void *arg;
    CryoAggTotals t;
} Job;

static void window_clear(Window *w)
{
    int i;
    for (i = 0; i < w->n; i++) free(w->e[i].comp);
    w->n = 0;
    w->bytes = 0;
}

static void say(Job *j, BlockNumber block, uint32 reason, uint32 detail)
{
    CryoAggReport r;
    r.block = block;
    r.reason = reason;
    r.detail = detail;
    j->t.reports++;
    if (j->report) j->report(j->arg, &r);
}

/* t += c: n and the 128-bit sum with carry; min and max only from a cell that has values */
static void cell_combine(cryo_agg_cell *t, const cryo_agg_cell *c)
{
    uint64_t lo;
    if (c->n == 0) return;
    if (t->n == 0 || c->min < t->min) t->min = c->min;
    if (t->n == 0 || c->max > t->max) t->max = c->max;
    t->n += c->n;
    lo = t->sum_lo + c->sum_lo;
    t->sum_hi = (int64_t)((uint64_t)t->sum_hi + (uint64_t)c->sum_hi + (lo < t->sum_lo ? 1u : 0u));
    t->sum_lo = lo;
}

/* the window's codec calls (one per method present), then its blocks and reports in block order */
static int window_flush(const CryoCodecOps *ops, const CryoCodecAggOps *aops, Job *j, Window *w)
{
    const uint32_t nc = j->agg->ncols;
    cryo_agg_block *rows[2] = {NULL, NULL};
    cryo_agg_cell *cells[2] = {NULL, NULL};
    int m, i, rc = CRYO_OK;
    uint32_t c;

    if (w->n == 0) return CRYO_OK;
    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        size_t k = 0;
        for (i = 0; i < w->n; i++) {
            Entry *e = &w->e[i];
            if (e->method != m) continue;
            w->src[k] = e->comp;
            w->src_size[k] = e->csize;
            e->at = k++;
        }
        if (k == 0) continue;
        rows[m] = malloc(k * sizeof *rows[m]);
        cells[m] = malloc(k * (nc ? nc : 1) * sizeof *cells[m]);
        if (!rows[m] || !cells[m]) { rc = CRYO_E_NOMEM; break; }
        rc = aops->agg_blocks(ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->agg, rows[m], cells[m]);
        j->t.codec_calls++;
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *rows[m] + k * nc * sizeof *cells[m];
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const Entry *e = &w->e[i];
        const cryo_agg_block *row;
        CryoAggBlock b;
        if (e->method < 0) { say(j, e->block, e->reason, e->detail); continue; }
        row = &rows[e->method][e->at];
        if (row->status != CRYO_FETCH_OK) { say(j, e->block, row->status, 0); continue; }
        j->t.items += row->n_items;
        j->t.matches += row->n_match;
        j->t.bad += row->n_bad;
        b.block = e->block;
        b.created_xid = e->xid;
        b.n_items = row->n_items;
        b.n_match = row->n_match;
        b.n_bad = row->n_bad;
        b.cells = cells[e->method] + e->at * nc;
        for (c = 0; c < nc; c++) {
            const uint8_t type = j->agg->cols[c].type;
            if (type == CRYO_KEY_FLOAT4 || type == CRYO_KEY_FLOAT8) { /* the same 40 bytes as a cryo_agg_cell_f */
                cryo_agg_cell_f tf, cf;
                memcpy(&tf, &j->t.cells[c], sizeof tf);
                memcpy(&cf, &b.cells[c], sizeof cf);
                cryo_agg_cell_f_combine(&tf, &cf);
                memcpy(&j->t.cells[c], &tf, sizeof tf);
            } else
                cell_combine(&j->t.cells[c], &b.cells[c]);
        }
        if (j->block_cb) j->block_cb(j->arg, &b);
    }
    for (m = 0; m < 2; m++) {
        free(rows[m]);
        free(cells[m]);
    }
    window_clear(w);
    return rc;
}

int cryo_aggregate_scan(CryoRel *rel, const cryo_filter *f, const cryo_agg *agg,
                        void (*block_cb)(void *arg, const CryoAggBlock *b),
                        void (*report)(void *arg, const CryoAggReport *r), void *arg, CryoAggTotals *totals)
{
    const CryoCodecOps *ops;
    const CryoCodecAggOps *aops;
    const Size ba = cryo_host_codec_bound(COMP_LZ4, cryo_blcksz), bb = cryo_host_codec_bound(COMP_ZSTD, cryo_blcksz);
    const uint32 max_chain = (uint32)cryo_pages_needed(ba > bb ? ba : bb);
    const int W = window_blocks;
    SeqScanIterator *iter = NULL;
    BlockNumber *chain = NULL, nblocks;
    Job j;
    Window w;
    int rc = CRYO_OK;

    memset(&j, 0, sizeof j);
    memset(&w, 0, sizeof w);
    if (totals) *totals = j.t;
    if (!rel || !f || !agg || agg->ncols == 0 || agg->ncols > CRYO_AGG_MAX_COLS) return CRYO_E_ARG; /* totals hold four cells */
    ops = cryo_host_codec_ops();
    if (!ops) return CRYO_E_NODEV;
    aops = cryo_host_agg_ops();
    if (!aops || !aops->agg_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.agg = agg; j.block_cb = block_cb; j.report = report; j.arg = arg;
    nblocks = rel->ops->nblocks(rel->handle);
    iter = cryo_seqscan_iter_create();
    chain = malloc((size_t)max_chain * sizeof *chain);
    w.e = malloc((size_t)W * sizeof *w.e);
    w.src = malloc((size_t)W * sizeof *w.src);
    w.src_size = malloc((size_t)W * sizeof *w.src_size);
    if (!iter || !chain || !w.e || !w.src || !w.src_size) rc = CRYO_E_NOMEM;

    while (rc == CRYO_OK) {
        const BlockNumber b = cryo_seqscan_iter_next(iter);
        char *comp = NULL;
        Size csize = 0;
        CompressionMethod sm = COMP_LZ4;
        TransactionId xid = 0;
        uint32 nb = 0, q;
        CryoError err;
        Entry *e;
        if (!BlockNumberIsValid(b) || b >= nblocks) break;
        err = cryo_stage_read_chain(rel, b, &comp, &csize, &sm, &xid, chain, max_chain, &nb);
        if (err == CRYO_ERR_EMPTY_BLOCK) { j.t.empty_pages++; continue; }
        j.t.blocks++;
        /* the chain's continuation pages are not block starts (a chain that broke off keeps the pages it did read) */
        for (q = 1; q < nb; q++) cryo_seqscan_iter_exclude(iter, chain[q], true);
        if (err == CRYO_ERR_SUCCESS && w.n > 0 && w.bytes + csize > window_bytes) rc = window_flush(ops, aops, &j, &w);
        if (rc != CRYO_OK) { free(comp); break; }
        e = &w.e[w.n++];
        memset(e, 0, sizeof *e);
        e->block = b;
        e->xid = xid;
        if (err != CRYO_ERR_SUCCESS) {
            e->method = -1; e->reason = CRYO_CHECK_CHAIN; e->detail = (uint32)err;
        } else if (sm != COMP_LZ4 && sm != COMP_ZSTD) {
            free(comp);
            e->method = -1; e->reason = CRYO_CHECK_METHOD; e->detail = (uint32)sm;
        } else {
            e->method = (int)sm; e->comp = comp; e->csize = (uint32)csize;
            w.bytes += csize;
        }
        if (w.n == W) rc = window_flush(ops, aops, &j, &w);
    }
    if (rc == CRYO_OK && w.e) rc = window_flush(ops, aops, &j, &w);
    if (w.e) window_clear(&w);
    if (totals) *totals = j.t;
    free(w.e); free(w.src); free(w.src_size);
    free(chain);
    if (iter) cryo_seqscan_iter_free(iter);
    return rc;
}
