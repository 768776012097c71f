/* aggregate.c -- see aggregate.h */
#include "aggregate.h"

static CryoWindowLimits window = {CRYO_AGG_WINDOW_BLOCKS, CRYO_AGG_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_aggregate_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_AGG_WINDOW_BLOCKS, CRYO_AGG_WINDOW_BYTES);
}
#endif

typedef struct {
    const CryoCodecOps *ops;
    const CryoCodecAggOps *aops;
    const cryo_filter *f;
    const cryo_agg *agg;
    void (*block_cb)(void *, const CryoAggBlock *);
    void (*report)(void *, const CryoAggReport *);
    void *arg;
    CryoAggTotals t;
} Job;

static void say(Job *j, BlockNumber block, uint32 reason, uint32 detail)
{
    j->t.reports++;
    cryo_walk_say(j->report, j->arg, block, reason, detail);
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
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    const uint32_t nc = j->agg->ncols;
    cryo_agg_block *rows[2] = {NULL, NULL};
    cryo_agg_cell *cells[2] = {NULL, NULL};
    int m, i, rc = CRYO_OK;
    uint32_t c;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const size_t k = cryo_window_gather(w, m);
        if (k == 0) continue;
        rows[m] = malloc(k * sizeof *rows[m]);
        cells[m] = malloc(k * (nc ? nc : 1) * sizeof *cells[m]);
        if (!rows[m] || !cells[m]) { rc = CRYO_E_NOMEM; break; }
        rc = j->aops->agg_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->agg, rows[m], cells[m]);
        j->t.codec_calls++;
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *rows[m] + k * nc * sizeof *cells[m];
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
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
    return rc;
}

int cryo_aggregate_scan(CryoRel *rel, const cryo_filter *f, const cryo_agg *agg,
                        void (*block_cb)(void *arg, const CryoAggBlock *b),
                        void (*report)(void *arg, const CryoAggReport *r), void *arg, CryoAggTotals *totals)
{
    Job j;
    int rc;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (!rel || !f || !agg || agg->ncols == 0 || agg->ncols > CRYO_AGG_MAX_COLS) return CRYO_E_ARG; /* totals hold four cells */
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    j.aops = cryo_host_agg_ops();
    if (!j.aops || !j.aops->agg_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.agg = agg; j.block_cb = block_cb; j.report = report; j.arg = arg;
    rc = cryo_walk_windowed(rel, window, window_flush, &j, &j.t.blocks, &j.t.empty_pages);
    if (totals) *totals = j.t;
    return rc;
}
