/* topn.c -- see topn.h */
#include "topn.h"
#include "filter.h"

#define TOPN_MAX_ITEMS (MaxHeapTuplesPerPage - 1) /* kept rows a block can have: one per item */

static CryoWindowLimits window = {CRYO_FILTER_WINDOW_BLOCKS, CRYO_FILTER_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_topn_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_FILTER_WINDOW_BLOCKS, CRYO_FILTER_WINDOW_BYTES);
}
#endif

typedef struct {
    const CryoCodecOps *ops;
    const CryoCodecTopnOps *tops;
    const cryo_filter *f;
    const cryo_order *ord;
    const cryo_project *prj;
    uint32 row_bytes;      /* 0: the descriptors are not ones a layout can be made of; the codec refuses them */
    void (*block_cb)(void *, const CryoTopnBlock *);
    void (*report)(void *, const CryoTopnReport *);
    void *arg;
    CryoTopnTotals t;
} Job;

static void say(Job *j, BlockNumber block, uint32 reason, uint32 detail)
{
    j->t.reports++;
    cryo_walk_say(j->report, j->arg, block, reason, detail);
}

/* row_bytes of the projection by the layout rule of include/cryo_codec.h, or 0 when a column is not one the rule covers (the
 * codec then refuses the descriptors with CRYO_E_ARG, and no buffer is looked at) */
static uint32 layout_row_bytes(const cryo_filter *f, const cryo_project *prj)
{
    uint32_t end = 0, j;
    if (!f->atts || !prj->cols || prj->ncols == 0 || prj->ncols > CRYO_PROJECT_MAX_COLS) return 0;
    for (j = 0; j < prj->ncols; j++) {
        const uint32_t att = prj->cols[j].att;
        int16_t len;
        if (att == 0 || att > f->natts) return 0;
        len = f->atts[att - 1].attlen;
        if (len != 1 && len != 2 && len != 4 && len != 8) return 0;
        end = CRYO_PROJECT_COL_OFFSET(end, len) + (uint32_t)len;
    }
    return CRYO_PROJECT_ROW_BYTES(end);
}

/* the window's codec calls (one per method present), then its blocks and reports in block order */
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    const size_t rb = j->row_bytes ? j->row_bytes : 8;
    const size_t per = j->ord->limit < TOPN_MAX_ITEMS ? (j->ord->limit ? j->ord->limit : 1) : TOPN_MAX_ITEMS;
    char *rows[2] = {NULL, NULL};
    cryo_topn_rec *rec[2] = {NULL, NULL};
    cryo_topn_block *table[2] = {NULL, NULL};
    size_t cap[2] = {0, 0};
    uint64_t total[2] = {0, 0};
    int m, i, rc = CRYO_OK;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const size_t k = cryo_window_gather(w, m);
        if (k == 0) continue;
        table[m] = malloc(k * sizeof *table[m]);
        if (!table[m]) { rc = CRYO_E_NOMEM; break; }
        cap[m] = k * per;
        rows[m] = cryo_walk_reserve(cap[m] * rb);
        rec[m] = cryo_walk_reserve(cap[m] * sizeof *rec[m]);
        if (!rows[m] || !rec[m]) { rc = CRYO_E_NOMEM; break; }
        rc = j->tops->topn_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->ord, j->prj, rows[m], rec[m], cap[m],
                                  table[m], &total[m]);
        j->t.codec_calls++;
        if (rc == CRYO_OK && (j->row_bytes == 0 || total[m] > cap[m])) rc = CRYO_E_HIP; /* not a placement */
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *table[m] + total[m] * (sizeof *rec[m] + rb);
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
        const cryo_topn_block *row;
        CryoTopnBlock b;
        if (e->method < 0) { say(j, e->block, e->reason, e->detail); continue; }
        m = e->method;
        row = &table[m][e->at];
        if (row->status != CRYO_FETCH_OK) { say(j, e->block, row->status, 0); continue; }
        if (row->n_rows > per || row->row_first > total[m] || row->n_rows > total[m] - row->row_first) {
            rc = CRYO_E_HIP; /* not a placement */
            break;
        }
        j->t.items += row->n_items;
        j->t.matches += row->n_match;
        j->t.bad += row->n_bad;
        j->t.rows += row->n_rows;
        b.block = e->block;
        b.created_xid = e->xid;
        b.n_items = row->n_items;
        b.n_match = row->n_match;
        b.n_bad = row->n_bad;
        b.n_rows = row->n_rows;
        b.rec = rec[m] + row->row_first;
        b.rows = rows[m] + row->row_first * rb;
        b.row_bytes = (uint32)rb;
        if (j->block_cb) j->block_cb(j->arg, &b);
    }
    for (m = 0; m < 2; m++) {
        cryo_walk_release(rows[m], cap[m] * rb);
        cryo_walk_release(rec[m], cap[m] * sizeof *rec[m]);
        free(table[m]);
    }
    return rc;
}

int cryo_topn_scan(CryoRel *rel, const cryo_filter *f, const cryo_order *ord, const cryo_project *prj,
                   void (*block_cb)(void *arg, const CryoTopnBlock *b),
                   void (*report)(void *arg, const CryoTopnReport *r), void *arg, CryoTopnTotals *totals)
{
    Job j;
    int rc;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (!rel || !f || !ord || !prj) return CRYO_E_ARG;
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    j.tops = cryo_host_topn_ops();
    if (!j.tops || !j.tops->topn_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.ord = ord; j.prj = prj; j.block_cb = block_cb; j.report = report; j.arg = arg;
    j.row_bytes = layout_row_bytes(f, prj);
    rc = cryo_walk_windowed(rel, window, window_flush, &j, &j.t.blocks, &j.t.empty_pages);
    if (totals) *totals = j.t;
    return rc;
}

/* ---- the merge ---- */

int cryo_topn_merge_init(CryoTopnMerge *m, const cryo_order *ord, uint32 limit, uint32 row_bytes)
{
    uint32 j;
    if (!m) return CRYO_E_ARG;
    memset(m, 0, sizeof *m);
    if (!ord || !ord->by || ord->nby == 0 || ord->nby > CRYO_ORDER_MAX_BY || limit == 0 || row_bytes == 0 || (row_bytes & 7u) != 0)
        return CRYO_E_ARG;
    for (j = 0; j < ord->nby; j++) {
        if ((ord->by[j].flags & ~(CRYO_ORDER_DESC | CRYO_ORDER_NULLS_FIRST)) != 0) return CRYO_E_ARG;
        m->by[j] = ord->by[j];
    }
    m->nby = ord->nby;
    m->limit = limit;
    m->row_bytes = row_bytes;
    return CRYO_OK;
}

int cryo_topn_merge_compare(const CryoTopnMerge *m, const cryo_topn_rec *a, const cryo_topn_rec *b)
{
    uint32 j;
    for (j = 0; j < m->nby; j++) {
        const uint32 flags = m->by[j].flags;
        const int null_class = (flags & CRYO_ORDER_NULLS_FIRST) ? 0 : 2;
        const int ca = ((a->key_nulls >> j) & 1u) ? null_class : 1, cb = ((b->key_nulls >> j) & 1u) ? null_class : 1;
        int64_t ka, kb;
        if (ca != cb) return ca < cb ? -1 : 1;
        if (ca != 1) continue; /* two NULLs are equal */
        /* DESC is the complement, never the negation: ~v reverses the signed order and exists for INT64_MIN */
        ka = (flags & CRYO_ORDER_DESC) ? ~a->key[j] : a->key[j];
        kb = (flags & CRYO_ORDER_DESC) ? ~b->key[j] : b->key[j];
        if (ka != kb) return ka < kb ? -1 : 1;
    }
    return 0;
}

/* a two-way merge of what is held (ordered) with the block (ordered), cut at the limit; on a tie what is held goes first */
int cryo_topn_merge_add(CryoTopnMerge *m, const cryo_topn_rec *rec, const void *rows, uint32 n)
{
    const size_t rb = m ? m->row_bytes : 0;
    uint64 want;
    uint32 out, a = 0, b = 0, k;
    cryo_topn_rec *nrec;
    char *nrows;
    if (!m || m->limit == 0 || (n > 0 && (!rec || !rows))) return CRYO_E_ARG;
    if (n == 0) return CRYO_OK;
    want = (uint64)m->n + n;
    out = want < m->limit ? (uint32)want : m->limit;
    nrec = malloc((size_t)out * sizeof *nrec);
    nrows = malloc((size_t)out * rb);
    if (!nrec || !nrows) {
        free(nrec);
        free(nrows);
        return CRYO_E_NOMEM;
    }
    for (k = 0; k < out; k++) {
        const bool held = a < m->n && (b >= n || cryo_topn_merge_compare(m, &m->rec[a], &rec[b]) <= 0);
        if (held) {
            nrec[k] = m->rec[a];
            memcpy(nrows + (size_t)k * rb, m->rows + (size_t)a * rb, rb);
            a++;
        } else {
            nrec[k] = rec[b];
            memcpy(nrows + (size_t)k * rb, (const char *)rows + (size_t)b * rb, rb);
            b++;
        }
    }
    free(m->rec);
    free(m->rows);
    m->rec = nrec;
    m->rows = nrows;
    m->n = out;
    return CRYO_OK;
}

uint32 cryo_topn_merge_finish(const CryoTopnMerge *m, const cryo_topn_rec **rec, const void **rows)
{
    if (rec) *rec = m ? m->rec : NULL;
    if (rows) *rows = m ? m->rows : NULL;
    return m ? m->n : 0;
}

void cryo_topn_merge_free(CryoTopnMerge *m)
{
    if (!m) return;
    free(m->rec);
    free(m->rows);
    m->rec = NULL;
    m->rows = NULL;
    m->n = 0;
}
