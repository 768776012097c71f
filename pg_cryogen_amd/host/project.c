/* project.c -- see project.h */
#include "project.h"
#include "filter.h"

#define PROJECT_MAX_ITEMS (MaxHeapTuplesPerPage - 1) /* records and rows a block can have: one per item */

static CryoWindowLimits window = {CRYO_FILTER_WINDOW_BLOCKS, CRYO_FILTER_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_project_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_FILTER_WINDOW_BLOCKS, CRYO_FILTER_WINDOW_BYTES);
}
#endif

typedef struct {
    const CryoCodecOps *ops;
    const CryoCodecProjectOps *pops;
    const cryo_filter *f;
    const cryo_project *prj;
    uint32 row_bytes;      /* 0: the descriptors are not ones a layout can be made of; the codec refuses them */
    void (*row)(void *, const CryoProjectedRow *);
    void (*report)(void *, const CryoProjectReport *);
    void *arg;
    CryoProjectTotals t;
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

/* the window's codec calls (one per method present), then its rows and reports in block order */
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    const size_t rb = j->row_bytes ? j->row_bytes : 8;
    char *rows[2] = {NULL, NULL};
    cryo_project_rec *rec[2] = {NULL, NULL};
    cryo_project_block *table[2] = {NULL, NULL};
    size_t cap[2] = {0, 0};
    uint64_t total[2][2] = {{0, 0}, {0, 0}};
    int m, i, rc = CRYO_OK;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const size_t k = cryo_window_gather(w, m);
        if (k == 0) continue;
        table[m] = malloc(k * sizeof *table[m]);
        if (!table[m]) { rc = CRYO_E_NOMEM; break; }
        cap[m] = k * PROJECT_MAX_ITEMS;
        rows[m] = cryo_walk_reserve(cap[m] * rb);
        rec[m] = cryo_walk_reserve(cap[m] * sizeof *rec[m]);
        if (!rows[m] || !rec[m]) { rc = CRYO_E_NOMEM; break; }
        rc = j->pops->project_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->prj, rows[m], cap[m], rec[m],
                                     cap[m], table[m], total[m]);
        j->t.codec_calls++;
        if (rc == CRYO_OK && (j->row_bytes == 0 || total[m][0] > cap[m] || total[m][1] > cap[m])) rc = CRYO_E_HIP; /* not a placement */
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *table[m] + total[m][1] * sizeof *rec[m] + total[m][0] * rb;
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
        const cryo_project_block *row;
        uint64_t at, r, r_end;
        if (e->method < 0) { say(j, e->block, e->reason, e->detail); continue; }
        m = e->method;
        row = &table[m][e->at];
        j->t.items += row->n_items;
        j->t.matches += row->n_match;
        j->t.bad += row->n_bad;
        if (row->status != CRYO_FETCH_OK) say(j, e->block, row->status, 0);
        at = row->row_first;
        r_end = row->rec_first + row->n_match + row->n_bad;
        if (r_end > total[m][1] || r_end < row->rec_first || at + row->n_match > total[m][0] || at + row->n_match < at) {
            rc = CRYO_E_HIP; /* not a placement */
            break;
        }
        for (r = row->rec_first; r < r_end; r++) {
            const cryo_project_rec *q = &rec[m][r];
            CryoProjectedRow t;
            /* any status but OK is passed on as it is: ITEM, TUPLE, and UNDECIDED under a byte-string key */
            if (q->status != CRYO_FETCH_OK) { say(j, e->block, q->status, q->pos); continue; }
            if (at >= row->row_first + row->n_match) { rc = CRYO_E_HIP; break; } /* more match records than rows */
            t.block = e->block;
            t.pos = q->pos;
            t.created_xid = e->xid;
            t.nulls = q->nulls;
            t.data = rows[m] + at * rb;
            t.row_bytes = (uint32)rb;
            at++;
            if (j->row) j->row(j->arg, &t);
        }
    }
    for (m = 0; m < 2; m++) {
        cryo_walk_release(rows[m], cap[m] * rb);
        cryo_walk_release(rec[m], cap[m] * sizeof *rec[m]);
        free(table[m]);
    }
    return rc;
}

int cryo_project_scan(CryoRel *rel, const cryo_filter *f, const cryo_project *prj,
                      void (*row_cb)(void *arg, const CryoProjectedRow *r),
                      void (*report)(void *arg, const CryoProjectReport *r), void *arg, CryoProjectTotals *totals)
{
    Job j;
    int rc;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (!rel || !f || !prj) return CRYO_E_ARG;
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    j.pops = cryo_host_project_ops();
    if (!j.pops || !j.pops->project_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.prj = prj; j.row = row_cb; j.report = report; j.arg = arg;
    j.row_bytes = layout_row_bytes(f, prj);
    rc = cryo_walk_windowed(rel, window, window_flush, &j, &j.t.blocks, &j.t.empty_pages);
    if (totals) *totals = j.t;
    return rc;
}
