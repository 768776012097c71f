/* filter.c -- see filter.h */
#include "filter.h"

#define FILTER_MAX_ITEMS (MaxHeapTuplesPerPage - 1) /* records a block can have: one per item */

static CryoWindowLimits window = {CRYO_FILTER_WINDOW_BLOCKS, CRYO_FILTER_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_filter_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_FILTER_WINDOW_BLOCKS, CRYO_FILTER_WINDOW_BYTES);
}
#endif

typedef struct {
    const CryoCodecOps *ops;
    const CryoCodecFilterOps *fops;
    const cryo_filter *f;
    void (*tuple)(void *, const CryoFilteredTuple *);
    void (*report)(void *, const CryoFilterReport *);
    void *arg;
    CryoFilterTotals t;
} Job;

static void say(Job *j, BlockNumber block, uint32 reason, uint32 detail)
{
    j->t.reports++;
    cryo_walk_say(j->report, j->arg, block, reason, detail);
}

/* the window's codec calls (one per method present), then its tuples and reports in block order */
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    const bool count_only = (j->f->flags & CRYO_FILTER_COUNT_ONLY) != 0;
    char *packed[2] = {NULL, NULL};
    cryo_filter_rec *rec[2] = {NULL, NULL};
    cryo_filter_block *rows[2] = {NULL, NULL};
    size_t cap[2] = {0, 0}, rcap[2] = {0, 0};
    uint64_t total[2][2] = {{0, 0}, {0, 0}};
    int m, i, rc = CRYO_OK;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const size_t k = cryo_window_gather(w, m);
        if (k == 0) continue;
        rows[m] = malloc(k * sizeof *rows[m]);
        if (!rows[m]) { rc = CRYO_E_NOMEM; break; }
        if (!count_only) {
            cap[m] = k * cryo_blcksz;
            rcap[m] = k * FILTER_MAX_ITEMS;
            packed[m] = cryo_walk_reserve(cap[m]);
            rec[m] = cryo_walk_reserve(rcap[m] * sizeof *rec[m]);
            if (!packed[m] || !rec[m]) { rc = CRYO_E_NOMEM; break; }
        }
        rc = j->fops->filter_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, packed[m], cap[m], rec[m], rcap[m],
                                    rows[m], total[m]);
        j->t.codec_calls++;
        if (rc == CRYO_OK && (total[m][0] > cap[m] || total[m][1] > rcap[m])) rc = CRYO_E_HIP; /* not a placement */
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *rows[m] + total[m][1] * sizeof *rec[m] + total[m][0];
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
        const cryo_filter_block *row;
        uint64_t at, r, r_end;
        if (e->method < 0) { say(j, e->block, e->reason, e->detail); continue; }
        m = e->method;
        row = &rows[m][e->at];
        j->t.items += row->n_items;
        j->t.matches += row->n_match;
        j->t.bad += row->n_bad;
        if (row->status != CRYO_FETCH_OK) say(j, e->block, row->status, 0);
        if (count_only) continue;
        at = row->off;
        r_end = row->rec_first + row->n_match + row->n_bad;
        if (r_end > total[m][1] || r_end < row->rec_first) { rc = CRYO_E_HIP; break; } /* not a placement */
        for (r = row->rec_first; r < r_end; r++) {
            const cryo_filter_rec *q = &rec[m][r];
            CryoFilteredTuple t;
            /* any status but OK is passed on as it is: ITEM, TUPLE, and UNDECIDED under a byte-string key */
            if (q->status != CRYO_FETCH_OK) { say(j, e->block, q->status, q->pos); continue; }
            if (q->len == 0 || at + MAXALIGN(q->len) > total[m][0]) { rc = CRYO_E_HIP; break; } /* not a placement */
            t.block = e->block;
            t.pos = q->pos;
            t.created_xid = e->xid;
            t.data = packed[m] + at;
            t.len = q->len;
            at += MAXALIGN(q->len);
            if (j->tuple) j->tuple(j->arg, &t);
        }
    }
    for (m = 0; m < 2; m++) {
        cryo_walk_release(packed[m], cap[m]);
        cryo_walk_release(rec[m], rcap[m] * sizeof *rec[m]);
        free(rows[m]);
    }
    return rc;
}

int cryo_filter_scan(CryoRel *rel, const cryo_filter *f,
                     void (*tuple)(void *arg, const CryoFilteredTuple *t),
                     void (*report)(void *arg, const CryoFilterReport *r), void *arg, CryoFilterTotals *totals)
{
    Job j;
    int rc;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (!rel || !f) return CRYO_E_ARG;
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    j.fops = cryo_host_filter_ops();
    if (!j.fops || !j.fops->filter_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.tuple = tuple; j.report = report; j.arg = arg;
    rc = cryo_walk_windowed(rel, window, window_flush, &j, &j.t.blocks, &j.t.empty_pages);
    if (totals) *totals = j.t;
    return rc;
}
