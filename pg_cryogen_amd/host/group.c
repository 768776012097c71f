/* group.c -- see group.h */
#include "group.h"

static CryoWindowLimits window = {CRYO_GROUP_WINDOW_BLOCKS, CRYO_GROUP_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_group_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_GROUP_WINDOW_BLOCKS, CRYO_GROUP_WINDOW_BYTES);
}
#endif

typedef struct {
    const CryoCodecOps *ops;
    const CryoCodecGroupOps *gops;
    const cryo_filter *f;
    const cryo_group *grp;
    const cryo_agg *agg;
    void (*block_cb)(void *, const CryoGroupBlock *);
    void (*report)(void *, const CryoGroupReport *);
    void *arg;
    CryoGroupTotals t;
} Job;

/* the cells of a group: the aggregate cells, then -- CRYO_GROUP_TEXT -- a cryo_group_key per byte-string group column.  A
 * descriptor the codec will refuse counts as it stands: the call comes back with CRYO_E_ARG before a cell is looked at */
static uint32_t cells_per_group(const cryo_group *grp, const cryo_agg *agg)
{
    uint32_t n = agg ? agg->ncols : 0, c;
    if (grp->rsv == CRYO_GROUP_TEXT && grp->by)
        for (c = 0; c < grp->nby && c < CRYO_GROUP_MAX_BY; c++)
            if (grp->by[c].type == CRYO_KEY_BYTES) n++;
    return n;
}

static void say(Job *j, BlockNumber block, uint32 reason, uint32 detail)
{
    j->t.reports++;
    cryo_walk_say(j->report, j->arg, block, reason, detail);
}

/* the window's codec calls (one per method present, each with room for the worst case: 290 groups per block), then its blocks
 * and reports in block order */
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    const uint32_t nc = cells_per_group(j->grp, j->agg);
    cryo_group_block *rows[2] = {NULL, NULL};
    cryo_group_rec *recs[2] = {NULL, NULL};
    cryo_agg_cell *cells[2] = {NULL, NULL};
    int m, i, rc = CRYO_OK;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const size_t k = cryo_window_gather(w, m), cap = k * 290;
        uint64_t total = 0;
        if (k == 0) continue;
        rows[m] = malloc(k * sizeof *rows[m]);
        recs[m] = malloc(cap * sizeof *recs[m]);
        cells[m] = malloc(cap * (nc ? nc : 1) * sizeof *cells[m]);
        if (!rows[m] || !recs[m] || !cells[m]) { rc = CRYO_E_NOMEM; break; }
        rc = j->gops->group_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->grp, j->agg, rows[m], recs[m], cap,
                                   nc ? cells[m] : NULL, &total);
        j->t.codec_calls++;
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *rows[m] + total * (sizeof *recs[m] + nc * sizeof *cells[m]);
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
        const cryo_group_block *row;
        CryoGroupBlock b;
        if (e->method < 0) { say(j, e->block, e->reason, e->detail); continue; }
        row = &rows[e->method][e->at];
        if (row->status != CRYO_FETCH_OK) { say(j, e->block, row->status, 0); continue; }
        j->t.items += row->n_items;
        j->t.matches += row->n_match;
        j->t.bad += row->n_bad;
        j->t.groups += row->n_groups;
        b.block = e->block;
        b.created_xid = e->xid;
        b.n_items = row->n_items;
        b.n_match = row->n_match;
        b.n_bad = row->n_bad;
        b.n_groups = row->n_groups;
        b.recs = recs[e->method] + row->first_group;
        b.cells = nc ? cells[e->method] + row->first_group * nc : NULL;
        if (j->block_cb) j->block_cb(j->arg, &b);
    }
    for (m = 0; m < 2; m++) {
        free(rows[m]);
        free(recs[m]);
        free(cells[m]);
    }
    return rc;
}

int cryo_group_scan(CryoRel *rel, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                    void (*block_cb)(void *arg, const CryoGroupBlock *b),
                    void (*report)(void *arg, const CryoGroupReport *r), void *arg, CryoGroupTotals *totals)
{
    Job j;
    int rc;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (!rel || !f || !grp || (agg && agg->ncols > CRYO_AGG_MAX_COLS)) return CRYO_E_ARG;
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    j.gops = cryo_host_group_ops();
    if (!j.gops || !j.gops->group_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.grp = grp; j.agg = agg; j.block_cb = block_cb; j.report = report; j.arg = arg;
    rc = cryo_walk_windowed(rel, window, window_flush, &j, &j.t.blocks, &j.t.empty_pages);
    if (totals) *totals = j.t;
    return rc;
}
