/* group.c -- see group.h */
#include "group.h"
#include "scan_iterator.h"

static int window_blocks = CRYO_GROUP_WINDOW_BLOCKS;
static Size window_bytes = CRYO_GROUP_WINDOW_BYTES;
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_group_set_window(int blocks, Size bytes)
{
    window_blocks = blocks > 0 && blocks < CRYO_GROUP_WINDOW_BLOCKS ? blocks : CRYO_GROUP_WINDOW_BLOCKS;
    window_bytes = bytes > 0 && bytes < CRYO_GROUP_WINDOW_BYTES ? bytes : CRYO_GROUP_WINDOW_BYTES;
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
    const cryo_group *grp;
    const cryo_agg *agg;
    void (*block_cb)(void *, const CryoGroupBlock *);
    void (*report)(void *, const CryoGroupReport *);
    void *arg;
    CryoGroupTotals t;
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
    CryoGroupReport r;
    r.block = block;
    r.reason = reason;
    r.detail = detail;
    j->t.reports++;
    if (j->report) j->report(j->arg, &r);
}

/* the window's codec calls (one per method present, each with room for the worst case: 290 groups per block), then its blocks
 * and reports in block order */
static int window_flush(const CryoCodecOps *ops, const CryoCodecGroupOps *gops, Job *j, Window *w)
{
    const uint32_t nc = j->agg ? j->agg->ncols : 0;
    cryo_group_block *rows[2] = {NULL, NULL};
    cryo_group_rec *recs[2] = {NULL, NULL};
    cryo_agg_cell *cells[2] = {NULL, NULL};
    int m, i, rc = CRYO_OK;

    if (w->n == 0) return CRYO_OK;
    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        size_t k = 0, cap;
        uint64_t total = 0;
        for (i = 0; i < w->n; i++) {
            Entry *e = &w->e[i];
            if (e->method != m) continue;
            w->src[k] = e->comp;
            w->src_size[k] = e->csize;
            e->at = k++;
        }
        if (k == 0) continue;
        cap = k * 290;
        rows[m] = malloc(k * sizeof *rows[m]);
        recs[m] = malloc(cap * sizeof *recs[m]);
        cells[m] = malloc(cap * (nc ? nc : 1) * sizeof *cells[m]);
        if (!rows[m] || !recs[m] || !cells[m]) { rc = CRYO_E_NOMEM; break; }
        rc = gops->group_blocks(ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->grp, j->agg, rows[m], recs[m], cap,
                                nc ? cells[m] : NULL, &total);
        j->t.codec_calls++;
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *rows[m] + total * (sizeof *recs[m] + nc * sizeof *cells[m]);
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const Entry *e = &w->e[i];
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
    window_clear(w);
    return rc;
}

int cryo_group_scan(CryoRel *rel, const cryo_filter *f, const cryo_group *grp, const cryo_agg *agg,
                    void (*block_cb)(void *arg, const CryoGroupBlock *b),
                    void (*report)(void *arg, const CryoGroupReport *r), void *arg, CryoGroupTotals *totals)
{
    const CryoCodecOps *ops;
    const CryoCodecGroupOps *gops;
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
    if (!rel || !f || !grp || (agg && agg->ncols > CRYO_AGG_MAX_COLS)) return CRYO_E_ARG;
    ops = cryo_host_codec_ops();
    if (!ops) return CRYO_E_NODEV;
    gops = cryo_host_group_ops();
    if (!gops || !gops->group_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.grp = grp; j.agg = agg; j.block_cb = block_cb; j.report = report; j.arg = arg;
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
        if (err == CRYO_ERR_SUCCESS && w.n > 0 && w.bytes + csize > window_bytes) rc = window_flush(ops, gops, &j, &w);
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
        if (w.n == W) rc = window_flush(ops, gops, &j, &w);
    }
    if (rc == CRYO_OK && w.e) rc = window_flush(ops, gops, &j, &w);
    if (w.e) window_clear(&w);
    if (totals) *totals = j.t;
    free(w.e); free(w.src); free(w.src_size);
    free(chain);
    if (iter) cryo_seqscan_iter_free(iter);
    return rc;
}
