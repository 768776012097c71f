/* project.c -- see project.h */
#include "project.h"
#include "filter.h"
#include "scan_iterator.h"

#include <sys/mman.h>

#define PROJECT_MAX_ITEMS (MaxHeapTuplesPerPage - 1) /* records and rows a block can have: one per item */

static int window_blocks = CRYO_FILTER_WINDOW_BLOCKS;
static Size window_bytes = CRYO_FILTER_WINDOW_BYTES;
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_project_set_window(int blocks, Size bytes)
{
    window_blocks = blocks > 0 && blocks < CRYO_FILTER_WINDOW_BLOCKS ? blocks : CRYO_FILTER_WINDOW_BLOCKS;
    window_bytes = bytes > 0 && bytes < CRYO_FILTER_WINDOW_BYTES ? bytes : CRYO_FILTER_WINDOW_BYTES;
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
    const cryo_project *prj;
    uint32 row_bytes;      /* 0: the descriptors are not ones a layout can be made of; the codec refuses them */
    void (*row)(void *, const CryoProjectedRow *);
    void (*report)(void *, const CryoProjectReport *);
    void *arg;
    CryoProjectTotals t;
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
    CryoProjectReport r;
    r.block = block;
    r.reason = reason;
    r.detail = detail;
    j->t.reports++;
    if (j->report) j->report(j->arg, &r);
}

/* the worst case as untouched virtual memory: only the used part is ever written */
static void *reserve(size_t bytes)
{
    void *p = mmap(NULL, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    return p == MAP_FAILED ? NULL : p;
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
static int window_flush(const CryoCodecOps *ops, const CryoCodecProjectOps *pops, Job *j, Window *w)
{
    const size_t rb = j->row_bytes ? j->row_bytes : 8;
    char *rows[2] = {NULL, NULL};
    cryo_project_rec *rec[2] = {NULL, NULL};
    cryo_project_block *table[2] = {NULL, NULL};
    size_t cap[2] = {0, 0};
    uint64_t total[2][2] = {{0, 0}, {0, 0}};
    int m, i, rc = CRYO_OK;

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
        table[m] = malloc(k * sizeof *table[m]);
        if (!table[m]) { rc = CRYO_E_NOMEM; break; }
        cap[m] = k * PROJECT_MAX_ITEMS;
        rows[m] = reserve(cap[m] * rb);
        rec[m] = reserve(cap[m] * sizeof *rec[m]);
        if (!rows[m] || !rec[m]) { rc = CRYO_E_NOMEM; break; }
        rc = pops->project_blocks(ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->f, j->prj, rows[m], cap[m], rec[m], cap[m],
                                  table[m], total[m]);
        j->t.codec_calls++;
        if (rc == CRYO_OK && (j->row_bytes == 0 || total[m][0] > cap[m] || total[m][1] > cap[m])) rc = CRYO_E_HIP; /* not a placement */
        if (rc == CRYO_OK) j->t.bytes_back += k * sizeof *table[m] + total[m][1] * sizeof *rec[m] + total[m][0] * rb;
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const Entry *e = &w->e[i];
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
        if (rows[m]) munmap(rows[m], cap[m] * rb);
        if (rec[m]) munmap(rec[m], cap[m] * sizeof *rec[m]);
        free(table[m]);
    }
    window_clear(w);
    return rc;
}

int cryo_project_scan(CryoRel *rel, const cryo_filter *f, const cryo_project *prj,
                      void (*row_cb)(void *arg, const CryoProjectedRow *r),
                      void (*report)(void *arg, const CryoProjectReport *r), void *arg, CryoProjectTotals *totals)
{
    const CryoCodecOps *ops;
    const CryoCodecProjectOps *pops;
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
    if (!rel || !f || !prj) return CRYO_E_ARG;
    ops = cryo_host_codec_ops();
    if (!ops) return CRYO_E_NODEV;
    pops = cryo_host_project_ops();
    if (!pops || !pops->project_blocks) return CRYO_E_UNSUPPORTED;
    j.f = f; j.prj = prj; j.row = row_cb; j.report = report; j.arg = arg;
    j.row_bytes = layout_row_bytes(f, prj);
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
        if (err == CRYO_ERR_SUCCESS && w.n > 0 && w.bytes + csize > window_bytes) rc = window_flush(ops, pops, &j, &w);
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
        if (w.n == W) rc = window_flush(ops, pops, &j, &w);
    }
    if (rc == CRYO_OK && w.e) rc = window_flush(ops, pops, &j, &w);
    if (w.e) window_clear(&w);
    if (totals) *totals = j.t;
    free(w.e); free(w.src); free(w.src_size);
    free(chain);
    if (iter) cryo_seqscan_iter_free(iter);
    return rc;
}
