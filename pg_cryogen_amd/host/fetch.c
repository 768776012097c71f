/* fetch.c -- see fetch.h */
#include "fetch.h"
#include "cryo_codec.h"

#include <sys/mman.h>

#define FETCH_MAX_ITEMS (MaxHeapTuplesPerPage - 1) /* what a lossy page asks for: every position a block can hold */

typedef struct {
    const CryoFetchPage *page;
    int method;            /* -1: not read (reason, detail say why) */
    TransactionId xid;
    char *comp;
    uint32 csize;
    uint32 reason, detail;
    uint64_t first;        /* its first request within the codec call of its method */
} Entry;

typedef struct {
    Entry *e;
    int n;
    Size bytes;
    /* one codec call: the streams of one method */
    const void **src;
    uint32_t *src_size;
    uint64_t *req_first;
    uint16_t *pos;
    size_t pos_cap;
} Window;

typedef struct {
    void (*tuple)(void *, const CryoFetchedTuple *);
    void (*report)(void *, const CryoFetchReport *);
    void *arg;
    CryoFetchTotals t;
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
    CryoFetchReport r;
    r.block = block;
    r.reason = reason;
    r.detail = detail;
    j->t.bad++;
    if (j->report) j->report(j->arg, &r);
}

static uint32 page_requests(const CryoFetchPage *p) { return p->ntuples < 0 ? FETCH_MAX_ITEMS : (uint32)p->ntuples; }

/* the window's codec calls (one per method present), then its tuples and reports in page order */
static int window_flush(const CryoCodecOps *ops, const CryoCodecFetchOps *fops, Job *j, Window *w)
{
    char *packed[2] = {NULL, NULL};
    cryo_fetch_result *res[2] = {NULL, NULL};
    Size cap[2] = {0, 0};
    int m, i, rc = CRYO_OK;

    if (w->n == 0) return CRYO_OK;
    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        size_t k = 0;
        uint64_t nreq = 0, total = 0;
        for (i = 0; i < w->n; i++)
            if (w->e[i].method == m) nreq += page_requests(w->e[i].page);
        if (nreq > w->pos_cap) {
            uint16_t *p = realloc(w->pos, (size_t)nreq * sizeof *p);
            if (!p) { rc = CRYO_E_NOMEM; break; }
            w->pos = p;
            w->pos_cap = (size_t)nreq;
        }
        nreq = 0;
        for (i = 0; i < w->n; i++) {
            Entry *e = &w->e[i];
            uint32 q, nq;
            if (e->method != m) continue;
            nq = page_requests(e->page);
            w->src[k] = e->comp;
            w->src_size[k] = e->csize;
            w->req_first[k] = e->first = nreq;
            for (q = 0; q < nq; q++) w->pos[nreq + q] = e->page->ntuples < 0 ? (uint16_t)(q + 1) : e->page->offsets[q];
            nreq += nq;
            k++;
        }
        if (k == 0) continue;
        w->req_first[k] = nreq;
        /* the worst case as untouched virtual memory: only the packed part is ever written */
        cap[m] = k * cryo_blcksz;
        packed[m] = mmap(NULL, cap[m], PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (packed[m] == MAP_FAILED) { packed[m] = NULL; rc = CRYO_E_NOMEM; break; }
        res[m] = malloc((size_t)(nreq ? nreq : 1) * sizeof *res[m]);
        if (!res[m]) { rc = CRYO_E_NOMEM; break; }
        rc = fops->fetch_blocks(ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, w->req_first, w->pos, packed[m], cap[m], res[m],
                                &total);
        j->t.codec_calls++;
        j->t.blocks += k;
        if (rc == CRYO_OK) j->t.bytes_back += total + nreq * sizeof *res[m];
        if (rc == CRYO_OK && total > cap[m]) rc = CRYO_E_HIP; /* not a placement */
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const Entry *e = &w->e[i];
        const CryoFetchPage *p = e->page;
        uint32 q, nq = page_requests(p);
        if (e->method < 0) { say(j, p->block, e->reason, e->detail); continue; }
        for (q = 0; q < nq; q++) {
            const cryo_fetch_result *r = &res[e->method][e->first + q];
            const uint16 pos = p->ntuples < 0 ? (uint16)(q + 1) : p->offsets[q];
            if (r->status == CRYO_FETCH_OK) {
                CryoFetchedTuple t;
                if (r->len == 0 || r->off + MAXALIGN(r->len) > cap[e->method]) { rc = CRYO_E_HIP; break; } /* not a placement */
                t.block = p->block;
                t.pos = pos;
                t.created_xid = e->xid;
                t.data = packed[e->method] + r->off;
                t.len = r->len;
                j->t.tuples++;
                if (j->tuple) j->tuple(j->arg, &t);
                continue;
            }
            if (p->ntuples < 0 && r->status == CRYO_FETCH_NOITEM) break; /* the lossy page's end */
            say(j, p->block, r->status, pos);
            if (r->status == CRYO_FETCH_STREAM || r->status == CRYO_FETCH_HEADER || r->status == CRYO_FETCH_BADREQ) break;
        }
    }
    for (m = 0; m < 2; m++) {
        if (packed[m]) munmap(packed[m], cap[m]);
        free(res[m]);
    }
    window_clear(w);
    return rc;
}

int cryo_fetch_tuples(CryoRel *rel, const CryoFetchPage *pages, size_t npages,
                      void (*tuple)(void *arg, const CryoFetchedTuple *t),
                      void (*report)(void *arg, const CryoFetchReport *r), void *arg, CryoFetchTotals *totals)
{
    const CryoCodecOps *ops;
    const CryoCodecFetchOps *fops;
    const Size ba = cryo_host_codec_bound(COMP_LZ4, cryo_blcksz), bb = cryo_host_codec_bound(COMP_ZSTD, cryo_blcksz);
    const uint32 max_chain = (uint32)cryo_pages_needed(ba > bb ? ba : bb);
    const int W = CRYO_FETCH_WINDOW_BLOCKS;
    BlockNumber *chain = NULL, nblocks;
    Job j;
    Window w;
    size_t i;
    int rc = CRYO_OK;

    memset(&j, 0, sizeof j);
    memset(&w, 0, sizeof w);
    if (totals) *totals = j.t;
    if (!rel || (!pages && npages)) return CRYO_E_ARG;
    ops = cryo_host_codec_ops();
    if (!ops) return CRYO_E_NODEV;
    fops = cryo_host_fetch_ops();
    if (!fops || !fops->fetch_blocks) return CRYO_E_UNSUPPORTED;
    j.tuple = tuple; j.report = report; j.arg = arg;
    nblocks = rel->ops->nblocks(rel->handle);
    chain = malloc((size_t)max_chain * sizeof *chain);
    w.e = malloc((size_t)W * sizeof *w.e);
    w.src = malloc((size_t)W * sizeof *w.src);
    w.src_size = malloc((size_t)W * sizeof *w.src_size);
    w.req_first = malloc(((size_t)W + 1) * sizeof *w.req_first);
    if (!chain || !w.e || !w.src || !w.src_size || !w.req_first) rc = CRYO_E_NOMEM;

    for (i = 0; rc == CRYO_OK && i < npages; i++) {
        const CryoFetchPage *p = &pages[i];
        char *comp = NULL;
        Size csize = 0;
        CompressionMethod sm = COMP_LZ4;
        TransactionId xid = 0;
        uint32 nb = 0;
        CryoError err;
        Entry *e;
        j.t.pages++;
        if (p->ntuples == 0) continue;
        if (p->ntuples > 0 && !p->offsets) { rc = CRYO_E_ARG; break; }
        /* the metapage and pages beyond the end are no chain starts (as cryo_read_data_batch treats them) */
        if (p->block == CRYO_META_PAGE || p->block >= nblocks) { j.t.not_block_starts++; continue; }
        err = cryo_stage_read_chain(rel, p->block, &comp, &csize, &sm, &xid, chain, max_chain, &nb);
        if (err == CRYO_ERR_WRONG_STARTING_BLOCK || err == CRYO_ERR_EMPTY_BLOCK) { j.t.not_block_starts++; continue; }
        if (err == CRYO_ERR_SUCCESS && w.n > 0 && w.bytes + csize > CRYO_FETCH_WINDOW_BYTES) rc = window_flush(ops, fops, &j, &w);
        if (rc != CRYO_OK) { free(comp); break; }
        e = &w.e[w.n++];
        memset(e, 0, sizeof *e);
        e->page = p;
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
        if (w.n == W) rc = window_flush(ops, fops, &j, &w);
    }
    if (rc == CRYO_OK && w.e) rc = window_flush(ops, fops, &j, &w);
    if (w.e) window_clear(&w);
    if (totals) *totals = j.t;
    free(w.e); free(w.src); free(w.src_size); free(w.req_first); free(w.pos);
    free(chain);
    return rc;
}
