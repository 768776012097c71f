/* fetch.c -- see fetch.h */
#include "fetch.h"
#include "cryo_codec.h"

#include <string.h>

#define FETCH_MAX_ITEMS (MaxHeapTuplesPerPage - 1) /* what a lossy page asks for: every position a block can hold */

static CryoWindowLimits window = {CRYO_FETCH_WINDOW_BLOCKS, CRYO_FETCH_WINDOW_BYTES};
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_fetch_set_window(int blocks, Size bytes)
{
    window = cryo_window_limits(blocks, bytes, CRYO_FETCH_WINDOW_BLOCKS, CRYO_FETCH_WINDOW_BYTES);
}
#endif

typedef struct {
    const CryoCodecOps *ops;
    const CryoCodecFetchOps *fops;
    void (*tuple)(void *, const CryoFetchedTuple *);
    void (*report)(void *, const CryoFetchReport *);
    void *arg;
    /* one codec call: stream k owns requests req_first[k] .. req_first[k + 1] - 1 of pos */
    uint64_t *req_first;
    uint16_t *pos;
    size_t pos_cap;
    CryoFetchTotals t;
} Job;

static void say(Job *j, BlockNumber block, uint32 reason, uint32 detail)
{
    j->t.bad++;
    cryo_walk_say(j->report, j->arg, block, reason, detail);
}

static uint32 page_requests(const CryoFetchPage *p) { return p->ntuples < 0 ? FETCH_MAX_ITEMS : (uint32)p->ntuples; }

/* the window's codec calls (one per method present), then its tuples and reports in page order */
static int window_flush(void *arg, CryoWindow *w)
{
    Job *j = arg;
    char *packed[2] = {NULL, NULL};
    cryo_fetch_result *res[2] = {NULL, NULL};
    Size cap[2] = {0, 0};
    uint64_t first[2] = {0, 0}; /* of the entry at hand, within the call of its method: the calls took them in entry order */
    int m, i, rc = CRYO_OK;

    for (m = 0; m < 2 && rc == CRYO_OK; m++) {
        const size_t k = cryo_window_gather(w, m);
        uint64_t nreq = 0, total = 0;
        if (k == 0) continue;
        for (i = 0; i < w->n; i++)
            if (w->e[i].method == m) nreq += page_requests(w->e[i].tag);
        if (nreq > j->pos_cap) {
            uint16_t *p = realloc(j->pos, (size_t)nreq * sizeof *p);
            if (!p) { rc = CRYO_E_NOMEM; break; }
            j->pos = p;
            j->pos_cap = (size_t)nreq;
        }
        nreq = 0;
        for (i = 0; i < w->n; i++) {
            const CryoWalkBlock *e = &w->e[i];
            const CryoFetchPage *p = e->tag;
            uint32 q, nq;
            if (e->method != m) continue;
            nq = page_requests(p);
            j->req_first[e->at] = nreq;
            for (q = 0; q < nq; q++) j->pos[nreq + q] = p->ntuples < 0 ? (uint16_t)(q + 1) : p->offsets[q];
            nreq += nq;
        }
        j->req_first[k] = nreq;
        /* the worst case as untouched virtual memory: only the packed part is ever written */
        cap[m] = k * cryo_blcksz;
        packed[m] = cryo_walk_reserve(cap[m]);
        if (!packed[m]) { rc = CRYO_E_NOMEM; break; }
        res[m] = malloc((size_t)(nreq ? nreq : 1) * sizeof *res[m]);
        if (!res[m]) { rc = CRYO_E_NOMEM; break; }
        rc = j->fops->fetch_blocks(j->ops->ctx, m, w->src, w->src_size, k, cryo_blcksz, j->req_first, j->pos, packed[m], cap[m],
                                   res[m], &total);
        j->t.codec_calls++;
        j->t.blocks += k;
        if (rc == CRYO_OK) j->t.bytes_back += total + nreq * sizeof *res[m];
        if (rc == CRYO_OK && total > cap[m]) rc = CRYO_E_HIP; /* not a placement */
    }
    for (i = 0; rc == CRYO_OK && i < w->n; i++) {
        const CryoWalkBlock *e = &w->e[i];
        const CryoFetchPage *p = e->tag;
        uint32 q, nq = page_requests(p);
        if (e->method < 0) { say(j, p->block, e->reason, e->detail); continue; }
        for (q = 0; q < nq; q++) {
            const cryo_fetch_result *r = &res[e->method][first[e->method] + q];
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
        first[e->method] += nq;
    }
    for (m = 0; m < 2; m++) {
        cryo_walk_release(packed[m], cap[m]);
        free(res[m]);
    }
    return rc;
}

int cryo_fetch_tuples(CryoRel *rel, const CryoFetchPage *pages, size_t npages,
                      void (*tuple)(void *arg, const CryoFetchedTuple *t),
                      void (*report)(void *arg, const CryoFetchReport *r), void *arg, CryoFetchTotals *totals)
{
    const CryoWindowLimits limits = window;
    const uint32 max_chain = cryo_walk_max_chain();
    BlockNumber *chain = NULL, nblocks;
    Job j;
    CryoWindow w;
    size_t i;
    int rc;

    memset(&j, 0, sizeof j);
    if (totals) *totals = j.t;
    if (!rel || (!pages && npages)) return CRYO_E_ARG;
    j.ops = cryo_host_codec_ops();
    if (!j.ops) return CRYO_E_NODEV;
    j.fops = cryo_host_fetch_ops();
    if (!j.fops || !j.fops->fetch_blocks) return CRYO_E_UNSUPPORTED;
    j.tuple = tuple; j.report = report; j.arg = arg;
    nblocks = rel->ops->nblocks(rel->handle);
    rc = cryo_window_init(&w, limits, window_flush, &j);
    chain = malloc((size_t)max_chain * sizeof *chain);
    j.req_first = malloc(((size_t)limits.blocks + 1) * sizeof *j.req_first);
    if (!chain || !j.req_first) rc = CRYO_E_NOMEM;

    for (i = 0; rc == CRYO_OK && i < npages; i++) {
        const CryoFetchPage *p = &pages[i];
        CryoWalkBlock b;
        CryoError err;
        j.t.pages++;
        if (p->ntuples == 0) continue;
        if (p->ntuples > 0 && !p->offsets) { rc = CRYO_E_ARG; break; }
        /* the metapage and pages beyond the end are no chain starts (as cryo_read_data_batch treats them) */
        if (p->block == CRYO_META_PAGE || p->block >= nblocks) { j.t.not_block_starts++; continue; }
        err = cryo_walk_read(rel, p->block, chain, max_chain, &b);
        if (err == CRYO_ERR_WRONG_STARTING_BLOCK || err == CRYO_ERR_EMPTY_BLOCK) { j.t.not_block_starts++; continue; }
        b.tag = p;
        rc = cryo_window_add(&w, &b);
    }
    rc = cryo_window_finish(&w, rc);
    if (totals) *totals = j.t;
    cryo_window_free(&w);
    free(j.req_first); free(j.pos);
    free(chain);
    return rc;
}
