/*
 * host_walk_check.c -- the code the host walks share (pg_cryogen_amd/host/walk.h) at a window of 4 entries and 3.5 streams' bytes,
 * directly and under cryo_recompress_relation and cryo_fetch_tuples, whose windows no other test lowers.  A program of its own:
 * tests/test_host_walk.py builds it with walk.c, staging.c, storage.c, scan_iterator.c, recompress.c and fetch.c under
 * -DCRYO_HOST_TEST_HOOKS -fsanitize=address,undefined and expects exit 0.  compression.c is left out: what the walks take from it
 * is defined below and points at stub codec calls, so neither the codec library nor HIP is loaded.
 *
 * The relation (S = 100 bytes, byte limit 350, entry limit 4).  Stream c is filled with the byte 'A' + c, its xid is 100 + c.
 *
 *    c  method  size  what                                  window before -> after
 *    0  LZ4     100                                         {}           -> {0}          100
 *    1  zstd    100                                         {0}          -> {0 1}        200
 *    2  LZ4     100                                         {0 1}        -> {0 1 2}      300
 *    3  LZ4     100   400 > 350: FLUSH 0 before the add     {0 1 2}      -> {3}          100
 *       -- a new (empty) page: counted, no entry --
 *    4  LZ4     9000  claims 9000 bytes, has one page and
 *                     no next: unread, a slot, no bytes     {3}          -> {3 4}        100
 *    5  9       100   unknown method: a slot, no bytes      {3 4}        -> {3 4 5}      100
 *    6  LZ4     100   the fourth entry: FLUSH 1 after it    {3 4 5}      -> {3 4 5 6}    200 -> {}
 *    7  zstd    400   over the limit, but the window is
 *                     empty: no flush                       {}           -> {7}          400
 *    8  LZ4     100   500 > 350: FLUSH 2, stream 7 alone    {7}          -> {8}          100
 *    9  zstd    100                                         {8}          -> {8 9}        200
 *   10  9       200   unknown method, but a chain that was
 *                     read is weighed: 400 > 350, FLUSH 3;
 *                     it then adds no bytes                 {8 9}        -> {10}         0
 *   11  LZ4     100                                         {10}         -> {10 11}      100
 *   12  LZ4     100                                         {10 11}      -> {10 11 12}   200
 *       the end: FLUSH 4
 *
 * Codec calls, one per method present in a flush, LZ4 first: (LZ4, 2) (zstd, 1) | (LZ4, 2) | (zstd, 1) | (LZ4, 1) (zstd, 1) | (LZ4, 2).
 */
#include "fetch.h"
#include "recompress.h"
#include "cryo_codec.h"

#include <stdarg.h>
#include <stdio.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

enum { NCHAINS = 13, S = 100, W_BLOCKS = 4, W_BYTES = 350, UNKNOWN = 9, FAIL_STATUS = -77 };

static const int c_method[NCHAINS] = {0, 1, 0, 0, -1, -1, 0, 1, 0, 1, -1, 0, 0}; /* as the walk sorts them */
static const int c_written[NCHAINS] = {0, 1, 0, 0, 0, UNKNOWN, 0, 1, 0, 1, UNKNOWN, 0, 0};
static const uint32 c_size[NCHAINS] = {S, S, S, S, S, S, S, 4 * S, S, S, 2 * S, S, S};
static const uint32 c_reason[NCHAINS] = {0, 0, 0, 0, CRYO_CHECK_CHAIN, CRYO_CHECK_METHOD, 0, 0, 0, 0, CRYO_CHECK_METHOD, 0, 0};
static const uint32 c_detail[NCHAINS] = {0, 0, 0, 0, CRYO_ERR_DECOMPRESSION_FAILED, UNKNOWN, 0, 0, 0, 0, UNKNOWN, 0, 0};

/* the five flushes: their entries, each entry's slot in the call of its method (-1: in none), the calls' sizes, the bytes held */
enum { NFLUSH = 5, NCALLS = 7 };
static const struct { int n, chain[4], at[4]; size_t k[2]; Size bytes; } want_flush[NFLUSH] = {
    {3, {0, 1, 2}, {0, 0, 1}, {2, 1}, 300},
    {4, {3, 4, 5, 6}, {0, -1, -1, 1}, {2, 0}, 200},
    {1, {7}, {0}, {0, 1}, 400},
    {2, {8, 9}, {0, 0}, {1, 1}, 200},
    {3, {10, 11, 12}, {-1, 0, 1}, {2, 0}, 200},
};
static const struct { int method; size_t n; } want_call[NCALLS] = {{0, 2}, {1, 1}, {0, 2}, {1, 1}, {0, 1}, {1, 1}, {0, 2}};

/* ---- what the walks take from compression.c ---- */
Size cryo_blcksz = 16384; /* with the bound below: chains of up to three pages */
int cryo_gpu_count_guc = 1;
int lz4_acceleration_guc = 1;
int zstd_compression_level_guc = 1;

void cryo_compat_elog(int elevel, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    if (elevel >= ERROR) exit(1);
}

static size_t stub_bound(int method, size_t n) { (void)method; return n + 64; }
size_t cryo_host_codec_bound(int method, size_t n) { return stub_bound(method, n); }

static struct { int method; size_t n; } calls[16];
static int ncalls, fail_at; /* fail_at: the call, counted from 1, that fails with FAIL_STATUS; 0: none */

static int note_call(int method, size_t n)
{
    CHECK(ncalls < 16);
    calls[ncalls].method = method;
    calls[ncalls].n = n;
    return ++ncalls == fail_at ? FAIL_STATUS : CRYO_OK;
}

/* the new stream is the old one, packed at 16-byte steps; the decoders "reject" stream 8 */
static int stub_recode(void *ctx, int src_method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                       int dst_method, int dst_param, void *dst, size_t dst_cap, uint64_t *out_off, uint32_t *out_size, int32_t *status)
{
    size_t i, off = 0;
    const int rc = note_call(src_method, n);
    (void)ctx; (void)block_size; (void)dst_method; (void)dst_param;
    if (rc != CRYO_OK) return rc;
    for (i = 0; i < n; i++) {
        CHECK(off + src_size[i] <= dst_cap);
        memcpy((char *)dst + off, src[i], src_size[i]);
        out_off[i] = off;
        out_size[i] = src_size[i];
        status[i] = *(const char *)src[i] == 'A' + 8 ? CRYO_E_CORRUPT : CRYO_OK;
        off += (src_size[i] + 15) & ~(size_t)15;
    }
    return CRYO_OK;
}

/* a block has the positions 1 .. 3; a tuple is 8 bytes: its stream's first byte, its position, zeros */
static int stub_fetch(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                      const uint64_t *req_first, const uint16_t *pos, void *dst, size_t dst_cap, void *result, uint64_t *total)
{
    cryo_fetch_result *res = result;
    size_t i;
    uint64_t r, off = 0;
    const int rc = note_call(method, n);
    (void)ctx; (void)src_size; (void)block_size;
    if (rc != CRYO_OK) return rc;
    CHECK(req_first[0] == 0);
    for (i = 0; i < n; i++)
        for (r = req_first[i]; r < req_first[i + 1]; r++) {
            res[r].off = off;
            if (pos[r] > 3) { res[r].status = CRYO_FETCH_NOITEM; res[r].len = 0; continue; }
            CHECK(off + 8 <= dst_cap);
            memset((char *)dst + off, 0, 8);
            ((char *)dst)[off] = *(const char *)src[i];
            ((char *)dst)[off + 1] = (char)pos[r];
            res[r].status = CRYO_FETCH_OK;
            res[r].len = 8;
            off += 8;
        }
    *total = off;
    return CRYO_OK;
}

static const CryoCodecOps stub_ops = {.bound = stub_bound, .recode_blocks = stub_recode};
static const CryoCodecFetchOps stub_fetch_ops = {stub_fetch};
const CryoCodecOps *cryo_host_codec_ops(void) { return &stub_ops; }
const CryoCodecFetchOps *cryo_host_fetch_ops(void) { return &stub_fetch_ops; }

/* ---- the relation ---- */
static CryoMemRel *mem;
static CryoRel rel;
static BlockNumber first[NCHAINS], empty_page;

static void build_relation(void)
{
    BlockNumber chain[4];
    char buf[4 * S];
    int c, np;
    mem = cryo_memrel_create();
    cryo_memrel_bind(mem, 1, &rel);
    CHECK(cryo_memrel_nblocks(mem) == 1); /* the metapage */
    for (c = 0; c < NCHAINS; c++) {
        if (c == 4) empty_page = cryo_memrel_reserve(mem);
        first[c] = cryo_memrel_reserve(mem);
        memset(buf, 'A' + c, sizeof buf);
        CHECK(cryo_stage_write_chain(&rel, first[c], (CompressionMethod)c_written[c], 100 + c, buf, c_size[c], chain, 4, &np) == 0);
        CHECK(np == 1);
    }
    ((CryoFirstPageHeader *)cryo_memrel_page(mem, first[4]))->compressed_size = 9000;
    CHECK(cryo_memrel_nblocks(mem) == NCHAINS + 2);
}

static void calls_are_the_first(int n)
{
    int i;
    CHECK(ncalls == n);
    for (i = 0; i < n; i++) CHECK(calls[i].method == want_call[i].method && calls[i].n == want_call[i].n);
}

/* ---- (a), (b), (c): the window by itself ---- */
static int nflush;

static int recording_flush(void *arg, CryoWindow *w)
{
    int i, m;
    (void)arg;
    CHECK(nflush < NFLUSH);
    CHECK(w->n == want_flush[nflush].n && w->bytes == want_flush[nflush].bytes);
    for (m = 0; m < 2; m++) {
        const size_t k = cryo_window_gather(w, m);
        CHECK(k == want_flush[nflush].k[m]);
        for (i = 0; i < w->n; i++) {
            const CryoWalkBlock *e = &w->e[i];
            const int c = want_flush[nflush].chain[i];
            CHECK(e->block == first[c] && e->method == c_method[c] && e->xid == (TransactionId)(100 + c) && e->npages == 1);
            if (e->method < 0) CHECK(e->comp == NULL && e->reason == c_reason[c] && e->detail == c_detail[c]);
            if (e->method != m) continue;
            CHECK(e->csize == c_size[c] && e->comp[0] == 'A' + c && e->comp[e->csize - 1] == 'A' + c);
            CHECK(e->at == (size_t)want_flush[nflush].at[i] && w->src[e->at] == e->comp && w->src_size[e->at] == e->csize);
        }
        if (k && note_call(m, k) != CRYO_OK) { nflush++; return FAIL_STATUS; }
    }
    nflush++;
    return CRYO_OK;
}

static void test_window(void)
{
    const CryoWindowLimits limits = {W_BLOCKS, W_BYTES};
    static const int flushes_until_call[NCALLS + 1] = {NFLUSH, 1, 1, 2, 3, 4, 4, 5};
    uint64 blocks, empty_pages;
    for (fail_at = 0; fail_at <= NCALLS; fail_at++) {
        blocks = empty_pages = 0;
        ncalls = nflush = 0;
        CHECK(cryo_walk_windowed(&rel, limits, recording_flush, NULL, &blocks, &empty_pages) == (fail_at ? FAIL_STATUS : CRYO_OK));
        /* after the failure no further flush and no further call; what the window held and the pending stream are freed */
        CHECK(nflush == flushes_until_call[fail_at]);
        calls_are_the_first(fail_at ? fail_at : NCALLS);
        if (!fail_at) CHECK(blocks == NCHAINS && empty_pages == 1);
    }
    fail_at = 0;
    CHECK(cryo_walk_max_chain() == 3);
}

/* the clamp behind the cryo_*_set_window hooks */
static void test_limits(void)
{
    CryoWindowLimits l = cryo_window_limits(4, 350, 4096, (Size)256 << 20);
    CHECK(l.blocks == 4 && l.bytes == 350);
    l = cryo_window_limits(0, 0, 4096, (Size)256 << 20);
    CHECK(l.blocks == 4096 && l.bytes == (Size)256 << 20);
    l = cryo_window_limits(4096, (Size)256 << 20, 4096, (Size)256 << 20);
    CHECK(l.blocks == 4096 && l.bytes == (Size)256 << 20);
    l = cryo_window_limits(-1, 1, 4096, (Size)256 << 20);
    CHECK(l.blocks == 4096 && l.bytes == 1);
}

/* ---- (d): the same relation under the recompression and the fetch ---- */
typedef struct { char kind; BlockNumber block; uint32 a, b; } Event;
static Event events[64];
static int nevents;

static void note_event(char kind, BlockNumber block, uint32 a, uint32 b)
{
    CHECK(nevents < 64);
    events[nevents].kind = kind; events[nevents].block = block; events[nevents].a = a; events[nevents].b = b;
    nevents++;
}

static void on_moved(void *arg, BlockNumber old_first, BlockNumber new_first, uint32 old_np, uint32 new_np)
{
    (void)arg;
    CHECK(old_np == 1 && new_np == 1);
    note_event('M', old_first, new_first, 0);
}
static void on_check_report(void *arg, const CryoCheckReport *r)
{
    (void)arg;
    CHECK(r->npages == 1);
    note_event('R', r->block, r->reason, r->offset);
}

static void test_recompress(void)
{
    CryoRecompressTotals t;
    int c, i;
    for (fail_at = 0; fail_at <= 2; fail_at++) {
        CryoMemRel *dmem = cryo_memrel_create();
        CryoRel dst;
        BlockNumber next = 1;
        cryo_memrel_bind(dmem, 2, &dst);
        CHECK(cryo_memrel_nblocks(dmem) == 1); /* a fresh relation: its metapage */
        ncalls = nevents = 0;
        CHECK(cryo_recompress_relation(&rel, &dst, COMP_ZSTD, 3, on_moved, on_check_report, NULL, &t) == (fail_at ? FAIL_STATUS : CRYO_OK));
        calls_are_the_first(fail_at ? fail_at : NCALLS);
        if (fail_at) {                             /* the first flush failed: nothing was written or reported */
            CHECK(nevents == 0 && t.codec_calls == (uint64)fail_at && t.recoded == 0 && cryo_memrel_nblocks(dmem) == 1);
            cryo_memrel_destroy(dmem);
            continue;
        }
        /* every chain in walk order, the reports at their place: moved for the ones written, a report for the ones skipped, and
         * both for stream 8, which is copied as it was */
        for (c = 0, i = 0; c < NCHAINS; c++) {
            CHECK(i < nevents && events[i].block == first[c]);
            if (c_method[c] < 0) {
                CHECK(events[i].kind == 'R' && events[i].a == c_reason[c] && events[i].b == c_detail[c]);
                i++;
                continue;
            }
            CHECK(events[i].kind == 'M' && events[i].a == next);
            {
                const CryoFirstPageHeader *fh = (const CryoFirstPageHeader *)cryo_memrel_page(dmem, next);
                const char *payload = (const char *)fh + sizeof *fh;
                CHECK(fh->compressed_size == c_size[c] && fh->created_xid == (TransactionId)(100 + c));
                CHECK(fh->compression_method == (c == 8 ? COMP_LZ4 : COMP_ZSTD));
                CHECK(payload[0] == 'A' + c && payload[c_size[c] - 1] == 'A' + c);
            }
            next++;
            i++;
            if (c == 8) {
                CHECK(i < nevents && events[i].kind == 'R' && events[i].block == first[c]);
                CHECK(events[i].a == CRYO_CHECK_STREAM && events[i].b == 0xFFFFFFFFu);
                i++;
            }
        }
        CHECK(i == nevents && cryo_memrel_nblocks(dmem) == next);
        CHECK(t.blocks == NCHAINS && t.empty_pages == 1 && t.skipped == 3 && t.recoded == 9 && t.verbatim == 1);
        CHECK(t.codec_calls == NCALLS && t.bytes_in == 9 * S + 4 * S && t.bytes_out == t.bytes_in && t.pages_in == 10 && t.pages_out == 10);
        cryo_memrel_destroy(dmem);
    }
    fail_at = 0;
}

static void on_tuple(void *arg, const CryoFetchedTuple *t)
{
    (void)arg;
    CHECK(t->len == 8);
    note_event('T', t->block, t->pos, ((uint32)(unsigned char)t->data[0] << 8 | (uint32)(unsigned char)t->data[1]) + (t->created_xid << 16));
}
static void on_fetch_report(void *arg, const CryoFetchReport *r)
{
    (void)arg;
    note_event('R', r->block, r->reason, r->detail);
}

static void test_fetch(void)
{
    /* every chain start asks for positions 2 and 3, but chain 2, a lossy page, and chain 11, which asks for 3 and 4; between them
     * a page with no tuple, the metapage, the new page and a page beyond the end */
    static const uint16 two[2] = {2, 3}, late[2] = {3, 4};
    CryoFetchPage pages[NCHAINS + 4];
    CryoFetchTotals t;
    size_t np = 0;
    int c, i;
    pages[np].block = CRYO_META_PAGE; pages[np].ntuples = 2; pages[np++].offsets = two;
    for (c = 0; c < NCHAINS; c++) {
        if (c == 4) { pages[np].block = empty_page; pages[np].ntuples = -1; pages[np++].offsets = NULL; }
        pages[np].block = first[c];
        pages[np].ntuples = c == 2 ? -1 : 2;
        pages[np++].offsets = c == 2 ? NULL : c == 11 ? late : two;
        if (c == 6) { pages[np].block = first[c]; pages[np].ntuples = 0; pages[np++].offsets = NULL; }
    }
    pages[np].block = cryo_memrel_nblocks(mem); pages[np].ntuples = 2; pages[np++].offsets = two;
    CHECK(np == NCHAINS + 4);

    for (fail_at = 0; fail_at <= 2; fail_at++) {
        ncalls = nevents = 0;
        CHECK(cryo_fetch_tuples(&rel, pages, np, on_tuple, on_fetch_report, NULL, &t) == (fail_at ? FAIL_STATUS : CRYO_OK));
        calls_are_the_first(fail_at ? fail_at : NCALLS);
        if (fail_at) { CHECK(nevents == 0 && t.codec_calls == (uint64)fail_at && t.tuples == 0); continue; }
        for (c = 0, i = 0; c < NCHAINS; c++) {
            const uint32 tag = ((uint32)('A' + c) << 8) + ((uint32)(100 + c) << 16);
            if (c_method[c] < 0) {
                CHECK(i < nevents && events[i].kind == 'R' && events[i].block == first[c]);
                CHECK(events[i].a == c_reason[c] && events[i].b == c_detail[c]);
                i++;
                continue;
            }
            if (c == 2) {                          /* the lossy page: positions 1 .. 3, and its end is no report */
                int p;
                for (p = 1; p <= 3; p++, i++)
                    CHECK(i < nevents && events[i].kind == 'T' && events[i].block == first[c] && events[i].a == (uint32)p && events[i].b == tag + p);
                continue;
            }
            CHECK(i < nevents && events[i].kind == 'T' && events[i].block == first[c]);
            CHECK(events[i].a == (c == 11 ? 3u : 2u) && events[i].b == tag + events[i].a);
            i++;
            CHECK(i < nevents && events[i].block == first[c]);
            if (c == 11) CHECK(events[i].kind == 'R' && events[i].a == CRYO_FETCH_NOITEM && events[i].b == 4);
            else CHECK(events[i].kind == 'T' && events[i].a == 3 && events[i].b == tag + 3);
            i++;
        }
        CHECK(i == nevents);
        /* 10 streams: 9 pages of 2 requests and the lossy one's 290; 2 * 9 - 1 + 3 tuples of 8 bytes, 16 bytes per request */
        CHECK(t.pages == NCHAINS + 4 && t.not_block_starts == 3 && t.blocks == 10 && t.tuples == 20 && t.bad == 4);
        CHECK(t.codec_calls == NCALLS && t.bytes_back == 20 * 8 + (9 * 2 + 290) * 16);
    }
    fail_at = 0;
}

int main(void)
{
    build_relation();
    test_window();
    test_limits();
    cryo_recompress_set_window(W_BLOCKS, W_BYTES);
    cryo_fetch_set_window(W_BLOCKS, W_BYTES);
    test_recompress();
    test_fetch();
    cryo_memrel_destroy(mem);
    puts("host walk check ok");
    return 0;
}
