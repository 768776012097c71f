/*
 * topn_merge_check.c -- the merge of the ordered scan (pg_cryogen_amd/host/topn.h: cryo_topn_merge_init / _add / _finish / _free)
 * on crafted records.  A program of its own: tests/test_topn_cpu.py builds it with topn.c, walk.c, staging.c, storage.c and
 * scan_iterator.c under -fsanitize=address,undefined and expects exit 0.  compression.c is left out: what the walks take from it
 * is defined below, no codec is bound, so neither the codec library nor HIP is loaded, and cryo_topn_scan answers CRYO_E_NODEV.
 *
 * A record is written {key 1, key 2, key_nulls}; its row is 8 bytes: the block's number, the record's rank in the block, zeros.
 * Each block is in its own order, as the codec hands it over.  The expected merges are worked out by hand at each case.
 */
#include "topn.h"

#include <stdarg.h>
#include <stdio.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

/* ---- what the walks take from compression.c ---- */
Size cryo_blcksz = 16384;
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
size_t cryo_host_codec_bound(int method, size_t n) { (void)method; return n + 64; }
const CryoCodecOps *cryo_host_codec_ops(void) { return NULL; }
const CryoCodecTopnOps *cryo_host_topn_ops(void) { return NULL; }

typedef struct { int64_t k0, k1; unsigned nulls; } Key;

/* adds block `b` of n keys (in the block's order) */
static void add(CryoTopnMerge *m, int b, const Key *keys, uint32 n)
{
    cryo_topn_rec *rec = malloc((n ? n : 1) * sizeof *rec); /* exactly n: a read past the block is the sanitizer's */
    char *rows = malloc((n ? n : 1) * 8);
    uint32 i;
    CHECK(rec && rows);
    for (i = 0; i < n; i++) {
        memset(&rec[i], 0, sizeof rec[i]);
        rec[i].key[0] = keys[i].k0;
        rec[i].key[1] = keys[i].k1;
        rec[i].key_nulls = (uint16_t)keys[i].nulls;
        rec[i].pos = (uint16_t)(i + 1);
        memset(rows + 8 * i, 0, 8);
        rows[8 * i] = (char)b;
        rows[8 * i + 1] = (char)i;
    }
    CHECK(cryo_topn_merge_add(m, n ? rec : NULL, n ? rows : NULL, n) == CRYO_OK);
    free(rec);
    free(rows);
}

/* the merge holds exactly the n rows (block, rank) of want, in order, and each record is its row's */
static void holds(const CryoTopnMerge *m, const int (*want)[2], uint32 n)
{
    const cryo_topn_rec *rec;
    const void *rows;
    uint32 i;
    CHECK(cryo_topn_merge_finish(m, &rec, &rows) == n);
    for (i = 0; i < n; i++) {
        const char *row = (const char *)rows + 8 * i;
        if (row[0] != want[i][0] || row[1] != want[i][1]) {
            fprintf(stderr, "place %u: block %d rank %d, expected block %d rank %d\n", i, row[0], row[1], want[i][0], want[i][1]);
            exit(1);
        }
        CHECK(rec[i].pos == want[i][1] + 1);
    }
}

static cryo_order order_of(cryo_order_col *by, uint32 nby, uint8_t f0, uint8_t f1)
{
    cryo_order o;
    memset(by, 0, 2 * sizeof *by);
    by[0].att = 1; by[0].type = CRYO_KEY_INT8; by[0].flags = f0;
    by[1].att = 2; by[1].type = CRYO_KEY_INT8; by[1].flags = f1;
    o.nby = nby; o.limit = 1; o.by = by;
    return o;
}

int main(void)
{
    cryo_order_col by[2];
    cryo_order o;
    CryoTopnMerge m;

    /* one column ascending; ties across blocks go to the block added earlier, then to the block's order */
    {
        const Key b0[] = {{1, 0, 0}, {5, 0, 0}, {5, 0, 0}}, b1[] = {{0, 0, 0}, {5, 0, 0}, {9, 0, 0}}, b2[] = {{5, 0, 0}};
        const int all[][2] = {{1, 0}, {0, 0}, {0, 1}, {0, 2}, {1, 1}, {2, 0}, {1, 2}};
        o = order_of(by, 1, 0, 0);
        CHECK(cryo_topn_merge_init(&m, &o, 1000, 8) == CRYO_OK); /* fewer rows than the limit */
        add(&m, 0, b0, 3); add(&m, 1, b1, 3); add(&m, 9, NULL, 0); add(&m, 2, b2, 1);
        holds(&m, all, 7);
        cryo_topn_merge_free(&m);
        CHECK(cryo_topn_merge_init(&m, &o, 4, 8) == CRYO_OK);    /* the cut falls between ties: the earlier block's stay */
        add(&m, 0, b0, 3); add(&m, 1, b1, 3); add(&m, 2, b2, 1);
        holds(&m, all, 4);
        cryo_topn_merge_free(&m);
        CHECK(cryo_topn_merge_init(&m, &o, 1, 8) == CRYO_OK);
        add(&m, 0, b0, 3); add(&m, 1, b1, 3);
        holds(&m, all, 1);
        cryo_topn_merge_free(&m);
        holds(&m, all, 0);                                        /* freed: empty, and free again is harmless */
        cryo_topn_merge_free(&m);
    }
    /* DESC over the extremes: the complement, not the negation.  NULLs last whatever the direction */
    {
        const Key b0[] = {{INT64_MAX, 0, 0}, {0, 0, 0}, {INT64_MIN, 0, 0}, {0, 0, 1}}, b1[] = {{1, 0, 0}, {-1, 0, 0}, {0, 0, 1}};
        const int want[][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {0, 2}, {0, 3}, {1, 2}};
        o = order_of(by, 1, CRYO_ORDER_DESC, 0);
        CHECK(cryo_topn_merge_init(&m, &o, 290, 8) == CRYO_OK);
        add(&m, 0, b0, 4); add(&m, 1, b1, 3);
        holds(&m, want, 7);
        cryo_topn_merge_free(&m);
    }
    /* NULLS FIRST ascending, and a second column DESC that decides within equal first keys (a NULL's key is 0 and is not compared) */
    {
        const Key b0[] = {{0, 7, 1}, {2, 9, 0}, {2, 3, 0}}, b1[] = {{0, 8, 1}, {2, 9, 0}, {2, 0, 2}, {3, 0, 0}};
        /* first keys: NULL, NULL | 2 with second keys 9 (b0), 9 (b1), 3, then NULL last | 3 */
        const int want[][2] = {{1, 0}, {0, 0}, {0, 1}, {1, 1}, {0, 2}, {1, 2}, {1, 3}};
        o = order_of(by, 2, CRYO_ORDER_NULLS_FIRST, CRYO_ORDER_DESC);
        CHECK(cryo_topn_merge_init(&m, &o, 291, 8) == CRYO_OK);
        add(&m, 0, b0, 3); add(&m, 1, b1, 4);
        holds(&m, want, 7);
        cryo_topn_merge_free(&m);
    }
    /* arguments */
    o = order_of(by, 1, 0, 0);
    CHECK(cryo_topn_merge_init(&m, &o, 0, 8) == CRYO_E_ARG && cryo_topn_merge_init(&m, &o, 1, 12) == CRYO_E_ARG);
    CHECK(cryo_topn_merge_init(&m, &o, 1, 0) == CRYO_E_ARG && cryo_topn_merge_init(NULL, &o, 1, 8) == CRYO_E_ARG);
    CHECK(cryo_topn_merge_init(&m, NULL, 1, 8) == CRYO_E_ARG);
    o = order_of(by, 3, 0, 0);
    CHECK(cryo_topn_merge_init(&m, &o, 1, 8) == CRYO_E_ARG);
    o = order_of(by, 1, 4, 0);
    CHECK(cryo_topn_merge_init(&m, &o, 1, 8) == CRYO_E_ARG);
    CHECK(cryo_topn_merge_add(&m, NULL, NULL, 1) == CRYO_E_ARG);  /* a merge that was never set up takes nothing */
    /* no codec is bound here */
    {
        CryoRel rel;
        cryo_filter f;
        cryo_project p;
        memset(&rel, 0, sizeof rel); memset(&f, 0, sizeof f); memset(&p, 0, sizeof p);
        o = order_of(by, 1, 0, 0);
        CHECK(cryo_topn_scan(&rel, &f, &o, &p, NULL, NULL, NULL, NULL) == CRYO_E_NODEV);
        CHECK(cryo_topn_scan(&rel, &f, NULL, &p, NULL, NULL, NULL, NULL) == CRYO_E_ARG);
    }
    puts("topn merge check ok");
    return 0;
}
