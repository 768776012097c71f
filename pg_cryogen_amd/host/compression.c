/*
 * compression.c -- cryo_compress / cryo_decompress over the MI355X codec C ABI.
 *
 * Mirrors reference compression.c:16-159: the three GUCs with the same names, ranges and
 * defaults (compression.c:24-58), palloc(bound) output owned by the caller
 * (pg_cryogen.c:826 pfrees it), elog(ERROR, "pg_cryogen: compression failed") on failure
 * (compression.c:73-74,105-106), `false` from cryo_decompress on malformed input
 * (compression.c:85-86,117-118), elog(ERROR) on an unknown method (compression.c:137,157).
 * Differences, all invisible to valid data: a block that decodes to fewer than CRYO_BLCKSZ
 * bytes returns false (the reference only Assert()s, compression.c:88,120).
 *
 * The GPU codec is opened lazily on first use, never in _PG_init: a library preloaded by the
 * postmaster must not create a HIP context before fork().  The C ABI never
 * longjmps; elog(ERROR) is raised here, in C, after the call returned.
 */
#include "compression.h"
#include "cryo_codec.h"
#ifdef CRYO_HAVE_POSTGRES
#include "utils/guc.h" /* DefineCustom*Variable, config_enum_entry, PGC_USERSET (reference compression.c:4) */
#endif

#include <stdarg.h>
#include <stdio.h>
#include <time.h>

int compression_method_guc = COMP_ZSTD;
int lz4_acceleration_guc = 1;
int zstd_compression_level_guc = 1;
int cryo_gpu_device_guc = 0;
int cryo_gpu_count_guc = 1;
int cryo_gpu_pool_mb_guc = 0;
int cryo_gpu_workspace_keep_mb_guc = 1024; /* device workspace a backend keeps between calls (-1: everything) */
int cryo_gpu_encode_segment_kb_guc = 0;    /* segment-parallel encode, KiB (0: the byte-identical encoders) */
int cryo_gpu_encode_segment_zstd_strategy_guc = 1; /* highest zstd strategy segment mode takes (1: `fast`) */
int cryo_gpu_verify_writes_guc = 0;       /* write verification (0: off) */
int cryo_gpu_zstd_checksum_guc = 0;       /* content checksums in the zstd frames the GPU writes (0: off) */
int cryo_gpu_readahead_blocks_guc = 8;    /* cryo blocks a sequential scan's cache miss decodes with one codec call (1: only the block asked for) */
Size cryo_blcksz = (Size)1 << 20; /* CRYO_BLCKSZ, reference storage.h:18 */

/* ---------------- codec binding ---------------- */
/* one handle per GPU of this backend: pg_cryogen.gpu_device is the first, pg_cryogen.gpu_count how many (consecutive
 * device numbers, wrapping).  With more than one, the K-block calls of the staging and cache code go through the
 * dispatcher of include/cryo_codec.h (block i of a call -> GPU i mod G, one host thread per GPU). */
static cryo_multi *hip_multi;
static int hip_multi_first = -1, hip_multi_count = 0, hip_pool_mb = 0, hip_keep_mb = -2, hip_seg_kb = 0,
           hip_seg_strategy = 1, hip_verify = 0, hip_zstd_checksum = 0;
/* A failed open is remembered until the GUCs change -- for good when the machine has no GPU (deterministic), for
 * CRYO_OPEN_RETRY_SECONDS when devices exist but cryo_multi_open failed (out of device memory, a busy device: transient;
 * a pooled backend must not refuse every cryo table for the rest of its life because of one bad moment). */
#define CRYO_OPEN_RETRY_SECONDS 5
static int hip_open_failed, hip_failed_first = -1, hip_failed_count = 0;
static time_t hip_failed_at; /* 0: the failure was deterministic */
static char codec_err[320];

static size_t hip_bound(int method, size_t n) { return cryo_codec_bound(method, n); }
static int hip_compress_blocks(void *ctx, int method, int param, const void *src, size_t bs, size_t n, void *dst,
                               size_t stride, uint32_t *out)
{
    return cryo_multi_compress_blocks((cryo_multi *)ctx, method, param, src, bs, n, dst, stride, out);
}
static int hip_decompress_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n,
                                 void *dst, size_t bs, int32_t *st)
{
    return cryo_multi_decompress_blocks((cryo_multi *)ctx, method, src, sz, n, dst, bs, st);
}

/* one destination per block: the decompressed-block cache hands its slots over (reference cache.c:46,178) */
static int hip_decompress_blocks_scatter(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n,
                                         void *const *dst, size_t bs, int32_t *st)
{
    return cryo_multi_decompress_blocks_to((cryo_multi *)ctx, method, src, sz, n, dst, bs, st);
}

static int hip_decompress_blocks_keyed(void *ctx, int method, const uint64_t *keys, const void *const *src, const uint32_t *sz,
                                       size_t n, void *const *dst, size_t bs, int32_t *st)
{
    return cryo_multi_decompress_blocks_keyed((cryo_multi *)ctx, method, keys, src, sz, n, dst, bs, st);
}
/* relid 0 (InvalidOid): PostgreSQL's relcache callback after a sinval-queue reset -- "anything may have changed": every entry */
static void hip_pool_invalidate(void *ctx, uint32_t relid) { (void)cryo_multi_pool_invalidate((cryo_multi *)ctx, relid, relid == 0u); }
static int hip_last_verify_failure(void *ctx, uint64_t *block, uint32_t *first_mismatch)
{
    return cryo_multi_last_verify_failure((cryo_multi *)ctx, block, first_mismatch);
}

static int hip_check_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs, uint32_t *result)
{
    return cryo_multi_check_blocks((cryo_multi *)ctx, method, src, sz, n, bs, (cryo_check_result *)result);
}

static int hip_recode_blocks(void *ctx, int src_method, const void *const *src, const uint32_t *sz, size_t n, size_t bs,
                             int dst_method, int dst_param, void *dst, size_t dst_cap, uint64_t *out_off, uint32_t *out_size,
                             int32_t *st)
{
    return cryo_multi_recode_blocks((cryo_multi *)ctx, src_method, src, sz, n, bs, dst_method, dst_param, dst, dst_cap, out_off,
                                    out_size, st);
}

static CryoCodecOps hip_ops = {hip_bound, hip_compress_blocks, hip_decompress_blocks, NULL, hip_decompress_blocks_scatter,
                               hip_decompress_blocks_keyed, hip_pool_invalidate, hip_last_verify_failure, hip_check_blocks,
                               hip_recode_blocks};
static const CryoCodecOps *bound_ops; /* CPU-only plumbing tests bind a double here (CRYO_HOST_TEST_HOOKS builds only) */

static int hip_fetch_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs,
                            const uint64_t *req_first, const uint16_t *pos, void *dst, size_t dst_cap, void *result, uint64_t *total)
{
    return cryo_multi_fetch_blocks((cryo_multi *)ctx, method, src, sz, n, bs, req_first, pos, dst, dst_cap,
                                   (cryo_fetch_result *)result, total);
}
static const CryoCodecFetchOps hip_fetch_ops = {hip_fetch_blocks};
static const CryoCodecFetchOps *bound_fetch_ops; /* the fetch table of a bound double (CRYO_HOST_TEST_HOOKS builds only) */

#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_codec_ops(const CryoCodecOps *ops) { bound_ops = ops; }
#endif
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_fetch_ops(const CryoCodecFetchOps *ops) { bound_fetch_ops = ops; }
#endif
const CryoCodecFetchOps *cryo_host_fetch_ops(void) { return bound_ops ? bound_fetch_ops : &hip_fetch_ops; }
static int hip_filter_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs,
                             const void *filter, void *dst, size_t dst_cap, void *rec, size_t rec_cap, void *blocks, uint64_t *total)
{
    return cryo_multi_filter_blocks((cryo_multi *)ctx, method, src, sz, n, bs, (const cryo_filter *)filter, dst, dst_cap,
                                    (cryo_filter_rec *)rec, rec_cap, (cryo_filter_block *)blocks, total);
}
static const CryoCodecFilterOps hip_filter_ops = {hip_filter_blocks};
static const CryoCodecFilterOps *bound_filter_ops; /* the filter table of a bound double (CRYO_HOST_TEST_HOOKS builds only) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_filter_ops(const CryoCodecFilterOps *ops) { bound_filter_ops = ops; }
#endif
const CryoCodecFilterOps *cryo_host_filter_ops(void) { return bound_ops ? bound_filter_ops : &hip_filter_ops; }
static int hip_agg_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs,
                          const void *filter, const void *agg, void *blocks, void *cells)
{
    return cryo_multi_agg_blocks((cryo_multi *)ctx, method, src, sz, n, bs, (const cryo_filter *)filter, (const cryo_agg *)agg,
                                 (cryo_agg_block *)blocks, (cryo_agg_cell *)cells);
}
static const CryoCodecAggOps hip_agg_ops = {hip_agg_blocks};
static const CryoCodecAggOps *bound_agg_ops; /* the aggregate table of a bound double (CRYO_HOST_TEST_HOOKS builds only) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_agg_ops(const CryoCodecAggOps *ops) { bound_agg_ops = ops; }
#endif
const CryoCodecAggOps *cryo_host_agg_ops(void) { return bound_ops ? bound_agg_ops : &hip_agg_ops; }
static int hip_group_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs,
                            const void *filter, const void *group, const void *agg, void *blocks, void *groups, size_t group_cap,
                            void *cells, uint64_t *total)
{
    return cryo_multi_group_blocks((cryo_multi *)ctx, method, src, sz, n, bs, (const cryo_filter *)filter, (const cryo_group *)group,
                                   (const cryo_agg *)agg, (cryo_group_block *)blocks, (cryo_group_rec *)groups, group_cap,
                                   (cryo_agg_cell *)cells, total);
}
static const CryoCodecGroupOps hip_group_ops = {hip_group_blocks};
static const CryoCodecGroupOps *bound_group_ops; /* the group table of a bound double (CRYO_HOST_TEST_HOOKS builds only) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_group_ops(const CryoCodecGroupOps *ops) { bound_group_ops = ops; }
#endif
const CryoCodecGroupOps *cryo_host_group_ops(void) { return bound_ops ? bound_group_ops : &hip_group_ops; }
static int hip_project_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs,
                              const void *filter, const void *project, void *rows, size_t row_cap, void *rec, size_t rec_cap,
                              void *blocks, uint64_t *total)
{
    return cryo_multi_project_blocks((cryo_multi *)ctx, method, src, sz, n, bs, (const cryo_filter *)filter,
                                     (const cryo_project *)project, rows, row_cap, (cryo_project_rec *)rec, rec_cap,
                                     (cryo_project_block *)blocks, total);
}
static const CryoCodecProjectOps hip_project_ops = {hip_project_blocks};
static const CryoCodecProjectOps *bound_project_ops; /* the project table of a bound double (CRYO_HOST_TEST_HOOKS builds only) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_project_ops(const CryoCodecProjectOps *ops) { bound_project_ops = ops; }
#endif
const CryoCodecProjectOps *cryo_host_project_ops(void) { return bound_ops ? bound_project_ops : &hip_project_ops; }
static int hip_topn_blocks(void *ctx, int method, const void *const *src, const uint32_t *sz, size_t n, size_t bs, const void *filter,
                           const void *order, const void *project, void *rows, void *rec, size_t row_cap, void *blocks, uint64_t *total)
{
    return cryo_multi_topn_blocks((cryo_multi *)ctx, method, src, sz, n, bs, (const cryo_filter *)filter, (const cryo_order *)order,
                                  (const cryo_project *)project, rows, (cryo_topn_rec *)rec, row_cap, (cryo_topn_block *)blocks, total);
}
static const CryoCodecTopnOps hip_topn_ops = {hip_topn_blocks};
static const CryoCodecTopnOps *bound_topn_ops; /* the topn table of a bound double (CRYO_HOST_TEST_HOOKS builds only) */
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_topn_ops(const CryoCodecTopnOps *ops) { bound_topn_ops = ops; }
#endif
const CryoCodecTopnOps *cryo_host_topn_ops(void) { return bound_ops ? bound_topn_ops : &hip_topn_ops; }
const char *cryo_host_codec_error(void) { return codec_err; }

const CryoCodecOps *cryo_host_codec_ops(void)
{
    if (bound_ops) return bound_ops;
    if (hip_multi && (hip_multi_first != cryo_gpu_device_guc || hip_multi_count != cryo_gpu_count_guc)) {
        cryo_multi_close(hip_multi); /* the GUCs changed: rebind */
        hip_multi = NULL;
    }
    if (!hip_multi) {
        int devs[64], i, ndev, rc;
        int cnt = cryo_gpu_count_guc < 1 ? 1 : (cryo_gpu_count_guc > 64 ? 64 : cryo_gpu_count_guc);
        /* not again for every call of a backend that cannot have a GPU (codec_err still says why) */
        if (hip_open_failed && hip_failed_first == cryo_gpu_device_guc && hip_failed_count == cryo_gpu_count_guc &&
            (hip_failed_at == 0 || time(NULL) - hip_failed_at < CRYO_OPEN_RETRY_SECONDS))
            return NULL;
        hip_open_failed = 1;
        hip_failed_at = 0;
        hip_failed_first = cryo_gpu_device_guc;
        hip_failed_count = cryo_gpu_count_guc;
        ndev = cryo_codec_device_count();
        if (ndev <= 0) {
            snprintf(codec_err, sizeof codec_err, "no GPU visible to the HIP runtime (%d; no CPU fallback)", ndev);
            return NULL;
        }
        for (i = 0; i < cnt; i++) devs[i] = (cryo_gpu_device_guc + i) % ndev;
        rc = cryo_multi_open(devs, cnt, &hip_multi);
        if (rc != CRYO_OK) {
            snprintf(codec_err, sizeof codec_err, "cryo_multi_open(first %d, count %d) failed with %d (no CPU fallback)",
                     cryo_gpu_device_guc, cnt, rc);
            hip_multi = NULL;
            hip_failed_at = time(NULL); /* devices exist: try again in a while */
            if (hip_failed_at == 0) hip_failed_at = 1;
            return NULL;
        }
        hip_open_failed = 0;
        hip_multi_first = cryo_gpu_device_guc;
        hip_multi_count = cryo_gpu_count_guc;
        hip_pool_mb = 0;
        hip_keep_mb = -2;
        hip_seg_kb = 0;
        hip_seg_strategy = 1;
        hip_verify = 0;
        hip_zstd_checksum = 0;
        hip_ops.ctx = hip_multi;
    }
    if (hip_keep_mb != cryo_gpu_workspace_keep_mb_guc) { /* a backend is long-lived: one large call must not pin its workspace for good */
        hip_keep_mb = cryo_gpu_workspace_keep_mb_guc;
        (void)cryo_multi_set_option(hip_multi, CRYO_OPT_WORKSPACE_KEEP_BYTES, hip_keep_mb < 0 ? -1 : (int64_t)hip_keep_mb << 20);
    }
    if (hip_pool_mb != cryo_gpu_pool_mb_guc) { /* the GUC changed: resize (0 frees the pool) */
        hip_pool_mb = cryo_gpu_pool_mb_guc;
        (void)cryo_multi_set_option(hip_multi, CRYO_OPT_POOL_BYTES, (int64_t)(hip_pool_mb < 0 ? 0 : hip_pool_mb) << 20);
    }
    if (hip_seg_kb != cryo_gpu_encode_segment_kb_guc && cryo_encode_segment_kb_valid(cryo_gpu_encode_segment_kb_guc)) {
        hip_seg_kb = cryo_gpu_encode_segment_kb_guc; /* a value the option refuses is never stored: the encoders stay as they are */
        (void)cryo_multi_set_option(hip_multi, CRYO_OPT_ENCODE_SEGMENT_BYTES, (int64_t)hip_seg_kb << 10);
    }
    if (hip_seg_strategy != cryo_gpu_encode_segment_zstd_strategy_guc &&
        cryo_encode_segment_zstd_strategy_valid(cryo_gpu_encode_segment_zstd_strategy_guc)) {
        hip_seg_strategy = cryo_gpu_encode_segment_zstd_strategy_guc;
        (void)cryo_multi_set_option(hip_multi, CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, (int64_t)hip_seg_strategy);
    }
    if (hip_verify != (cryo_gpu_verify_writes_guc != 0)) {
        hip_verify = cryo_gpu_verify_writes_guc != 0;
        (void)cryo_multi_set_option(hip_multi, CRYO_OPT_ENCODE_VERIFY, (int64_t)hip_verify);
    }
    if (hip_zstd_checksum != (cryo_gpu_zstd_checksum_guc != 0)) {
        hip_zstd_checksum = cryo_gpu_zstd_checksum_guc != 0;
        (void)cryo_multi_set_option(hip_multi, CRYO_OPT_ZSTD_CHECKSUM, (int64_t)hip_zstd_checksum);
    }
    return &hip_ops;
}

/* worst-case compressed size of a block: pure arithmetic (cryo_codec_bound), no GPU -- the cache sizes its chain lists with
 * it at _PG_init (cryo_init_cache, reference pg_cryogen.c:172), long before a backend may ever touch a cryo table */
size_t cryo_host_codec_bound(int method, size_t n)
{
    if (bound_ops) return bound_ops->bound(method, n);
    return cryo_codec_bound(method, n);
}

/* The binding if this backend has one already -- never opens the GPU.  For the relcache invalidation callback
 * (cryo_cache_invalidate_relation), which PostgreSQL fires for every invalidation of any relation in every backend that
 * loaded the extension: a backend that never touched a cryo table must not pay a HIP context for a sinval message. */
const CryoCodecOps *cryo_host_codec_ops_if_open(void)
{
    if (bound_ops) return bound_ops;
    return hip_multi ? &hip_ops : NULL;
}

void cryo_host_transfer_counters(uint64_t *h2d_bytes, uint64_t *d2h_bytes, uint64_t *pool_hits, uint64_t *pool_misses)
{
    cryo_codec_transfer_counters t = {0, 0, 0, 0, 0, 0};
    if (hip_multi) (void)cryo_multi_get_transfer_counters(hip_multi, &t);
    if (h2d_bytes) *h2d_bytes = t.h2d_bytes;
    if (d2h_bytes) *d2h_bytes = t.d2h_bytes;
    if (pool_hits) *pool_hits = t.pool_hits;
    if (pool_misses) *pool_misses = t.pool_misses;
}

/* idle backend: give the GPU memory of the binding back (device workspace, staging buffers; not the pool) */
void cryo_host_codec_trim(void)
{
    if (hip_multi) (void)cryo_multi_trim(hip_multi);
}

/* ---------------- GUCs ---------------- */
/* pg_cryogen.gpu_encode_segment_kb: 0, or a power of two from 4 to 128 (CRYO_OPT_ENCODE_SEGMENT_BYTES) */
int cryo_encode_segment_kb_valid(int kb)
{
    return kb == 0 || (kb >= 4 && kb <= 128 && (kb & (kb - 1)) == 0);
}
/* pg_cryogen.gpu_encode_segment_zstd_strategy: libzstd's ZSTD_strategy number, 1 (`fast`) .. 6 (`btlazy2`)
 * (CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY) */
int cryo_encode_segment_zstd_strategy_valid(int strategy)
{
    return strategy >= 1 && strategy <= 6;
}
#ifdef CRYO_HAVE_POSTGRES
static bool check_encode_segment_kb(int *newval, void **extra, GucSource source)
{
    (void)extra;
    (void)source;
    return cryo_encode_segment_kb_valid(*newval) != 0; /* false: "invalid value for parameter" */
}
#endif

void cryo_define_compression_gucs(void)
{
#ifdef CRYO_HAVE_POSTGRES
    static const struct config_enum_entry compression_method_options[] = {
        {"lz4", COMP_LZ4, false}, {"zstd", COMP_ZSTD, false}, {NULL, 0, false}};
    DefineCustomEnumVariable("pg_cryogen.compression_method", "Possible values are lz4 and zstd.", NULL,
                             &compression_method_guc, COMP_ZSTD, compression_method_options, PGC_USERSET, 0,
                             NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.lz4_acceleration", "Sets lz4 acceleration.", NULL,
                            &lz4_acceleration_guc, 1, 0, 50, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.zstd_compression_level", "Sets zstd compression level.", NULL,
                            &zstd_compression_level_guc, 1, -5, 22, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.gpu_device", "GPU used by this backend.", NULL, &cryo_gpu_device_guc, 0,
                            0, 63, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.gpu_count", "Number of GPUs (from gpu_device on) the K-block calls of this backend are spread over.",
                            NULL, &cryo_gpu_count_guc, 1, 1, 64, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.gpu_pool_mb", "Decoded blocks kept in GPU memory so that repeated scans skip the transfer and the decode (MiB, 0 = off).",
                            NULL, &cryo_gpu_pool_mb_guc, 0, 0, 262144, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.gpu_workspace_keep_mb", "GPU workspace this backend keeps between codec calls (MiB; -1 = everything a call ever needed).",
                            NULL, &cryo_gpu_workspace_keep_mb_guc, 1024, -1, 262144, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.gpu_readahead_blocks",
                            "Cryo blocks a sequential scan's cache miss decodes with one codec call (1 = only the block asked for).",
                            NULL, &cryo_gpu_readahead_blocks_guc, 8, 1, 64, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomIntVariable("pg_cryogen.gpu_encode_segment_kb",
                            "Segment size (KiB) of the segment-parallel GPU encoders: each segment of a block gets its own wave "
                            "(0 = the encoders whose output equals liblz4's / libzstd's; 4 .. 128, a power of two = valid streams "
                            "the stock libraries decode, but not byte-identical to theirs).",
                            NULL, &cryo_gpu_encode_segment_kb_guc, 0, 0, 128, PGC_USERSET, 0, check_encode_segment_kb,
                            NULL, NULL);
    static const struct config_enum_entry encode_segment_zstd_strategy_options[] = {
        {"fast", 1, false}, {"dfast", 2, false}, {"greedy", 3, false}, {"lazy", 4, false},
        {"lazy2", 5, false}, {"btlazy2", 6, false}, {NULL, 0, false}};
    DefineCustomEnumVariable("pg_cryogen.gpu_encode_segment_zstd_strategy",
                             "Deepest zstd strategy the segment-parallel GPU encoder takes when gpu_encode_segment_kb is set "
                             "(fast = levels up to 2 only, as before; dfast .. btlazy2 = deeper levels too, whose output then "
                             "stops being byte-identical to libzstd's).",
                             NULL, &cryo_gpu_encode_segment_zstd_strategy_guc, 1, encode_segment_zstd_strategy_options,
                             PGC_USERSET, 0, NULL, NULL, NULL);
    /* a boolean, spelt as PostgreSQL's own on/off enums are (synchronous_commit, huge_pages).  The hidden entries are every
     * other spelling parse_bool() takes -- true / false / yes / no and their unique prefixes, "of", 1 / 0 -- so that any value
     * a bool GUC accepts is accepted here too (enum names match case-insensitively, as bool values do) */
    static const struct config_enum_entry verify_writes_options[] = {
        {"off", 0, false}, {"on", 1, false},
        {"true", 1, true}, {"tru", 1, true}, {"tr", 1, true}, {"t", 1, true},
        {"false", 0, true}, {"fals", 0, true}, {"fal", 0, true}, {"fa", 0, true}, {"f", 0, true},
        {"yes", 1, true}, {"ye", 1, true}, {"y", 1, true}, {"no", 0, true}, {"n", 0, true},
        {"of", 0, true}, {"1", 1, true}, {"0", 0, true}, {NULL, 0, false}};
    DefineCustomEnumVariable("pg_cryogen.gpu_verify_writes",
                             "Decode every block the GPU compressed and compare it with the input before it is written "
                             "(a block that fails raises ERROR, so the transaction aborts before any page is written).",
                             NULL, &cryo_gpu_verify_writes_guc, 0, verify_writes_options, PGC_USERSET, 0, NULL, NULL, NULL);
    DefineCustomEnumVariable("pg_cryogen.zstd_checksum",
                             "Write a content checksum into every zstd frame the GPU compresses (stock zstd and every GPU decode "
                             "route check it on each read; off = the frames libzstd writes by default).",
                             NULL, &cryo_gpu_zstd_checksum_guc, 0, verify_writes_options, PGC_USERSET, 0, NULL, NULL, NULL);
#else
    /* no GUC machinery without PostgreSQL: the variables keep the reference's defaults */
    compression_method_guc = COMP_ZSTD;
    lz4_acceleration_guc = 1;
    zstd_compression_level_guc = 1;
#endif
}

/* ---------------- the two calls ---------------- */
static int method_param(CompressionMethod method)
{
    return method == COMP_LZ4 ? lz4_acceleration_guc : zstd_compression_level_guc;
}

char *cryo_compress(CompressionMethod method, const char *data, Size *compressed_size)
{
    const CryoCodecOps *ops;
    Size estimate;
    char *compressed;
    uint32_t csize = 0;
    int rc;

    if (method != COMP_LZ4 && method != COMP_ZSTD)
        elog(ERROR, "pg_cryogen: unknown compression method");
    ops = cryo_host_codec_ops();
    if (!ops)
        elog(ERROR, "pg_cryogen: compression failed (%s)", codec_err);
    estimate = ops->bound((int)method, cryo_blcksz);
    compressed = palloc(estimate);
    rc = ops->compress_blocks(ops->ctx, (int)method, method_param(method), data, cryo_blcksz, 1, compressed,
                              estimate, &csize);
    if (rc != 0 || csize == 0) {
        uint64_t vblock = 0;
        uint32_t voff = 0xFFFFFFFFu;
        pfree(compressed);
        if (rc == CRYO_E_VERIFY) {   /* pg_cryogen.gpu_verify_writes: the block never reaches a page */
            if (ops->last_verify_failure && ops->last_verify_failure(ops->ctx, &vblock, &voff) == 1 && voff != 0xFFFFFFFFu)
                elog(ERROR, "pg_cryogen: compressed block failed verification at byte %u", voff);
            else
                elog(ERROR, "pg_cryogen: compressed block failed verification (its stream does not decode)");
        } else if (rc == CRYO_E_UNSUPPORTED)   /* same ERROR as the reference, with the reason (this build has no kernel for it) */
            elog(ERROR, "pg_cryogen: compression failed (no GPU kernel for %s parameter %d at block size %lu)",
                 method == COMP_LZ4 ? "lz4" : "zstd", method_param(method), (unsigned long)cryo_blcksz);
        else
            elog(ERROR, "pg_cryogen: compression failed");
        return NULL;
    }
    *compressed_size = csize;
    return compressed;
}

bool cryo_decompress(CompressionMethod method, const char *compressed, Size compressed_size, char *out)
{
    const CryoCodecOps *ops;
    const void *srcs[1];
    uint32_t sizes[1];
    int32_t status[1] = {0};
    int rc;

    if (method != COMP_LZ4 && method != COMP_ZSTD)
        elog(ERROR, "pg_cryogen: unknown compression method");
    if (compressed_size == 0 || compressed_size > 0xFFFFFFFFu)
        return false;
    ops = cryo_host_codec_ops();
    if (!ops)
        elog(ERROR, "pg_cryogen: decompression unavailable (%s)", codec_err);
    srcs[0] = compressed;
    sizes[0] = (uint32_t)compressed_size;
    rc = ops->decompress_blocks(ops->ctx, (int)method, srcs, sizes, 1, out, cryo_blcksz, status);
    if (rc != 0)
        elog(ERROR, "pg_cryogen: decompression failed to run (%d)", rc);
    return status[0] == 0;
}

#ifndef CRYO_HAVE_POSTGRES
/* ---------------- pg_compat: elog ---------------- */
static cryo_error_handler err_handler;
void cryo_compat_set_error_handler(cryo_error_handler h) { err_handler = h; }
void cryo_compat_elog(int elevel, const char *fmt, ...)
{
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    if (err_handler) { err_handler(elevel, msg); return; }
    if (elevel >= ERROR) { fprintf(stderr, "ERROR: %s\n", msg); abort(); }
}
#endif
