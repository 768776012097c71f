/*
 * compression.h -- host-side mirror of the reference's codec boundary
 * (reference compression.h:7-24): same type, same three GUC variables, same three
 * functions with the same argument meaning, ownership and error behaviour
 * (SURVEY.md section 8b).  pg_cryogen.c:726 and cache.c:178 call it unchanged.
 *
 * Underneath, instead of liblz4/libzstd, it drives the MI355X codec through the C ABI
 * (include/cryo_codec.h).
 */
#ifndef __COMPRESSION_H__
#define __COMPRESSION_H__

#ifdef CRYO_HAVE_POSTGRES
#include "postgres.h"
#else
#include "pg_compat.h"
#endif

typedef enum
{
    COMP_LZ4 = 0,
    COMP_ZSTD
} CompressionMethod;

extern int compression_method_guc;
extern int lz4_acceleration_guc;
extern int zstd_compression_level_guc;

extern char *cryo_compress(CompressionMethod method,
                           const char *data,
                           Size *compressed_size);
extern bool cryo_decompress(CompressionMethod method,
                            const char *compressed,
                            Size compressed_size,
                            char *out);
extern void cryo_define_compression_gucs(void);

/* ---- additions (not in the reference) ---- */

/* the reference hard-codes CRYO_BLCKSZ = 1 MiB (storage.h:18); here it is a run-time value
 * with the same default so the benchmark's 128 KiB blocks use the same code */
extern Size cryo_blcksz;
/* GPU used by this backend (additive GUC pg_cryogen.gpu_device, default 0) */
extern int cryo_gpu_device_guc;
/* how many GPUs, from gpu_device on, the K-block calls are spread over (additive GUC pg_cryogen.gpu_count, default 1) */
extern int cryo_gpu_count_guc;
/* device-resident pool of decoded blocks, MiB over all GPUs of the backend (additive GUC pg_cryogen.gpu_pool_mb, default 0 = off) */
extern int cryo_gpu_pool_mb_guc;
extern int cryo_gpu_workspace_keep_mb_guc; /* pg_cryogen.gpu_workspace_keep_mb (default 1024, -1 = keep everything) */
/* pg_cryogen.gpu_encode_segment_kb (default 0 = the byte-identical encoders; 4 .. 128, a power of two: segment-parallel
 * encode, CRYO_OPT_ENCODE_SEGMENT_BYTES -- for the write path's one-block calls) */
extern int cryo_gpu_encode_segment_kb_guc;
int cryo_encode_segment_kb_valid(int kb);
/* pg_cryogen.gpu_encode_segment_zstd_strategy (enum fast, dfast, greedy, lazy, lazy2, btlazy2 = 1 .. 6, default fast): the
 * deepest zstd strategy segment mode takes (CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY; no effect while the segment size is 0) */
extern int cryo_gpu_encode_segment_zstd_strategy_guc;
int cryo_encode_segment_zstd_strategy_valid(int strategy);
/* pg_cryogen.gpu_verify_writes (on/off, default off): every compress call decodes what the GPU encoded and compares it with
 * the input before the block is handed back (CRYO_OPT_ENCODE_VERIFY); a block that fails raises ERROR */
extern int cryo_gpu_verify_writes_guc;
/* pg_cryogen.zstd_checksum (on/off, default off): every zstd frame the GPU writes carries a content checksum, which stock
 * ZSTD_decompress and the GPU decoders check on every read (CRYO_OPT_ZSTD_CHECKSUM); no effect on LZ4 */
extern int cryo_gpu_zstd_checksum_guc;
extern int cryo_gpu_readahead_blocks_guc;  /* pg_cryogen.gpu_readahead_blocks (default 8, 1 = off): host/cache.c, cryo_read_data_rel */
/* bytes the codec moved towards the device / back, blocks served from the pool / decoded (0 when no GPU codec is bound) */
void cryo_host_transfer_counters(uint64_t *h2d_bytes, uint64_t *d2h_bytes, uint64_t *pool_hits, uint64_t *pool_misses);

/* the codec entry points the host side calls; production binds them to libcryo_codec.so
 * (include/cryo_codec.h), CPU-only plumbing tests may bind a test double */
typedef struct CryoCodecOps {
    size_t (*bound)(int method, size_t block_size);
    int (*compress_blocks)(void *ctx, int method, int param, const void *src, size_t block_size, size_t n,
                           void *dst, size_t dst_stride, uint32_t *out_size);
    int (*decompress_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n,
                             void *dst, size_t block_size, int32_t *status);
    void *ctx;
    /* optional (may be NULL): one destination per block, so the cache decodes straight into its slots */
    int (*decompress_blocks_scatter)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n,
                                     void *const *dst, size_t block_size, int32_t *status);
    /* optional (may be NULL): the same with a key per block (relation oid << 32 | first block number): a codec with a
     * device-resident pool (pg_cryogen.gpu_pool_mb) serves a block it still holds from HBM -- nothing crosses PCIe towards
     * the device, no kernel runs for it */
    int (*decompress_blocks_keyed)(void *ctx, int method, const uint64_t *keys, const void *const *src, const uint32_t *src_size,
                                   size_t n, void *const *dst, size_t block_size, int32_t *status);
    /* optional (may be NULL): forget the pooled blocks of a relation (reference: relcache callback, pg_cryogen.c:163-167) */
    void (*pool_invalidate)(void *ctx, uint32_t relid);
    /* optional (may be NULL): after compress_blocks returned CRYO_E_VERIFY, the failing block and its first differing byte
     * (0xFFFFFFFF: the decoders reject its stream); 1 when there is one (cryo_multi_last_verify_failure) */
    int (*last_verify_failure)(void *ctx, uint64_t *block, uint32_t *first_mismatch);
    /* optional (may be NULL): the stored-block check of n streams (cryo_multi_check_blocks): result[2i], result[2i + 1] =
     * block i's {reason, offset} (cryo_check_result); check.h, cryo_check_relation, needs it */
    int (*check_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                        uint32_t *result);
    /* optional (may be NULL): recompression of n streams on the device (cryo_multi_recode_blocks): stream i is decoded and
     * encoded with (dst_method, dst_param); the new stream is the out_size[i] bytes at dst + out_off[i] (packed at 16-byte
     * steps, only compressed bytes cross PCIe), status[i] its cryo_status; recompress.h, cryo_recompress_relation, needs it */
    int (*recode_blocks)(void *ctx, int src_method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                         int dst_method, int dst_param, void *dst, size_t dst_cap, uint64_t *out_off, uint32_t *out_size,
                         int32_t *status);
} CryoCodecOps;
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_codec_ops(const CryoCodecOps *ops); /* test builds only: bind a double; NULL restores the HIP binding */
#endif
/* the tuple fetch (fetch.h, cryo_fetch_tuples) is bound through a table of its own: CryoCodecOps keeps its layout.  It is called
 * with the ctx of the bound CryoCodecOps.  fetch_blocks is cryo_multi_fetch_blocks (include/cryo_codec.h): block i owns requests
 * req_first[i] .. req_first[i + 1] - 1 of pos (1-based item positions), result is cryo_fetch_result[req_first[n]] (16 bytes per
 * request: u32 status, u32 len, u64 off), the OK tuples lie packed in dst, *total is the end of the last byte used */
typedef struct CryoCodecFetchOps {
    int (*fetch_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                        const uint64_t *req_first, const uint16_t *pos, void *dst, size_t dst_cap, void *result, uint64_t *total);
} CryoCodecFetchOps;
/* the fetch table that goes with cryo_host_codec_ops(): production's binds the GPU codec; NULL when a bound double has none */
const CryoCodecFetchOps *cryo_host_fetch_ops(void);
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_fetch_ops(const CryoCodecFetchOps *ops); /* test builds only: the fetch table of the bound double, or NULL */
#endif
/* the scan filter (filter.h, cryo_filter_scan) is bound through a table of its own as well.  filter_blocks is
 * cryo_multi_filter_blocks (include/cryo_codec.h): filter is a const cryo_filter * with host arrays, blocks gets one
 * cryo_filter_block (32 bytes) per stream, rec one cryo_filter_rec (8 bytes) per match and per bad item, the matches lie packed
 * in dst, total[0] / total[1] are the ends of the last byte / record used */
typedef struct CryoCodecFilterOps {
    int (*filter_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                         const void *filter, void *dst, size_t dst_cap, void *rec, size_t rec_cap, void *blocks, uint64_t *total);
} CryoCodecFilterOps;
/* the filter table that goes with cryo_host_codec_ops(): production's binds the GPU codec; NULL when a bound double has none */
const CryoCodecFilterOps *cryo_host_filter_ops(void);
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_filter_ops(const CryoCodecFilterOps *ops); /* test builds only: the filter table of the bound double, or NULL */
#endif
/* the scan aggregate (aggregate.h, cryo_aggregate_scan) is bound through a table of its own as well.  agg_blocks is
 * cryo_multi_agg_blocks (include/cryo_codec.h): filter is a const cryo_filter * and agg a const cryo_agg *, both with host
 * arrays; blocks gets one cryo_agg_block (16 bytes) per stream, cells agg->ncols cryo_agg_cell (40 bytes each) per stream, in
 * call order */
typedef struct CryoCodecAggOps {
    int (*agg_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                      const void *filter, const void *agg, void *blocks, void *cells);
} CryoCodecAggOps;
/* the aggregate table that goes with cryo_host_codec_ops(): production's binds the GPU codec; NULL when a bound double has none */
const CryoCodecAggOps *cryo_host_agg_ops(void);
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_agg_ops(const CryoCodecAggOps *ops); /* test builds only: the aggregate table of the bound double, or NULL */
#endif
/* the grouped scan (group.h, cryo_group_scan) is bound through a table of its own as well.  group_blocks is
 * cryo_multi_group_blocks (include/cryo_codec.h): filter is a const cryo_filter *, group a const cryo_group * and agg a const
 * cryo_agg * (or NULL), all with host arrays; blocks gets one cryo_group_block (32 bytes) per stream in call order, groups up to
 * group_cap cryo_group_rec (24 bytes), cells agg->ncols cryo_agg_cell (40 bytes each) per group, *total the call's groups */
typedef struct CryoCodecGroupOps {
    int (*group_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                        const void *filter, const void *group, const void *agg, void *blocks, void *groups, size_t group_cap,
                        void *cells, uint64_t *total);
} CryoCodecGroupOps;
/* the group table that goes with cryo_host_codec_ops(): production's binds the GPU codec; NULL when a bound double has none */
const CryoCodecGroupOps *cryo_host_group_ops(void);
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_group_ops(const CryoCodecGroupOps *ops); /* test builds only: the group table of the bound double, or NULL */
#endif
/* the projecting scan (project.h, cryo_project_scan) is bound through a table of its own as well.  project_blocks is
 * cryo_multi_project_blocks (include/cryo_codec.h): filter is a const cryo_filter * and project a const cryo_project *, both with
 * host arrays; rows gets up to row_cap rows of row_bytes (the layout rule of include/cryo_codec.h), rec up to rec_cap
 * cryo_project_rec (8 bytes), blocks one cryo_project_block (32 bytes) per stream in call order, total[0] / total[1] the end of
 * the last row / record used */
typedef struct CryoCodecProjectOps {
    int (*project_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                          const void *filter, const void *project, void *rows, size_t row_cap, void *rec, size_t rec_cap,
                          void *blocks, uint64_t *total);
} CryoCodecProjectOps;
/* the project table that goes with cryo_host_codec_ops(): production's binds the GPU codec; NULL when a bound double has none */
const CryoCodecProjectOps *cryo_host_project_ops(void);
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_project_ops(const CryoCodecProjectOps *ops); /* test builds only: the project table of the bound double, or NULL */
#endif
/* the ordered scan (topn.h, cryo_topn_scan) is bound through a table of its own as well.  topn_blocks is cryo_multi_topn_blocks
 * (include/cryo_codec.h): filter is a const cryo_filter *, order a const cryo_order * and project a const cryo_project *, all with
 * host arrays; rows gets up to row_cap rows of row_bytes and rec as many cryo_topn_rec (24 bytes), blocks one cryo_topn_block (32
 * bytes) per stream in call order, *total the end of the last entry used */
typedef struct CryoCodecTopnOps {
    int (*topn_blocks)(void *ctx, int method, const void *const *src, const uint32_t *src_size, size_t n, size_t block_size,
                       const void *filter, const void *order, const void *project, void *rows, void *rec, size_t row_cap,
                       void *blocks, uint64_t *total);
} CryoCodecTopnOps;
/* the topn table that goes with cryo_host_codec_ops(): production's binds the GPU codec; NULL when a bound double has none */
const CryoCodecTopnOps *cryo_host_topn_ops(void);
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_host_set_topn_ops(const CryoCodecTopnOps *ops); /* test builds only: the topn table of the bound double, or NULL */
#endif
const CryoCodecOps *cryo_host_codec_ops(void);         /* lazily opens the GPU codec */
void cryo_host_codec_trim(void);                         /* idle backend: free the binding's device workspace and staging buffers */
size_t cryo_host_codec_bound(int method, size_t n);      /* cryo_codec_bound (or the bound double's): never opens the GPU */
const CryoCodecOps *cryo_host_codec_ops_if_open(void); /* the binding if there is one already; never opens the GPU */
const char *cryo_host_codec_error(void);

#endif /* __COMPRESSION_H__ */
