/*
 * cryo_codec.h -- C ABI of the MI355X-native cryo-block codec.
 *
 * This is the drop-in boundary underneath pg_cryogen's compression.h
 * (reference compression.h:7-24).  The reference reaches its codec through
 * six third-party calls; each entry point below names the call (file:line in
 * adjust/pg_cryogen) it replaces.  Plain C, plain pointers and sizes, no HIP or
 * torch types.  Nothing here ever calls elog()/exit()/throws: every function
 * returns a cryo_status (0 = ok, negative = error) so that the PG-side C shim
 * (pg_cryogen_amd/host/compression.c) can raise ereport(ERROR) itself without a
 * longjmp crossing C++ frames.
 *
 * Process model: a cryo_codec handle is bound to one GPU and one HIP stream and
 * is used by one thread at a time (a PostgreSQL backend is single-threaded;
 * reference pg_cryogen.c:603-663).  HIP is initialised lazily by
 * cryo_codec_open(), never at library load, so loading the library in the
 * postmaster before fork() is safe.
 *
 * There is NO CPU fallback in this library: without a usable GPU,
 * cryo_codec_open() fails with CRYO_E_NODEV and nothing else can be called.
 */
#ifndef CRYO_CODEC_H
#define CRYO_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* numeric values are an on-disk contract: CryoFirstPageHeader.compression_method
 * (reference compression.h:7-11, storage.h:64, cache.c:133) */
enum { CRYO_METHOD_LZ4 = 0, CRYO_METHOD_ZSTD = 1 };

typedef enum {
    CRYO_OK = 0,
    CRYO_E_ARG = -1,         /* bad argument (null pointer, unknown method, size 0 ...) */
    CRYO_E_HIP = -2,         /* HIP runtime call failed (see cryo_codec_last_error)     */
    CRYO_E_NODEV = -3,       /* no usable gfx950 device                                 */
    CRYO_E_CORRUPT = -4,     /* malformed compressed block, or decoded size != block_size */
    CRYO_E_DSTSIZE = -5,     /* destination capacity below cryo_codec_bound()           */
    CRYO_E_UNSUPPORTED = -6, /* valid request this build has no kernel for              */
    CRYO_E_NOMEM = -7,
    CRYO_E_VERIFY = -8       /* a compressed block failed verification (CRYO_OPT_ENCODE_VERIFY, cryo_codec_verify_batch) */
} cryo_status;

typedef struct cryo_codec cryo_codec; /* opaque: device id, stream, workspace */

/* ---- library / device ---- */

/* "cryo-codec X.Y (lz4 block format as liblz4 1.9.3; zstd frames as libzstd 1.4.8)" */
const char *cryo_codec_version(void);
/* number of visible HIP devices, or a negative cryo_status */
int cryo_codec_device_count(void);
/* bind a handle to `device`; creates its stream.  Lazy HIP init happens here. */
int cryo_codec_open(int device, cryo_codec **out);
void cryo_codec_close(cryo_codec *c);
/* text of the last HIP error seen by this handle ("" if none) */
const char *cryo_codec_last_error(const cryo_codec *c);
/* the handle's HIP stream as an opaque pointer (hipStream_t) for profilers/interop */
void *cryo_codec_stream(cryo_codec *c);
/* wait for everything queued on the handle's stream */
int cryo_codec_sync(cryo_codec *c);

/* ---- per-handle options (tuning and tests; the defaults are what production runs) ----
 * Values are read at every call, so a test can flip a path between two batches of one handle. */
typedef enum {
    /* LZ4 decode path: 0 = automatic (by the work in the batch), 1 = in-wave parse kernel (k_lz4_dec_ring),
     * 2 = sequence index + indexed decoder (k_lz4_index* + k_lz4_dec_seq) whatever the batch size, 3 = the few-blocks path
     * (every output byte in parallel, k_lat_*; calls it is not made for -- more than 64 blocks or 64 MiB, blocks below
     * 32 KiB or above 2 MiB -- take the automatic choice) */
    CRYO_OPT_LZ4_DECODE_PATH = 1,
    /* walkers per block of the sequence-index pass: 0 = automatic, else a power of two 1..64 */
    CRYO_OPT_LZ4_INDEX_WALKERS = 2,
    /* K-block host calls: minimum bytes of a call that is cut into pipelined chunks (default 64 MiB) */
    CRYO_OPT_PIPE_MIN_BYTES = 3,
    /* device-resident block pool (cryo_codec_decompress_blocks_keyed): capacity in bytes (0 = pool off, the default) */
    CRYO_OPT_POOL_BYTES = 4,
    /* zstd decode path: 0 = automatic (the four-kernel pipeline; the fused kernel for frames its planner does not take),
     * 1 = the fused one-wave-per-frame kernel for everything, 2 = the pipeline, 3 = the pipeline without the byte-parallel
     * execution it uses for calls of up to 64 frames (k_zlat_* + lat_copy.h): one wave per frame (k_zexec) whatever the call */
    CRYO_OPT_ZSTD_DECODE_PATH = 5,
    /* device workspace kept between calls (the LZ4 sequence index: 2.1 GB for 65 536 x 128 KiB blocks; the zstd decode
     * tiles: up to 12.8 GiB each, four in flight): the host-buffer calls (cryo_codec_*_blocks*), which end synchronised,
     * give back what exceeds this many bytes when they return; -1 = keep everything (the default of a bare handle: a
     * benchmark loop must not reallocate; host/compression.c sets pg_cryogen.gpu_workspace_keep_mb, default 1 GiB) */
    CRYO_OPT_WORKSPACE_KEEP_BYTES = 6,
    /* the most device workspace one call may allocate: 0 = automatic (70 % of what hipMemGetInfo reports free plus what
     * the handle already holds); the zstd decode pipeline runs fewer tiles at once to fit (1 tile at least) */
    CRYO_OPT_WORKSPACE_MAX_BYTES = 7,
    /* 1 (default): the staging worker threads, the pinned staging buffers and -- for the duration of a K-block call of
     * 8 MiB or more -- the calling thread are placed on the cpus of the NUMA node the handle's GPU hangs on (sysfs
     * local_cpulist of its PCI function, cut to the process's affinity mask; the caller's mask is restored on return);
     * 0: wherever the scheduler puts them.  get_option reports 0 when the node could not be determined. */
    CRYO_OPT_NUMA_LOCAL = 8,
    /* waves per block of the indexed LZ4 decoder: 0 = automatic (two for batches that leave most of the chip idle: up to
     * 3 072 blocks; one otherwise), 1 = k_lz4_dec_seq, 2 = k_lz4_dec_dual whatever the batch size */
    CRYO_OPT_LZ4_DECODE_WAVES = 9,
    /* segment-parallel encode, for calls of few blocks (the access method's write path hands over one block per call):
     * 0 (default) = the byte-identical encoders; a power of two S from 4 096 to 131 072 = every block of more than S bytes
     * is cut into ceil(B / S) segments, each encoded by its own wave (LZ4: any acceleration, blocks up to 16 MiB; zstd: the
     * levels whose strategy is at most CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY -- by default `fast`, levels -5 .. 2 -- other
     * levels, and blocks of at most S bytes, take the byte-identical path).  The
     * result is ONE valid LZ4 block / ONE zstd frame per cryo block (matches reach back into earlier segments; a zstd frame
     * holds ceil(B / S) blocks, each with its own entropy tables) that liblz4 1.9.3 / libzstd 1.4.8 decode to the input,
     * of at most cryo_codec_bound() bytes, and deterministic -- the same bytes for the same block whatever the call or the
     * batch -- but NOT the libraries' own output.  Applies to every compress entry point (cryo_codec_compress_batch,
     * _block, _blocks, cryo_multi_compress_blocks via cryo_multi_set_option).  Other values: CRYO_E_ARG. */
    CRYO_OPT_ENCODE_SEGMENT_BYTES = 10,
    /* the highest zstd strategy segment mode takes, in libzstd's ZSTD_strategy numbering: 1 = `fast` (default: exactly the
     * behaviour before this option existed, so that levels 3 and up stay byte-identical under CRYO_OPT_ENCODE_SEGMENT_BYTES),
     * 2 = `dfast`, 3 = `greedy`, 4 = `lazy`, 5 = `lazy2`, 6 = `btlazy2`.  By strategy, not by level: which strategy a level
     * maps to depends on the block size (libzstd's parameter tables).  A segment of a deeper strategy is that strategy's
     * zstd block over the segment's bytes with a seeded history of the 16 KiB before it (instead of everything before it),
     * repeat offsets that start disabled and fresh entropy tables; the stream properties are those above.  The optimal
     * parsers (`btopt`, `btultra`, `btultra2`: levels 13 / 16 and up) carry statistics from block to block and always take
     * the byte-identical path.  No effect while CRYO_OPT_ENCODE_SEGMENT_BYTES is 0.  Other values: CRYO_E_ARG. */
    CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY = 11,
    /* write verification: 0 (default) = none, exactly the behaviour before this option existed; 1 = every compress entry point
     * (cryo_codec_compress_batch, _block, _blocks, cryo_multi_compress_blocks via cryo_multi_set_option) decodes what it
     * encoded, with the automatic decode routes a later read takes, into handle workspace and compares it with the input
     * (cryo_codec_verify_batch below) on the device before it returns or before its statuses become visible.  A block that fails gets
     * CRYO_E_VERIFY: d_status[i] of cryo_codec_compress_batch; the return value of the host-buffer calls, with the block's
     * index and first differing byte in cryo_codec_last_error() and cryo_codec_last_verify_failure().  The output bytes are
     * the same with verification on or off.  Other values: CRYO_E_ARG. */
    CRYO_OPT_ENCODE_VERIFY = 12,
    /* zstd content checksums: 0 (default) = none, exactly the bytes written before this option existed; 1 = every zstd frame
     * written by every compress entry point (cryo_codec_compress_batch, _block, _blocks, cryo_multi_compress_blocks via
     * cryo_multi_set_option) carries one: the checksum flag in its frame header and the low 32 bits of XXH64 (seed 0) of the
     * block's input after its last block (RFC 8878 3.1.1), 4 bytes more per block.  The frames are libzstd's with
     * ZSTD_c_checksumFlag = 1, byte for byte, wherever the byte-identical encoders write them; segment mode
     * (CRYO_OPT_ENCODE_SEGMENT_BYTES) adds the same flag and trailer to its own frames.  Stock ZSTD_decompress checks the
     * checksum of every frame it reads, and so do the decoders here, on every route.  It costs one pass over the input after
     * the encode (bound by memory reads on large calls) and one over the output after a decode; a single frame of B bytes
     * is hashed by one quad of lanes: about 2 ms for a lone 1 MiB frame.  cryo_codec_bound is unchanged: the frame and its
     * checksum stay within ZSTD_compressBound.  LZ4 blocks have no checksum field: no effect on them.  Other values:
     * CRYO_E_ARG. */
    CRYO_OPT_ZSTD_CHECKSUM = 13,
    /* form of the sequence-index pass where the plan is ONE walker per block (full batches, CRYO_OPT_LZ4_INDEX_WALKERS = 1):
     * 0 (default) = automatic (the pair for batches that are resident at once, up to 256 blocks per compute unit; the single
     * wave for larger ones), 1 = one wave walks 64 blocks and feeds their LDS rings itself (k_lz4_index), 2 = a pair of
     * waves per 64 blocks, one walking and one feeding the same rings (k_lz4_idx_pair).  Both write the same rows; batches
     * indexed with several walkers per block are not affected.  Other values: CRYO_E_ARG. */
    CRYO_OPT_LZ4_INDEX_FORM = 14
} cryo_option;
int cryo_codec_set_option(cryo_codec *c, int option, int64_t value);
/* a long-lived backend between bursts: waits for the handle's queued work, then frees its device workspace, the device and
 * pinned staging buffers of the host-buffer calls and the single-block scratch (they are grow-only otherwise and come
 * back with the next call that needs them).  The device-resident pool stays (CRYO_OPT_POOL_BYTES = 0 frees it).
 * Reference contrast: the CPU libraries hold nothing between calls (compression.c:70-72,102-104 are one-shot). */
int cryo_codec_trim(cryo_codec *c);
int cryo_codec_get_option(const cryo_codec *c, int option, int64_t *value);

/* ---- sizes ---- */

/* replaces LZ4_compressBound (compression.c:67) / ZSTD_compressBound (compression.c:99):
 * identical values (131602 / 131584 at 128 KiB, 1052704 / 1052672 at 1 MiB). 0 on bad args. */
size_t cryo_codec_bound(int method, size_t block_size);

/* ---- device memory plumbing (plain hipMalloc/hipMemcpy wrappers so that C
 *      callers and ctypes need no HIP headers) ----
 * The kernels read compressed input in aligned 16-byte pieces: up to 15 bytes before a block's
 * first byte and after its last byte may be read (never used).  cryo_dev_alloc pads every
 * allocation by 64 bytes; a caller that brings its own device memory must leave that slack
 * after the last compressed block. */
int cryo_dev_alloc(cryo_codec *c, size_t bytes, void **d_ptr);
int cryo_dev_free(cryo_codec *c, void *d_ptr);
int cryo_dev_upload(cryo_codec *c, void *d_dst, const void *h_src, size_t bytes);   /* sync */
int cryo_dev_download(cryo_codec *c, void *h_dst, const void *d_src, size_t bytes); /* sync */
int cryo_dev_memset(cryo_codec *c, void *d_dst, int value, size_t bytes);           /* async */

/* ---- batch codec on DEVICE-RESIDENT buffers (the hot path) ----
 *
 * One wavefront per cryo block; blocks are independent (the reference uses the
 * stateless one-shot APIs, compression.c:70-72,102-104).  All calls are
 * asynchronous on the handle's stream; per-block results land in the device
 * arrays d_out_size / d_status (cryo_status values).
 *
 * block_size: 1 .. 0x7E000000 (LZ4_MAX_INPUT_SIZE, 2 GiB - 32 MiB) for both methods.  Every entry point that takes a
 * block size, these and the host-buffer and multi-GPU ones below, returns CRYO_E_ARG for a larger one, also for a call of
 * no blocks; nothing is launched.
 */

/*
 * Compress n_blocks blocks of block_size bytes.  Block i is read at
 * d_src + i*src_stride and written at d_dst + i*dst_stride
 * (dst_stride >= cryo_codec_bound(method, block_size)).
 *   method LZ4 : replaces LZ4_compress_fast(src,dst,B,LZ4_compressBound(B),accel)
 *                (compression.c:70-72); param = lz4_acceleration_guc (0..50);
 *                output bytes identical to liblz4 1.9.3.
 *   method ZSTD: replaces ZSTD_compress(dst,bound,src,B,level) (compression.c:102-104);
 *                param = zstd_compression_level_guc (-5..22).  Output bytes identical to
 *                libzstd 1.4.8 at every level (strategies fast ... btlazy2 and the optimal parsers
 *                btopt, btultra, btultra2) and every block size; a level above 22 returns
 *                CRYO_E_UNSUPPORTED (no CPU fallback).
 */
int cryo_codec_compress_batch(cryo_codec *c, int method, int param,
                              const void *d_src, uint64_t src_stride,
                              uint32_t block_size, uint64_t n_blocks,
                              void *d_dst, uint64_t dst_stride,
                              uint32_t *d_out_size, int32_t *d_status);

/*
 * Decompress n_blocks blocks.  Compressed block i is the d_src_size[i] bytes at
 * d_src + d_src_off[i]; it must decode to exactly block_size bytes, written at
 * d_dst + i*dst_stride.  d_status[i] = CRYO_OK or CRYO_E_CORRUPT.
 *   method LZ4 : replaces LZ4_decompress_safe(src,dst,csize,B) (compression.c:84)
 *   method ZSTD: replaces ZSTD_decompress(dst,B,src,csize)     (compression.c:116)
 * A stream that decodes to fewer than block_size bytes is reported as
 * CRYO_E_CORRUPT (the reference only Assert()s this, compression.c:88,120).
 */
int cryo_codec_decompress_batch(cryo_codec *c, int method,
                                const void *d_src, const uint64_t *d_src_off,
                                const uint32_t *d_src_size,
                                void *d_dst, uint64_t dst_stride,
                                uint32_t block_size, uint64_t n_blocks,
                                int32_t *d_status);

/*
 * Verify n_blocks compressed blocks against their raw input: raw block i is the block_size bytes at d_raw + i*raw_stride,
 * its stream the d_comp_size[i] bytes at d_comp + d_comp_off[i] (the slack rule of cryo_dev_alloc above applies, as for
 * cryo_codec_decompress_batch).  Each stream is decoded with the automatic decode routes of cryo_codec_decompress_batch
 * (whatever the handle's decode-path options say) into handle workspace -- never into caller memory -- in chunks that keep
 * the decoded blocks and the decoders' workspace within CRYO_OPT_WORKSPACE_MAX_BYTES -- and compared byte for byte.
 *   d_status[i] (out)          CRYO_OK, or CRYO_E_VERIFY: the stream is malformed, decodes to other than block_size bytes,
 *                              or decodes to other bytes
 *   d_first_mismatch[i] (out)  offset of the first byte that differs; 0xFFFFFFFF when the block verified, and when the
 *                              decoders rejected its stream (no decoded bytes to compare).  May be NULL.
 * Asynchronous on the handle's stream, like cryo_codec_decompress_batch.  The decodes do not count in
 * cryo_codec_counters (blocks_decompressed, bytes_out).
 *
 * What verification proves: that the project's OWN decoders turn the DEVICE copy of the stream back into the input.  It
 * catches encoder faults.  It checks nothing after that copy: the host-buffer calls copy the verified slots to host memory
 * afterwards, and that copy is not compared again.  It does not compare against liblz4 / libzstd, so a mistake made
 * identically in an encoder and its decoder would pass.  The decoders are
 * pinned to the stock libraries' streams separately, by the test suite.
 */
int cryo_codec_verify_batch(cryo_codec *c, int method, const void *d_raw, uint64_t raw_stride, uint32_t block_size,
                            uint64_t n_blocks, const void *d_comp, const uint64_t *d_comp_off, const uint32_t *d_comp_size,
                            int32_t *d_status, uint32_t *d_first_mismatch);

/* ---- checking stored blocks ----
 * A decoded cryo block is checked against the layout that cryo_init_page / cryo_storage_insert (pg_cryogen_amd/host/
 * storage.c; reference storage.c:15-50, include/cryo_synth.h) give every byte of a block except the tuple bodies.  The
 * rules, for a block of B bytes (B a multiple of 8, at least 16; all fields LE u32):
 *   lower at byte 0, upper at byte 4, n = (lower - 8) / 8; item i (0-based) is off_i at 8 + 8i and len_i at 12 + 8i;
 *   MAXALIGN(x) = (x + 7) & ~7.
 *   1. HEADER: lower >= 8, (lower - 8) % 8 == 0, n <= 290 (MaxHeapTuplesPerPage - 1), lower <= upper <= B, and upper == B
 *      when n == 0.
 *   2. ITEM i fails (in 64-bit arithmetic) when len_i == 0, or off_i + MAXALIGN(len_i) != (i == 0 ? B : off_{i-1}) --
 *      off_{i-1} as stored in item i - 1 --, or i == n - 1 and off_i != upper.
 *   3. NONZERO: a byte in [lower, upper) or in a pad [off_i + len_i, off_i + MAXALIGN(len_i)) is not zero.
 * Each block gets one {reason, offset}; the first failing class wins:
 *   CRYO_CHECK_OK       every rule holds                                      offset 0xFFFFFFFF
 *   CRYO_CHECK_STREAM   the decoders reject the stream: malformed, other than   offset 0xFFFFFFFF
 *                       B bytes, or a zstd content checksum mismatch
 *   CRYO_CHECK_HEADER   rule 1                                                offset 0
 *   CRYO_CHECK_ITEM     rule 2                                                offset 8 + 8i of the lowest failing item
 *   CRYO_CHECK_NONZERO  rule 3, checked when rules 1 and 2 hold               offset of the lowest such byte
 * What the check does not see: tuple bodies.  An LZ4 block has no checksum field, so a damaged LZ4 stream that still
 * decodes to B bytes with an intact header, item array, gap and pads passes; a zstd frame written with
 * CRYO_OPT_ZSTD_CHECKSUM has its whole content covered by the checksum (STREAM).  A checksum mismatch is not told apart
 * from a malformed stream.  Tuple headers are not checked. */
typedef enum {
    CRYO_CHECK_OK = 0,
    CRYO_CHECK_STREAM = 1,
    CRYO_CHECK_HEADER = 2,
    CRYO_CHECK_ITEM = 3,
    CRYO_CHECK_NONZERO = 4
} cryo_check_reason;
typedef struct {
    uint32_t reason, offset;
} cryo_check_result;
/* Check n_blocks stored blocks: stream i is the d_src_size[i] bytes at d_src + d_src_off[i] (the slack rule of
 * cryo_dev_alloc applies, as for cryo_codec_decompress_batch); d_result[i] (device) gets its {reason, offset}.  Decoded
 * with the automatic decode routes whatever the handle's decode-path options say, into handle workspace -- never into
 * caller memory -- in chunks within CRYO_OPT_WORKSPACE_MAX_BYTES, as cryo_codec_verify_batch; the device pool is neither
 * read nor filled, and nothing counts in cryo_codec_counters.  Asynchronous on the handle's stream.  CRYO_E_ARG: an
 * unknown method, a block_size that is not a multiple of 8 or is below 16, a null pointer; n_blocks == 0: CRYO_OK. */
int cryo_codec_check_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                           const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks,
                           cryo_check_result *d_result);

/* ---- recompression: stored streams -> decoded in handle workspace -> encoded again, all on the device ----
 * A cryo relation is append-only and every block keeps the codec it was written with; this is the codec side of rewriting
 * one (pg_cryogen_amd/host/recompress.h): an LZ4 relation to checksummed zstd, zstd-1 to a deep level.  Stream i (src_method:
 * the d_src_size[i] bytes at d_src + d_src_off[i], the slack rule of cryo_dev_alloc applies) is decoded and encoded with
 * (dst_method, dst_param) into d_dst + i * dst_stride, dst_stride >= cryo_codec_bound(dst_method, block_size).
 *   Bytes    d_out_size[i] bytes that are exactly what cryo_codec_compress_batch(dst_method, dst_param) writes for the decoded
 *            block under the handle's current encode options (CRYO_OPT_ENCODE_SEGMENT_BYTES, _SEGMENT_ZSTD_STRATEGY,
 *            _ZSTD_CHECKSUM, _ENCODE_VERIFY): the encode IS that call, so with the defaults liblz4 1.9.3's / libzstd 1.4.8's
 *            own output.  No new stream format.  dst_method == src_method is allowed (a level change, adding checksums).
 *   Decode   the automatic decode routes whatever the handle's decode-path options say, into handle workspace -- never into
 *            caller memory --, zstd content checksums checked as on every read.  The call runs in chunks of K blocks that keep
 *            the decoded blocks, the stream tables, the encoder's and the decoders' workspace (and, for the host-buffer call
 *            below, K output slots and a packed area of K slots) within CRYO_OPT_WORKSPACE_MAX_BYTES; with verification on,
 *            the verifier plans its own chunks within what is left (one block at least).  The device pool is neither read
 *            nor filled.
 *   Status   d_status[i] = CRYO_OK; CRYO_E_CORRUPT: the decoders reject stream i (its neighbours are unaffected);
 *            CRYO_E_VERIFY: CRYO_OPT_ENCODE_VERIFY is on and the new stream failed it.  d_out_size[i] is 0 unless the status
 *            is CRYO_OK.
 *   Counters the internal decodes do not count in cryo_codec_counters (as in verify and check); the encode counts in
 *            blocks_compressed / bytes_in as any compress does.
 * Asynchronous on the handle's stream.  CRYO_E_ARG: an unknown method, block_size 0, a null pointer; CRYO_E_DSTSIZE: dst_stride
 * below the bound; CRYO_E_UNSUPPORTED: a zstd level above 22; n_blocks == 0: CRYO_OK. */
int cryo_codec_recode_batch(cryo_codec *c, int src_method, const void *d_src, const uint64_t *d_src_off,
                            const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks,
                            int dst_method, int dst_param, void *d_dst, uint64_t dst_stride,
                            uint32_t *d_out_size, int32_t *d_status);

/* ---- fetching tuples by position: stored streams -> decoded in handle workspace -> only the tuples asked for come back ----
 * Every other read route returns whole decoded blocks.  Two of the access method's read paths want a few tuples of a block (a
 * bitmap heap scan: reference pg_cryogen.c:412-509; an index fetch: pg_cryogen.c:372-410); this is their codec side
 * (pg_cryogen_amd/host/fetch.h walks a relation with it).
 * A call names n_blocks stored streams as cryo_codec_check_batch does and, per block, a list of 1-based item positions
 * (PostgreSQL's OffsetNumber) in CSR form: block i owns requests req_first[i] .. req_first[i + 1] - 1 of pos[]; req_first has
 * n_blocks + 1 entries, req_first[0] = 0, req_first[n_blocks] = n_req.  A block may have no request.  Every request gets one
 * cryo_fetch_result.  With the names of the check's rules above (lower, upper, n, off_i, len_i, MAXALIGN, a block of B bytes, B a
 * multiple of 8 and at least 16, 64-bit arithmetic), for block i, the first failing class wins:
 *   CRYO_FETCH_STREAM   every request of the block    the decoders reject the stream (malformed, other than B bytes, a zstd
 *                                                     content checksum mismatch)
 *   CRYO_FETCH_HEADER   every request of the block    the check's rule 1 fails
 *   CRYO_FETCH_BADREQ   every request of the block    a position is 0, or the block's positions are not strictly ascending (a TID
 *                                                     bitmap yields them sorted and distinct)
 *   CRYO_FETCH_NOITEM   the request                   pos > n
 *   CRYO_FETCH_ITEM     the request                   item pos - 1 has len == 0, off % 8 != 0, off < upper, or
 *                                                     off + MAXALIGN(len) > B
 *   CRYO_FETCH_OVERLAP  every request of the block    the MAXALIGNed lengths of the block's OK requests sum to more than
 *                       that is still OK              B - upper (distinct items of a well-formed block are disjoint inside
 *                                                     [upper, B), so only overlapping items get there)
 *   CRYO_FETCH_OK       the request                   otherwise; len = len_i
 * Values 1 .. 3 equal cryo_check_reason's; 4 (NONZERO) has no meaning here and is unused.  The fetch reads only the items it is
 * asked for: it does NOT apply the check's chain rule (rule 2) or its zero rules (rule 3), and it does not look at tuple headers.
 * Placement: requests are laid out in call order.  `off` of a request is the sum of MAXALIGN(len) over the OK requests before it
 * (a failed request has len = 0, takes no room, and carries the offset at which the next tuple starts).  For an OK request the
 * destination holds the tuple's len bytes at off, then zeros up to MAXALIGN(len) whatever the block holds in its pad; nothing at
 * or beyond the call's total is written.  Because of the OVERLAP rule the total never exceeds the sum of B - upper_i, which is
 * below n_blocks * B: a destination of n_blocks * block_size bytes always suffices, and a caller may pass untouched virtual
 * memory of that size. */
typedef enum {
    CRYO_FETCH_OK = 0,
    CRYO_FETCH_STREAM = 1,
    CRYO_FETCH_HEADER = 2,
    CRYO_FETCH_ITEM = 3,
    CRYO_FETCH_NOITEM = 5,
    CRYO_FETCH_BADREQ = 6,
    CRYO_FETCH_OVERLAP = 7
} cryo_fetch_status;
typedef struct {
    uint32_t status, len;
    uint64_t off;
} cryo_fetch_result; /* 16 bytes */
/* Device buffers; asynchronous on the handle's stream.  Everything, the request table included, is device memory: d_req_first
 * 8-byte, d_dst 8-byte, d_result 16-byte, d_total 8-byte aligned (CRYO_E_ARG otherwise).  *d_total receives the call's packed
 * total; it is also where the running base lives between the call's internal chunks, so no host wait lies inside the call.
 * Tuples that would end beyond dst_cap are not written, and *d_total > dst_cap tells the caller so (the records are complete
 * either way).  Entries of d_req_first are cut to n_req, so a damaged table reads no request beyond d_pos[n_req - 1].
 * Decode as in the check: the automatic routes whatever the handle's decode-path options say, into handle workspace, in chunks
 * within CRYO_OPT_WORKSPACE_MAX_BYTES (the workspace also holds 8 bytes per request); the device pool is neither read nor
 * filled, nothing counts in cryo_codec_counters.  CRYO_E_ARG as for cryo_codec_check_batch (the same block-size rule), a null
 * request table with n_req > 0, a null d_dst with dst_cap > 0; n_blocks == 0: CRYO_OK, total 0. */
int cryo_codec_fetch_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                           const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks,
                           const uint64_t *d_req_first, const uint16_t *d_pos, uint64_t n_req,
                           void *d_dst, uint64_t dst_cap, cryo_fetch_result *d_result, uint64_t *d_total);

/* ---- filtering a scan: stored streams -> decoded in handle workspace -> a column test per tuple -> only the matches come back ----
 * The read route a sequential scan with a range predicate takes (WHERE ts >= a AND ts < b, WHERE id = x): the reference accepts
 * scan keys in cryo_beginscan and ignores them (pg_cryogen.c:185-211), so every decoded byte crosses PCIe and the executor throws
 * most of them away.  Here the test runs where the decoded block lies (pg_cryogen_amd/host/filter.h walks a relation with it).
 * A call names n_blocks stored streams as cryo_codec_check_batch does and one descriptor: the relation's columns as far as the
 * keys need them (pg_attribute.attlen, and attalign as 1 / 2 / 4 / 8 bytes) and up to four scan keys, which are ANDed -- or,
 * under CRYO_FILTER_TRUTH, combined by a truth table ("Truth table" below).
 *
 * Descriptor.  CRYO_E_ARG when: natts is 0 or above 1600 (MaxHeapAttributeNumber), or nkeys above 4 (nkeys == 0 is allowed:
 * every well-formed tuple matches); a key's att outside 1 .. natts; an attlen of 0, below -1 (cstring is not supported) or above
 * 32767; an attalign other than 1, 2, 4, 8; a varlena column (attlen == -1) with attalign < 4; a comparison key (CRYO_OP_LT ..
 * CRYO_OP_NE) with an unknown type, on a column whose attlen is not the type's size or whose attalign is below its attlen, or with
 * a value outside the type's range; an unknown op; a reserved field that is not zero; an unknown bit in flags.  For
 * CRYO_OP_ISNULL and CRYO_OP_NOTNULL, type and value are ignored.  Key values are signed and compared as such; tuples are
 * little-endian.
 * Byte-string keys.  A comparison key (CRYO_OP_LT .. CRYO_OP_NE) of type CRYO_KEY_BYTES (16; 4 .. 15 are kept for fixed-width
 * types, of which 8 and 9 are the float types below; the rest of them, 0 and anything above 16 are unknown) compares a text / varchar / bytea column with a constant: rsv is the
 * constant's length n, 0 .. CRYO_KEY_BYTES_MAX, and value the address of its n bytes -- a device address for cryo_codec_*_batch,
 * a host address for cryo_codec_*_blocks and cryo_multi_*_blocks; any alignment; not looked at when n == 0.  CRYO_E_ARG when the
 * key's column is not a varlena (attlen != -1), n > CRYO_KEY_BYTES_MAX, or n > 0 with a null address.  For every other type and
 * for the null tests rsv != 0 stays refused (a set key, below, apart).  The caller's arrays are never written: the library makes its own device copy of
 * the keys and of the constants, in which the kernels find each constant 8-byte aligned and zero-padded to a multiple of 8.
 * Such a key is no aggregate and no group column (CRYO_E_ARG there, as any unknown type).
 * Set keys.  CRYO_OP_IN (9) and CRYO_OP_NOT_IN (10) test an integer column against a list of integers (WHERE app_id IN (3, 17, 40),
 * campaign_id = ANY($1)): type is CRYO_KEY_INT2, CRYO_KEY_INT4 or CRYO_KEY_INT8, rsv the number of list members n, 1 ..
 * CRYO_KEY_SET_MAX, and value the address of n int64_t members -- a device address for cryo_codec_*_batch, a host address for
 * cryo_codec_*_blocks and cryo_multi_*_blocks; any alignment: the library only copies from it, as for a byte-string constant.
 * Members come in any order and may repeat; a member outside the range of the key's type is allowed and equals no value, so
 * that validating a descriptor never depends on the list's contents.  The column rule is the comparison key's: attlen is the
 * type's size and attalign at least that.  CRYO_E_ARG when n == 0, n > CRYO_KEY_SET_MAX, the address is null, or the type is not
 * one of the three integer types (CRYO_KEY_BYTES included).  A set key counts as one of the four keys; several may be used, also
 * on one column and beside comparisons, null tests and byte-string keys.  The library's device copy holds a set as its distinct
 * members, ascending as signed 64-bit integers and 8-byte aligned; the caller's key array and lists are only read.  The binder's
 * part, not enforced here: drop NULL members from an IN list, never push down a NOT IN whose list holds a NULL, and fold an
 * empty list itself.
 * Float keys.  A comparison key (CRYO_OP_LT .. CRYO_OP_NE) of type CRYO_KEY_FLOAT4 (8: the column's attlen is 4, its attalign
 * at least 4) or CRYO_KEY_FLOAT8 (9: attlen 8, attalign 8) compares a float4 / float8 column with a constant (WHERE revenue > 0).
 * For both types value holds the 64 bits of an IEEE DOUBLE: a float4 column's value is widened to double -- exactly, a subnormal
 * included -- and compared with it, which serves PostgreSQL's float4, float8, float48 and float84 operator families alike; the
 * binder widens a float4 constant.  Every bit pattern is a valid constant, NaN included; rsv must be 0.  The order is
 * PostgreSQL's float8_cmp_internal: -Inf < every finite value < +Inf < NaN; all NaNs are equal to each other, whatever their
 * sign or payload, so x = 'NaN' is true on a NaN; -0 equals +0.  A comparison is false on a NULL, as for integers, and the null
 * tests ignore the type, as always.  CRYO_OP_IN / CRYO_OP_NOT_IN with a float type is CRYO_E_ARG (no lists of floats), and so is a
 * float type as a group column (no GROUP BY a float); as an aggregate column it is allowed ("A float column's cell", below).
 * The order as integers: the double bits b map to the signed 64-bit integer m(b) = INT64_MAX for a NaN, 0 for either zero, and
 * otherwise b ^ ((b >> 63, arithmetic) & 0x7FFFFFFFFFFFFFFF), whose integer order is the order above; m is its own inverse apart
 * from the two canonical cases.  The library's own copy of a float key holds m(value) -- the caller's arrays are never written
 * -- and the kernels map a column's value the same way, so the compare, the minimum and the maximum are the integers'.
 * Pattern keys.  CRYO_OP_LIKE (11) and CRYO_OP_NOT_LIKE (12) match a text / varchar / bytea column against a LIKE pattern (WHERE
 * url LIKE '%utm_source=%', bundle LIKE 'com.adjust.%', user_agent NOT LIKE '%bot%').  type is CRYO_KEY_BYTES and the column a
 * varlena (attlen == -1): the byte-string key's column rule.  value is the address of the pattern -- a device address for
 * cryo_codec_*_batch, a host address for cryo_codec_*_blocks and cryo_multi_*_blocks; any alignment; the caller's memory is only
 * read.  Bits 0-15 of rsv are the pattern's length n, 0 .. CRYO_KEY_BYTES_MAX; bit 16 of rsv is CRYO_LIKE_UTF8; every other
 * bit must be 0.
 *   Pattern syntax: '%' matches any run of characters, the empty run included; '_' matches exactly one character; '\' followed
 *   by a byte x is x taken literally; every other byte is literal.  Literal bytes are compared as unsigned bytes.  The binder
 *   rewrites any other ESCAPE character to '\' before the call.
 *   What a character is: without CRYO_LIKE_UTF8 one byte (bytea, SQL_ASCII and the single-byte encodings).  With CRYO_LIKE_UTF8
 *   one byte plus every byte 10xxxxxx (0x80 .. 0xBF) that directly follows it, which is PostgreSQL's stepping for UTF-8: '_'
 *   consumes one character, '%' tries character starts only -- the place where it stands and from there on every place one
 *   character further --, and literal pattern bytes are always compared bytewise.  On text that is not valid UTF-8 the same rule
 *   applies and defines the answer.  The pattern is the database's own text and valid UTF-8 under the flag; for a pattern that is
 *   not -- a '%' or '_' between the bytes of one character -- the answer is defined as that of matching the segments between
 *   the '%' greedily, each at its leftmost place (tests/like_ref.py: greedy), which there may differ from trying every run.
 *   CRYO_E_ARG: a type other than CRYO_KEY_BYTES; a column that is not a varlena; n > CRYO_KEY_BYTES_MAX (256); n > 0 with a null
 *   address; an rsv bit above 16; a pattern whose last byte is an unescaped '\' (PostgreSQL raises for it;
 *   cryo_filter_like_check of pg_cryogen_amd/host/filter.h tells the binder beforehand) -- in the device-resident calls this last
 *   one is found after the library has read the pattern back, that is with n_blocks > 0 alone.  (att, CRYO_KEY_INT4, 11, ..) and
 *   (att, CRYO_KEY_BYTES, 9, ..) stay refused.
 *   Verdicts: on a NULL column, a column beyond tnatts included, both ops are false.  A value is UNDECIDED when it is a TOAST
 *   pointer, compressed in line, or its payload is longer than CRYO_LIKE_TEXT_MAX (2048) bytes; an undecided value is what an
 *   undecided byte-string compare is: CRYO_FILTER_UNDECIDED, n_bad, in no cell, group or row, and under CRYO_FILTER_TRUTH the
 *   tuple is undecided only when the decided keys do not settle the table.  Otherwise CRYO_OP_LIKE is true iff the whole payload
 *   matches the whole pattern, and CRYO_OP_NOT_LIKE is its negation.  Only the payload's bytes are read, never the pad behind them.
 *   Why the cap: a lane matches its tuple's value alone while its wave waits, and the cap bounds a wave's work at about 2 049
 *   candidate starts times 256 pattern elements whatever the data -- a 1 MiB in-line value cannot stall a shared machine.  The
 *   caller re-reads the blocks with undecided items, as for toasted values.
 *   A pattern key counts as one of the four keys; several may be used, also on one column and beside every other kind of key.
 *   The filter (CRYO_FILTER_COUNT_ONLY included), the aggregate (float columns included), the grouped scan (plain, buckets,
 *   text), the projection and the ordered scan take them, device-resident, from host buffers and across devices, with or without
 *   CRYO_FILTER_TRUTH.  The library's device copy of such a key holds the pattern compiled (its segments between the '%', as
 *   literal bytes and any-one-character elements); the caller's arrays are never written.
 *   The binder's part, not enforced here: push a LIKE only under a deterministic collation; set CRYO_LIKE_UTF8 iff the database
 *   encoding is UTF8; never push for any other multibyte encoding; no ILIKE, no SIMILAR TO, no regular expressions.
 * Truth table.  CRYO_FILTER_TRUTH (4) in flags: the keys are not ANDed but combined by any tree of AND and OR (WHERE country =
 * 'de' OR app_id = 3; WHERE ts >= a AND ts < b AND (campaign_id IN (..) OR source IS NULL)).  f->rsv is then not reserved: it
 * holds the truth table W of the tree over its nkeys leaves.  Bit m of W, 0 <= m < 2^nkeys, says whether a tuple matches when
 * exactly the keys whose index bit is set in m are true: bit k of m is keys[k].  Four keys have 16 combinations, so every such
 * tree is 16 bits.  Without the flag nothing changes: rsv != 0 is refused and the keys are ANDed.  Flag 2 stays unknown and
 * refused.  The filter takes CRYO_FILTER_TRUTH alone or with CRYO_FILTER_COUNT_ONLY; the aggregate, the grouping and the
 * projection take flags == 0 or flags == CRYO_FILTER_TRUTH and refuse CRYO_FILTER_COUNT_ONLY as before.  CRYO_E_ARG with the
 * flag set when: nkeys == 0; W == 0 (a constant false is the binder's to fold); a bit at or above 2^nkeys is set; or W is not
 * monotone -- W is monotone when W[m] implies W[m | 1 << k] for every k < nkeys.  The all-ones table (constant true) and tables
 * that ignore a key are valid; an ignored key is still evaluated, the walk still goes to the highest key column for every
 * tuple, and the TUPLE rule is unchanged.  The key count stays four.
 * Why monotone: every key here is already false on NULL, while SQL's a OR b is three-valued.  For a formula built of AND and OR
 * alone, Kleene's result is TRUE exactly when the formula is true with every unknown leaf replaced by false, which is why W may
 * be indexed by "key is true" bits alone; and exactly the formulas of AND and OR have monotone tables.  NOT is the binder's to
 * push into the leaves (<>, >=, CRYO_OP_NOT_IN, CRYO_OP_NOTNULL), which is exact under three-valued logic for every op here; the
 * NULL caveats of set keys stand as they are.  cryo_filter_truth_dnf (pg_cryogen_amd/host/filter.h) builds W from a disjunctive
 * normal form and is monotone by construction: binders use it and do not hand-roll tables.
 *
 * Per block (names as in the check's rules above: lower, upper, n, off_i, len_i, MAXALIGN, B), the first failing rule wins:
 *   CRYO_FETCH_STREAM (1), CRYO_FETCH_HEADER (2)   exactly the fetch's; no item is examined, the block has no record
 *   otherwise every item 1 .. n is examined:
 *     CRYO_FETCH_ITEM (3)    the item fails the fetch's ITEM rule (len == 0, off % 8 != 0, off < upper, off + MAXALIGN(len) > B)
 *     CRYO_FILTER_TUPLE (8)  the tuple fails a tuple rule below
 *     CRYO_FILTER_UNDECIDED (9)  no key is false on the tuple, and a byte-string key met a value whose bytes are not in it
 *                                (under CRYO_FILTER_TRUTH: the keys that are decided do not decide W, see the verdict below)
 *     the items that pass these and pass every key (under CRYO_FILTER_TRUTH: and match by W) are the block's matches; the rest
 *     is silently no match
 *   CRYO_FETCH_OVERLAP (7)   the MAXALIGNed lengths of the matches sum to more than B - upper: the block delivers no tuple and no
 *                            match record (n_match = 0); its bad items keep their records
 *
 * Per tuple of len bytes at t (PostgreSQL's access/htup_details.h: HeapTupleHeaderData, HEAP_NATTS_MASK, HEAP_HASNULL, att_isnull;
 * access/tupmacs.h: att_align_nominal, att_align_pointer, att_addlength_pointer; postgres.h / varatt.h: VARATT_IS_1B, VARATT_IS_1B_E,
 * VARSIZE_1B, VARSIZE_4B, VARTAG_SIZE(VARTAG_ONDISK); the walk is heap_deform_tuple's, common/heaptuple.c -- restated for a
 * little-endian machine):
 *   t_infomask2 = u16 at t + 18, tnatts = t_infomask2 & 0x07FF;  t_infomask = u16 at t + 20, HASNULL = t_infomask & 1;
 *   t_hoff = the byte at t + 22;  the null bitmap starts at t + 23, bit i - 1 (byte (i - 1) / 8, bit (i - 1) % 8) SET means column
 *   i is NOT null.
 *   TUPLE rule, checked before anything else of the tuple is read: len >= 23, hoff % 8 == 0,
 *   hoff >= MAXALIGN(23 + (HASNULL ? (tnatts + 7) / 8 : 0)), hoff <= len.  Any larger multiple of 8 is as good, with HASNULL clear
 *   as with HASNULL set: the bytes between the header (and its bitmap) and t + hoff are not looked at.  Nothing else of the two
 *   infomask words is looked at either: the bits of t_infomask2 above HEAP_NATTS_MASK and every bit of t_infomask but HASNULL.
 *   A column i > tnatts is NULL (missing-attribute defaults are not known here: the binder must not push down a key on a column
 *   with atthasmissing).  With HASNULL, a column whose bitmap bit is clear is NULL.  A NULL column takes no room.
 *   The walk keeps an offset o from t + hoff, starting at 0, over the columns i = 1 .. the highest key column -- that far for
 *   every tuple, whatever the keys on the way said, and not a column further:
 *     fixed width   o = align(o, attalign); the column is the attlen bytes at o
 *     varlena       if the byte at o is 0: o = align(o, attalign).  With b the byte at o:
 *                   b == 0x01         an external pointer: the byte at o + 1 is its tag; tag 18 (on-disk TOAST): 18 bytes; any
 *                                     other tag: TUPLE
 *                   b & 1             a 1-byte header: b >> 1 bytes, header included
 *                   otherwise         a 4-byte header: (u32 at o) >> 2 bytes, header included; below 4: TUPLE
 *     then o += the column's size
 *   Every byte a column covers, its header (and an external pointer's tag) included, must lie below len: TUPLE otherwise.
 *   Nothing outside [t, t + len) is ever loaded, whatever the tuple says.
 *   Keys: a comparison on a NULL column is false; ISNULL and NOTNULL are what they say; the column's value is the signed
 *   little-endian integer of the key's type at o.
 *   Byte-string keys: the stepping above is unchanged.  The value of a non-NULL varlena column at o is
 *     1-byte header b (b & 1, b != 1)      the payload: the (b >> 1) - 1 bytes from o + 1
 *     4-byte header w, (w & 3) == 0        the payload: the (w >> 2) - 4 bytes from o + 4
 *     4-byte header w, (w & 3) == 2 (compressed in line), or an external pointer (0x01, tag 18)
 *                                          not in the tuple: the key is UNDECIDED on this tuple
 *   With plen the payload's length and n the constant's: c = memcmp(payload, constant, min(plen, n)) on UNSIGNED bytes, and when
 *   that is 0, c = sign(plen - n); the six ops are the obvious tests on c (= is c == 0, < is c < 0, ...).  Only the payload's
 *   plen bytes are read, never the pad behind them.
 *   Set keys: on a NULL column (a column beyond tnatts included) CRYO_OP_IN and CRYO_OP_NOT_IN are both false.  Otherwise, with v
 *   the column's value as above, sign-extended to 64 bits: IN is true when v equals some member of the list, NOT_IN when it
 *   equals none.  A set key is never undecided, and the walk still goes to the highest key column for every tuple.
 *   The verdict on a tuple, the first rule that applies: CRYO_FILTER_TUPLE if the walk fails anywhere up to the highest column
 *   it visits (it still goes that far whatever the keys said); no match if some key is decidedly false (false AND unknown is
 *   false); CRYO_FILTER_UNDECIDED if a byte-string key met an undecided value; otherwise a match.
 *   Under CRYO_FILTER_TRUTH the verdict is sharper.  With t the mask of keys that are true on the tuple and u the mask of keys
 *   that are undecided on it (a byte-string key on a value compressed in line or external; t & u == 0), the first rule that
 *   applies: CRYO_FILTER_TUPLE as above; a match if W[t] -- true even if every undecided key were false; no match if not
 *   W[t | u] -- false even if every undecided key were true; otherwise CRYO_FILTER_UNDECIDED.  So country = 'de' OR app_id = 3
 *   with a toasted country and app_id = 3 is a match, not a bad item.  With the AND table W = 1 << (2^nkeys - 1) this is the
 *   rule without the flag, word for word: W[t] says every key is true, not W[t | u] that some key is decidedly false.
 *
 * Results.  One cryo_filter_block per block, in call order.  One cryo_filter_rec per match {pos, 0, len} and one per bad item
 * {pos, CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE or CRYO_FILTER_UNDECIDED, 0} -- a damaged tuple is never silently absent from a scan,
 * and an undecided one is a bad item everywhere: it counts in n_bad (under CRYO_FILTER_COUNT_ONLY, in the aggregate and in the
 * grouped scan too), is in no cell and no group, and has a record and no tuple bytes here, so that the caller fetches or
 * rechecks the positions the records name --, in position order
 * within the block; the block's records are records rec_first .. rec_first + n_match + n_bad - 1 of the call.  Its tuples lie
 * packed from byte `off` of the destination on: each its len bytes, then zeros up to MAXALIGN(len) whatever the block holds in its
 * pad (as the fetch writes them); a tuple's offset is `off` plus the MAXALIGNed lengths of the block's matches before it.  Blocks
 * are placed in call order: rec_first and off of a block are the sums over the blocks before it (a STREAM, HEADER or OVERLAP block
 * carries the values at which the next block starts).  n_items = n (0 under STREAM and HEADER).  total[0] = the packed bytes,
 * total[1] = the records of the whole call, counted in full even where the caps cut the writing off; nothing at or beyond
 * either total, and nothing beyond dst_cap bytes or rec_cap records, is written: a tuple that would end beyond dst_cap and a
 * record at or beyond rec_cap are left out.  Because of the OVERLAP rule dst_cap >= n_blocks * B and rec_cap >= n_blocks * 290
 * always suffice.
 * CRYO_FILTER_COUNT_ONLY: the per-block table only -- status, n_items, n_match, n_bad; rec_first, off and both totals are 0; no
 * record, no tuple is written; OVERLAP is not applied, because nothing is placed. */
typedef struct { int16_t attlen; uint8_t attalign; uint8_t rsv; } cryo_att; /* pg_attribute.attlen; attalign as 1/2/4/8; 4 bytes */
typedef enum {
    CRYO_KEY_INT2 = 1, CRYO_KEY_INT4 = 2, CRYO_KEY_INT8 = 3, /* signed, little-endian */
    CRYO_KEY_FLOAT4 = 8, CRYO_KEY_FLOAT8 = 9,                /* IEEE single / double columns; a key's value: the bits of a double */
    CRYO_KEY_BYTES = 16                                      /* a byte string: rsv its length, value its address */
} cryo_key_type;
typedef enum {
    CRYO_OP_LT = 1, CRYO_OP_LE, CRYO_OP_EQ, CRYO_OP_GE, CRYO_OP_GT, CRYO_OP_NE, CRYO_OP_ISNULL, CRYO_OP_NOTNULL,
    CRYO_OP_IN = 9, CRYO_OP_NOT_IN = 10, /* a set key: rsv the number of members, value the address of that many int64_t */
    CRYO_OP_LIKE = 11, CRYO_OP_NOT_LIKE = 12 /* a pattern key: rsv the pattern's length and CRYO_LIKE_UTF8, value its address */
} cryo_key_op;
typedef struct { uint16_t att; uint8_t type, op; uint32_t rsv; int64_t value; } cryo_scan_key; /* att 1-based; 16 bytes */
typedef struct {
    uint32_t natts, nkeys, flags, rsv; /* rsv: 0, or under CRYO_FILTER_TRUTH the truth table W */
    const cryo_att *atts;      /* natts entries */
    const cryo_scan_key *keys; /* nkeys entries (may be null when nkeys == 0) */
} cryo_filter;
#define CRYO_FILTER_COUNT_ONLY 1u /* per-block table only: no records, no tuples */
#define CRYO_FILTER_TRUTH 4u      /* f->rsv is a truth table over the keys, which are not ANDed but combined by it */
#define CRYO_FILTER_TUPLE 8u      /* a record's status beside CRYO_FETCH_ITEM: the tuple breaks a tuple rule */
#define CRYO_FILTER_UNDECIDED 9u  /* a record's status: a byte-string key met a compressed or external value */
#define CRYO_KEY_BYTES_MAX 256u   /* the longest constant of a CRYO_KEY_BYTES key */
#define CRYO_KEY_SET_MAX 1024u    /* the most members of a CRYO_OP_IN / CRYO_OP_NOT_IN list */
#define CRYO_LIKE_UTF8 0x10000u   /* bit 16 of a pattern key's rsv: a character is a byte and the bytes 10xxxxxx behind it */
#define CRYO_LIKE_TEXT_MAX 2048u  /* the longest payload a pattern key is matched against; a longer one is undecided */
#define CRYO_FILTER_MAX_ATTS 1600u
#define CRYO_FILTER_MAX_KEYS 4u
typedef struct { uint32_t status, n_items, n_match, n_bad; uint64_t rec_first, off; } cryo_filter_block; /* 32 bytes, one per block */
typedef struct { uint16_t pos, status; uint32_t len; } cryo_filter_rec;                                   /* 8 bytes */
/* Device buffers.  The struct *f itself is host memory; f->atts and f->keys are DEVICE arrays (4-byte / 8-byte aligned).  The
 * host validates the descriptor before anything is queued: it reads the two arrays back on the handle's stream (one wait for
 * what the stream held before the call, at most 6400 + 64 bytes); from there on the call is asynchronous.  With a byte-string
 * or a set key the constants and lists are read back too (at most 4 x 8 192 more bytes) and the library's copy of keys and constants goes into
 * handle-owned device memory: two more waits before the call turns asynchronous; the copy serves all of the call's internal
 * chunks.  d_dst 8-byte, d_rec
 * 8-byte, d_blocks 16-byte, d_total 8-byte aligned (CRYO_E_ARG otherwise); d_total has two entries and is also where the two
 * running totals live between the call's internal chunks.  Decode as in the fetch: the automatic routes, handle workspace,
 * chunks within CRYO_OPT_WORKSPACE_MAX_BYTES (the workspace also holds 16 bytes per possible item of a chunk); the device pool
 * is neither read nor filled, nothing counts in cryo_codec_counters.  CRYO_E_ARG as for cryo_codec_fetch_batch (the same
 * block-size rule), a bad descriptor, a null d_blocks, and -- without CRYO_FILTER_COUNT_ONLY -- a null d_dst with dst_cap > 0 or a
 * null d_rec with rec_cap > 0; n_blocks == 0: CRYO_OK, totals 0. */
int cryo_codec_filter_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                            const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks, const cryo_filter *f,
                            void *d_dst, uint64_t dst_cap, cryo_filter_rec *d_rec, uint64_t rec_cap,
                            cryo_filter_block *d_blocks, uint64_t *d_total);

/* ---- aggregating a scan: stored streams -> decoded in handle workspace -> keys tested, integer and float columns reduced per block -> a
 *      row and a few cells per block come back ----
 * The query an append-only analytics store answers most: SELECT sum(x), min(ts), max(ts), count(x) FROM t WHERE ts >= a AND
 * ts < b.  The filter above ships every matching tuple back and the host deforms it a second time to add up one column; here the
 * column is reduced where the decoded block lies, and 16 + 40 * ncols bytes per block leave the device
 * (pg_cryogen_amd/host/aggregate.h walks a relation with it).  The unit is the block because visibility is a per-block decision in
 * this access method: a cryo block is written by one transaction (created_xid in the first page header), so the caller tests each
 * block's xid once and adds up the partial aggregates of the visible blocks -- exact under any snapshot.
 * A call names n_blocks stored streams as cryo_codec_check_batch does, the filter's descriptor *f (columns and up to four ANDed
 * keys, unchanged) and an aggregate descriptor *agg: ncols columns, each {att, type}, whose values are reduced over the block's
 * matches.
 *
 * Descriptor.  CRYO_E_ARG when: *f breaks one of the filter's descriptor rules above; f->flags is neither 0 nor
 * CRYO_FILTER_TRUTH (CRYO_FILTER_COUNT_ONLY has no meaning here); ncols is 0 or above 4 (a bare count is CRYO_FILTER_COUNT_ONLY's job); a column's att outside 1 .. f->natts; a
 * column's type not a cryo_key_type; the column's attlen not the type's size, or its attalign below its attlen (the comparison
 * key's rules); a reserved field (agg->rsv, a column's rsv or rsv2) that is not zero.  The same column may be named twice, and it
 * may also carry a key.
 *
 * Per block (names as in the check's and the filter's rules above):
 *   CRYO_FETCH_STREAM (1), CRYO_FETCH_HEADER (2)   exactly the filter's; n_items = n_match = n_bad = 0 and every cell of the block
 *                                                  is all zero
 *   otherwise (status 0, n_items = n) every item 1 .. n is examined with the filter's ITEM rule and TUPLE rule.  The walk over the
 *   tuple is the filter's with ONE difference: it goes over the columns 1 .. max(highest key column, highest aggregate column) --
 *   that far for every tuple, whatever the keys on the way said, and not a column further.  So a tuple whose bytes end before an
 *   aggregate column that lies beyond the last key column is CRYO_FILTER_TUPLE here, where the same keys alone would pass it in the
 *   filter.
 *     n_match   the items that pass both rules and every key
 *     n_bad     the items that fail the ITEM rule or the TUPLE rule (the walk included) or are undecided: counted, not listed, as under
 *               CRYO_FILTER_COUNT_ONLY -- a caller who sees n_bad > 0 reads that block through the filter
 *   OVERLAP is not applied, because nothing is placed.
 *
 * Per cell (block i, column j: cell i * ncols + j), over the block's matches:
 *   n               the matches whose column j is not NULL (a column beyond the tuple's natts is NULL, as is one whose bitmap bit
 *                   is clear)
 *   min, max        over those values, each the signed little-endian integer of the column's type at its place in the tuple
 *   sum_hi:sum_lo   their exact sum as a 128-bit two's-complement number (sum_lo the low 64 bits, unsigned; sum_hi the high 64
 *                   bits, signed).  A block has at most 290 items, so it never overflows.
 *   n == 0          min = max = 0 and the sum is 0
 * count(col) is n, count(*) is n_match, avg is the caller's division; the partials of blocks combine by adding n and the 128-bit
 * sums (with carry) and taking min / max over the cells with n > 0.
 *
 * A float column's cell.  An aggregate column of type CRYO_KEY_FLOAT4 or CRYO_KEY_FLOAT8 (the float key's column rule) may stand
 * beside integer columns in one descriptor; an integer column's cell is byte for byte what it is without them.  The float
 * column's 40 bytes are a cryo_agg_cell_f {n, min, max, sum, err}:
 *   n           as above; n == 0 gives all-zero bytes
 *   min, max    over the non-NULL matches in the float keys' order: max is NaN if any value is NaN, min only if all are.
 *               Returned widened to double and canonical: any NaN as 0x7FF8000000000000, any zero as +0.0
 *   sum, err    with P / M / Q "some value is +Inf / -Inf / NaN": if Q, or both P and M, sum = the canonical NaN and err = +0;
 *               else if P (or M), sum = +Inf (or -Inf) and err = +0; otherwise (sum, err) is the double-double result of the
 *               reduction below over the FINITE values: sum + err is the answer and sum = RN(sum + err).  If the finite values
 *               leave the double range inside the reduction, sum and err both come out as the canonical NaN; err is NaN in no
 *               other case.  PostgreSQL raises "value out of range: overflow" there, and so should the binder.
 * The reduction is part of the contract, so that a call's output stays defined byte for byte.  Every operation is IEEE
 * binary64, round to nearest, nothing fused, subnormals kept:
 *   TwoSum(a, b):      s = a + b; bb = s - a; e = (a - (s - bb)) + (b - bb)
 *   FastTwoSum(s, t):  h = s + t; l = t - (h - s)
 *   x (+) y on pairs:  (s, t) = TwoSum(x.hi, y.hi); t = t + (x.lo + y.lo); the result is FastTwoSum(s, t).  Commutative.
 *   aggregate call:    leaf S_l, l = 0 .. 63, starts at (+0, +0) and takes S_l <- S_l (+) (v, +0) for the finite non-NULL values
 *                      of the matches at positions p with (p - 1) mod 64 = l, in ascending p; then for d = 32, 16, .., 1 every
 *                      S_l <- S_l (+) S_(l xor d) at once; the result is S_0
 *   grouped call:      from (+0, +0), (+) (v, +0) over the group's matches in position order
 *   blocks and groups combine on the host (cryo_agg_cell_f_combine, pg_cryogen_amd/host/aggregate.h): add n, take min / max in
 *                      the order above, fold the P / M / Q rule, and (+) over (sum, err) in block order.
 * Accuracy: for finite inputs without overflow |sum + err - exact| <= 2^-90 * sum |v|.  A block has at most 290 items, each
 * (+) errs by an amount of order 2^-104 relative to the magnitudes it adds, and 290 steps stay below 2^-95: the bound has
 * margin, and it is still 2^30 tighter than the best guarantee plain double summation can give. */
typedef struct { uint16_t att; uint8_t type, rsv; uint32_t rsv2; } cryo_agg_col;   /* att 1-based; type: cryo_key_type; 8 bytes */
typedef struct { uint32_t ncols, rsv; const cryo_agg_col *cols; } cryo_agg;
#define CRYO_AGG_MAX_COLS 4u
typedef struct { uint32_t status, n_items, n_match, n_bad; } cryo_agg_block;      /* 16 bytes, one per block */
typedef struct { uint64_t n; int64_t min, max; uint64_t sum_lo; int64_t sum_hi; } cryo_agg_cell; /* 40 bytes */
typedef struct { uint64_t n; double min, max, sum, err; } cryo_agg_cell_f; /* a float column's cell: the same 40 bytes */
#ifdef __cplusplus
static_assert(sizeof(cryo_agg_cell_f) == 40, "a float column's cell is a cryo_agg_cell's 40 bytes");
#else
_Static_assert(sizeof(cryo_agg_cell_f) == 40, "a float column's cell is a cryo_agg_cell's 40 bytes");
#endif
/* Device buffers.  The structs *f and *agg are host memory; f->atts, f->keys and agg->cols are DEVICE arrays (4-byte / 8-byte /
 * 8-byte aligned).  The host validates the descriptors before anything is queued: it reads the three arrays back on the handle's
 * stream (one wait for what the stream held before the call); from there on the call is asynchronous, with no host wait between
 * its internal chunks.  d_blocks (n_blocks rows) 16-byte, d_cells (n_blocks * ncols cells) 8-byte aligned (CRYO_E_ARG otherwise).
 * Decode as in the filter: the automatic routes, handle workspace, chunks within CRYO_OPT_WORKSPACE_MAX_BYTES (the aggregate
 * itself needs no workspace); the device pool is neither read nor filled, nothing counts in cryo_codec_counters.  CRYO_E_ARG as
 * for cryo_codec_filter_batch (the same block-size rule), a bad descriptor, a null d_blocks or d_cells; n_blocks == 0: CRYO_OK. */
int cryo_codec_agg_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                         const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks, const cryo_filter *f,
                         const cryo_agg *agg, cryo_agg_block *d_blocks, cryo_agg_cell *d_cells);

/* ---- grouping a scan: stored streams -> decoded in handle workspace -> keys tested, matches partitioned by one or two integer
 *      columns per block, integer columns reduced per group -> a row per block, a record and a few cells per group come back ----
 * The query that follows the aggregate above: SELECT app_id, country, count(*), sum(revenue) FROM t WHERE ts >= a AND ts < b
 * GROUP BY app_id, country.  Through the filter every matching tuple crosses PCIe and the host deforms it a second time; here each
 * block's matches are grouped where the decoded block lies, and 32 bytes per block and 24 + 40 * ncols bytes per group and block
 * leave the device (pg_cryogen_amd/host/group.h walks a relation with it).  The unit is the block for the aggregate's reason:
 * one created_xid per block, so the caller tests each block's xid once and merges the groups of the visible blocks -- exact
 * under any snapshot.  Merging the groups of different blocks is the caller's (a hash table on the key and the null bits).
 * A call names n_blocks stored streams as cryo_codec_check_batch does, the filter's descriptor *f (unchanged), a group
 * descriptor *grp: nby columns, each {att, type}, and an aggregate descriptor *agg (may be NULL): ncols columns.
 *
 * Descriptors.  CRYO_E_ARG when: *f breaks one of the filter's descriptor rules above; f->flags is neither 0 nor CRYO_FILTER_TRUTH; nby is 0 or above 2; a
 * group column breaks a rule of an aggregate column above (att outside 1 .. f->natts; a type that is not a cryo_key_type; the
 * column's attlen not the type's size, or its attalign below its attlen; rsv or rsv2 not zero); grp->rsv none of zero,
 * CRYO_GROUP_BUCKETS ("Bucketed group columns" below) and CRYO_GROUP_TEXT ("Text group columns" below, which alone lets a group
 * column be a byte string); ncols above 4;
 * with ncols > 0, anything cryo_codec_agg_batch refuses in *agg.  ncols == 0 is allowed here -- agg NULL, or agg->ncols 0 with
 * agg->rsv 0 (agg->cols is not looked at) --: SELECT g, count(*) ... GROUP BY g needs no cell.  A column may be a group column,
 * an aggregate column and a key column at once, and may be named twice.
 *
 * Per block (names as in the check's, the filter's and the aggregate's rules above):
 *   CRYO_FETCH_STREAM (1), CRYO_FETCH_HEADER (2)   exactly the filter's; n_items = n_match = n_bad = n_groups = 0: the block has no
 *                                                  group
 *   otherwise (status 0, n_items = n) every item 1 .. n is examined with the filter's ITEM rule and TUPLE rule and the walk over
 *   the columns 1 .. max(highest key column, highest group column, highest aggregate column) -- that far for every tuple and not a
 *   column further: the aggregate's documented difference from the filter, the group columns included.  n_match and n_bad are the
 *   aggregate's (n_bad: the items that fail the ITEM or the TUPLE rule or are undecided); a damaged or undecided item is in no group (a caller who sees n_bad > 0 reads that block through the filter).  OVERLAP is not
 *   applied, because nothing is placed.
 *
 * Groups of a block.  The block's matches are partitioned by the tuple (null_1, value_1[, null_2, value_2]) of the group columns:
 * value_j the signed little-endian integer of the column's type, sign-extended to 64 bits; null_j set when the column is NULL -- its
 * bitmap bit is clear, or the column lies beyond the tuple's natts.  NULL is a value of its own, so NULLs form groups: (NULL, 5),
 * (5, NULL) and (NULL, NULL) are three groups.  A block's groups are ordered ascending by column 1, then by column 2; values compare
 * as signed 64-bit integers and NULL sorts after every value (PostgreSQL's ASC NULLS LAST).  The order is part of the contract:
 * the output of a call is defined byte for byte.
 *
 * Results.  One cryo_group_block per block, in call order: n_groups the block's groups, first_group the sum of n_groups over the
 * call's blocks before it (a block without groups carries the value at which the next block starts); rsv is 0.  One
 * cryo_group_rec per group: the block's are records first_group .. first_group + n_groups - 1 of the call, in the order above.
 * key[j] is value_j, or 0 when column j is NULL or j >= nby; bit j of nulls is set when group column j is NULL (no other bit is);
 * n_rows is the number of the group's matches -- count(*) --, so a block's n_rows sum to its n_match.  Per group and aggregate
 * column j one cryo_agg_cell, cell (first_group + g) * ncols + j for the block's group g: exactly the aggregate's cell (n of
 * non-NULL values, min, max, the exact 128-bit sum; all zero when n == 0), over the group's matches instead of the block's.
 * *total is the call's number of groups, counted in full even where group_cap cuts the writing off: no record at or beyond
 * group_cap and no cell at or beyond group_cap * ncols is written.  A block has at most 290 groups, so group_cap >= 290 *
 * n_blocks always suffices. */
typedef struct { uint32_t nby, rsv; const cryo_agg_col *by; } cryo_group;
#define CRYO_GROUP_MAX_BY 2u
typedef struct { uint32_t status, n_items, n_match, n_bad; uint32_t n_groups, rsv; uint64_t first_group; } cryo_group_block; /* 32 bytes, one per block */
typedef struct { int64_t key[2]; uint32_t n_rows, nulls; } cryo_group_rec;                                    /* 24 bytes, one per group */
/* Bucketed group columns: SELECT date_trunc('day', ts), app_id, count(*), sum(revenue) ... GROUP BY 1, 2.  A raw timestamp is
 * unique per row; what a report groups by is its hour, day, week or month.  cryo_group keeps its 16 bytes and its meaning: with
 * rsv == 0 a call is what it was.  With rsv == CRYO_GROUP_BUCKETS (1) the cryo_group pointer a call is handed points to a
 * cryo_group_b -- cryo_group's two words and `by`, then `buckets`: nby entries, one per group column, a DEVICE array for
 * cryo_codec_group_batch and a host array for cryo_codec_group_blocks / cryo_multi_group_blocks, exactly as `by` is; 8-byte
 * aligned.  The key of group column j is then a function of its non-NULL value v (sign-extended from its type), by kind:
 *   CRYO_BUCKET_NONE (0)    key = v, as without buckets.  flags, n, origin and value are 0.
 *   CRYO_BUCKET_WIDTH (1)   origin = o, value = w >= 1, n = 0: key = v - ((v - o) mod w), the difference and the modulus taken in
 *                           exact integers and the modulus in [0, w) -- o + w * floor((v - o) / w), PostgreSQL's date_bin: floored,
 *                           not truncated, below the origin.  The key is an int64_t and is not clamped to the column's type; a
 *                           key below INT64_MIN is not representable, and that value is undecided.
 *   CRYO_BUCKET_BOUNDS (2)  n = the number of boundaries, 1 .. CRYO_BUCKET_BOUNDS_MAX; value = the address of n int64_t -- a device
 *                           address for cryo_codec_group_batch, a host address for the other two --, origin = 0.  Any alignment,
 *                           any order, duplicates allowed: the contents never decide whether the descriptor is valid, the memory
 *                           is only read, and the library searches an ascending, duplicate-free copy of its own.  key = the
 *                           greatest boundary <= v; a value below the smallest boundary is undecided (a caller who wants every
 *                           value in a bucket adds INT64_MIN as a boundary).
 * flags bit CRYO_BUCKET_INFINITE (1), with kinds 1 and 2: the column is a date or timestamp, whose type minimum and maximum (of
 * int2, int4 or int8, by the group column's type) are -infinity and +infinity.  Such a value is its own bucket, key = v, as
 * date_bin and date_trunc return it; a value that is not an extreme but whose key would equal one is undecided.
 * NULL stays the NULL group.  A tuple that passes the keys but has an undecided bucket in any group column is counted in n_bad and
 * not in n_match, and is in no group and no cell -- the rule of an undecided byte-string key --, so a block's n_rows still sum to
 * its n_match and the caller reads a block with n_bad > 0 through the filter.  Everything else is unchanged: the order (ascending
 * by key 1, then key 2, NULLS LAST), records, cells, first_group, group_cap, *total, chunking, float aggregate columns and every
 * kind of key beside the grouping.  A column may be a bucketed group column, a raw aggregate column and a key at once (min(ts),
 * max(ts) per day), and may be named twice with two different buckets (hour and day).  With every kind CRYO_BUCKET_NONE the
 * result is byte for byte that of the rsv == 0 call.
 * CRYO_E_ARG when: grp->rsv is neither 0 nor 1 (4: "Text group columns" below, without buckets); buckets is null or not 8-byte aligned; a kind is unknown; WIDTH with value < 1 or
 * n != 0; BOUNDS with n == 0, n > CRYO_BUCKET_BOUNDS_MAX, a null address or origin != 0; NONE with flags, n, origin or value not
 * 0; an unknown flag bit, or CRYO_BUCKET_INFINITE with NONE; a bucket's rsv not 0. */
#define CRYO_GROUP_BUCKETS 1u          /* cryo_group.rsv: the struct is a cryo_group_b */
#define CRYO_BUCKET_NONE 0
#define CRYO_BUCKET_WIDTH 1
#define CRYO_BUCKET_BOUNDS 2
#define CRYO_BUCKET_INFINITE 1u        /* cryo_bucket.flags */
#define CRYO_BUCKET_BOUNDS_MAX 1024u   /* the most boundaries of a list: CRYO_KEY_SET_MAX */
typedef struct { uint8_t kind, flags; uint16_t rsv; uint32_t n; int64_t origin; int64_t value; } cryo_bucket; /* 24 bytes, one per group column */
typedef struct { uint32_t nby, rsv; const cryo_agg_col *by; const cryo_bucket *buckets; } cryo_group_b;       /* 24 bytes; rsv = CRYO_GROUP_BUCKETS */
/* Text group columns: SELECT country, count(*), sum(revenue) ... GROUP BY country.  cryo_group keeps its 16 bytes and its meaning:
 * with rsv == 0 or rsv == CRYO_GROUP_BUCKETS a call is what it was, byte for byte, and a group column of type CRYO_KEY_BYTES is
 * CRYO_E_ARG there.  With rsv == CRYO_GROUP_TEXT (4) the struct is still a cryo_group, and
 *   Columns.  A group column's type may be CRYO_KEY_BYTES, on a varlena column (attlen == -1: the column rule of a byte-string
 *     key; rsv and rsv2 zero, att in 1 .. f->natts).  The other group column, if there is one, may be an integer type or
 *     CRYO_KEY_BYTES too.  CRYO_KEY_BYTES stays refused as an aggregate column.  With integer group columns only the flag is legal
 *     and the call returns exactly the bytes of the rsv == 0 call.  ntext below: the group columns of type CRYO_KEY_BYTES, 0 .. 2.
 *   Value.  A non-NULL value's key is its in-line payload, 0 .. CRYO_GROUP_TEXT_MAX (32) bytes: the bytes behind a 1-byte header
 *     or behind an uncompressed 4-byte header.  '' is a value, not NULL.  Undecided are: an on-disk TOAST pointer, a value
 *     compressed in line, and a payload above CRYO_GROUP_TEXT_MAX bytes.  A tuple that passes the keys but has an undecided value in
 *     any text group column is counted in n_bad and not in n_match, and is in no group and no cell -- the rule of an undecided
 *     bucket --, so a block's n_rows still sum to its n_match and the caller reads a block with n_bad > 0 through the filter.  A
 *     tuple that fails the keys is a non-match, whatever its group value.
 *   Order within a block.  As without the flag: column 1, then column 2, NULLS LAST.  A text column orders by memcmp on unsigned
 *     bytes over the shorter length, then by length: the order of the byte-string keys ("ab" < "ab\0" < "abc").  Equal keys are
 *     equal byte strings, so the grouping is exact under any deterministic collation (there equal strings are equal bytes); the
 *     order of a block's groups is the collation's order under "C" only, and a caller that merges blocks by hashing needs none.
 *   Results.  Rows and records keep their layout.  For a text column j, key[j] is the value's length in bytes, or 0 when it is
 *     NULL; bit j of nulls as without the flag.  The bytes come back in the cells array: a group has ncols + ntext cells of 40
 *     bytes, the ncols aggregate cells as without the flag, then one cryo_group_key per text group column in column order -- cell
 *     (first_group + g) * (ncols + ntext) + ncols + t for the t-th text column.  A cryo_group_key holds the payload in bytes[0 ..
 *     len), zeros behind it, len, and rsv 0; a NULL's is all zero.  Wherever the rules of a group call say ncols for the number or
 *     the place of cells, read ncols + ntext: the capacity of d_cells / h_cells (group_cap * (ncols + ntext) cells), the rule that
 *     the cells pointer may be null (only when ncols + ntext == 0), the side area (24 + 40 * (ncols + ntext) bytes per possible
 *     group), the cut-off at group_cap, and what crosses PCIe.
 * Everything else is unchanged: first_group, group_cap, *total, chunking, float aggregate columns and every kind of key beside
 * the grouping -- a byte-string key on the group column itself included.
 * CRYO_E_ARG when: grp->rsv is none of 0, CRYO_GROUP_BUCKETS and CRYO_GROUP_TEXT -- both flags together (5) included: a call
 * has buckets or text columns --; a CRYO_KEY_BYTES group column on a column whose attlen is not -1, or without the flag. */
#define CRYO_GROUP_TEXT 4u             /* cryo_group.rsv: group columns may be CRYO_KEY_BYTES */
#define CRYO_GROUP_TEXT_MAX 32u        /* the longest payload that is a key */
typedef struct { uint8_t bytes[32]; uint32_t len, rsv; } cryo_group_key; /* 40 bytes: a text group column's cell */
/* Device buffers.  The structs *f, *grp and *agg are host memory; f->atts, f->keys, grp->by and agg->cols are DEVICE arrays (4-byte
 * / 8-byte / 8-byte / 8-byte aligned).  The host validates the descriptors before anything is queued: it reads the arrays back on
 * the handle's stream (one wait for what the stream held before the call); from there on the call is asynchronous, with no host
 * wait between its internal chunks.  d_blocks (n_blocks rows) 16-byte, d_groups (group_cap records) 8-byte, d_cells (group_cap *
 * ncols cells; may be NULL only when ncols == 0; under CRYO_GROUP_TEXT ncols + ntext in both places) 8-byte, d_total (one u64, also where the running total lives between the call's
 * internal chunks) 8-byte aligned: CRYO_E_ARG otherwise.  Decode as in the filter: the automatic routes, handle workspace, chunks
 * within CRYO_OPT_WORKSPACE_MAX_BYTES (the workspace also holds a side area of 24 + 40 * ncols bytes -- under CRYO_GROUP_TEXT 24 + 40 * (ncols + ntext) -- per possible group of a chunk:
 * up to 290 per block); the device pool is neither read nor filled, nothing counts in cryo_codec_counters.  CRYO_E_ARG as for
 * cryo_codec_filter_batch (the same block-size rule), a bad descriptor, a null d_total, a null d_blocks, and a null d_groups or
 * (with ncols > 0) a null d_cells with group_cap > 0; n_blocks == 0: CRYO_OK, *d_total = 0, nothing else is written. */
int cryo_codec_group_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                           const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks, const cryo_filter *f,
                           const cryo_group *grp, const cryo_agg *agg, cryo_group_block *d_blocks, cryo_group_rec *d_groups,
                           uint64_t group_cap, cryo_agg_cell *d_cells, uint64_t *d_total);

/* ---- projecting a scan: stored streams -> decoded in handle workspace -> keys tested, the named fixed-width columns of every
 *      match copied into a fixed row -> a row per block, an 8-byte record and a row of 8 .. 64 bytes per match come back ----
 * The SELECT list of the query the filter answers: SELECT id, ts, revenue FROM t WHERE ts >= a AND ts < b.  Through the filter
 * every matching tuple crosses PCIe whole -- 23 bytes of header, the null bitmap and every text column the query never asked for --
 * and the host deforms it a second time to pick three integers; here the columns are picked where the decoded block lies, and 8
 * + row_bytes bytes per match leave the device instead of 8 + MAXALIGN(len) (pg_cryogen_amd/host/project.h walks a relation with
 * it).  A projected column is only copied, never compared or added, so it needs no type: float4, float8, bool, date, timestamp
 * and oid columns come back bit for bit.
 * A call names n_blocks stored streams as cryo_codec_check_batch does, the filter's descriptor *f (columns and up to four ANDed
 * keys, unchanged; byte-string keys are allowed exactly as in the aggregate) and a projection *prj: ncols columns, each {att}.
 * Out of scope: varlena columns in the projection (text stays with the filter), fixed columns wider than 8 bytes (uuid, name),
 * expressions, more than 8 columns, and a combined project-and-aggregate call.
 *
 * Descriptor.  CRYO_E_ARG when: *f breaks one of the filter's descriptor rules above; f->flags is neither 0 nor CRYO_FILTER_TRUTH (a bare count is
 * CRYO_FILTER_COUNT_ONLY's job); ncols is 0 or above 8; a column's att outside 1 .. f->natts; the column's attlen not 1, 2, 4 or
 * 8, or its attalign below its attlen (varlena and wider fixed columns are not projected); a reserved field (prj->rsv, a column's
 * rsv or rsv2) that is not zero.  The same column may be named twice, and it may also carry a key.
 *
 * Row layout, fixed by the descriptor alone and the same for every match of the call: column j of the descriptor, of width w_j =
 * its attlen, lies at o_j, with o_0 = 0 and o_j = align(o_(j-1) + w_(j-1), w_j); row_bytes = MAXALIGN(o_last + w_last), 8 .. 64
 * (CRYO_PROJECT_COL_OFFSET and CRYO_PROJECT_ROW_BYTES below).  A non-NULL column is the column's w_j bytes as they lie in the tuple
 * (little-endian), bit for bit; a NULL column -- its bitmap bit is clear, or it lies beyond the tuple's natts -- is zero, and so is
 * every pad byte.
 *
 * Per block (names as in the check's, the filter's and the aggregate's rules above):
 *   CRYO_FETCH_STREAM (1), CRYO_FETCH_HEADER (2)   exactly the filter's; no item is examined, the block has no record and no row
 *   otherwise (status 0, n_items = n) every item 1 .. n is examined with the filter's ITEM rule and TUPLE rule.  The walk is the
 *   aggregate's: over the columns 1 .. max(highest key column, highest projected column) -- that far for every tuple, whatever the
 *   keys on the way said, and not a column further.  So a tuple whose bytes end before a projected column that lies beyond the
 *   last key column is CRYO_FILTER_TUPLE here, where the same keys alone would pass it in the filter.  An undecided tuple is a bad
 *   item (CRYO_FILTER_UNDECIDED).
 *   OVERLAP is never reported: a block places at most 290 * row_bytes bytes whatever it holds, so status 7 does not occur here.
 *
 * Results.  One cryo_project_block per block, in call order.  One cryo_project_rec per match {pos, 0, nulls} -- bit j of nulls is
 * set when projected column j is NULL, and no other bit is -- and one per bad item {pos, CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE or
 * CRYO_FILTER_UNDECIDED, 0}, in position order within the block; the block's records are records rec_first .. rec_first +
 * n_match + n_bad - 1 of the call: exactly the filter's record rule.  One row per match: the block's rows are rows row_first ..
 * row_first + n_match - 1 of the call, in position order, so the k-th match record of the block belongs to row row_first + k;
 * row r lies at byte r * row_bytes of the rows.  rec_first and row_first are the sums over the blocks before the block (a STREAM
 * or HEADER block carries the values at which the next block starts).  total[0] = the rows, total[1] = the records of the whole
 * call, counted in full even where a cap cuts the writing off: no row at or beyond row_cap rows, no record at or beyond rec_cap,
 * and nothing at or beyond either total is written.  row_cap >= 290 * n_blocks and rec_cap >= 290 * n_blocks always suffice.
 * The output of a call is defined byte for byte. */
typedef struct { uint16_t att; uint16_t rsv; uint32_t rsv2; } cryo_project_col;              /* att 1-based; 8 bytes */
typedef struct { uint32_t ncols, rsv; const cryo_project_col *cols; } cryo_project;
#define CRYO_PROJECT_MAX_COLS 8u
typedef struct { uint32_t status, n_items, n_match, n_bad; uint64_t rec_first, row_first; } cryo_project_block; /* 32 bytes */
typedef struct { uint16_t pos, status; uint32_t nulls; } cryo_project_rec;                    /* 8 bytes */
/* the row layout, column by column: with `end` the end of the column before (0 for the first), a column of width w lies at
 * CRYO_PROJECT_COL_OFFSET(end, w) and ends at that plus w; the row takes CRYO_PROJECT_ROW_BYTES(the last column's end) bytes */
#define CRYO_PROJECT_COL_OFFSET(end, w) (((uint32_t)(end) + (uint32_t)(w) - 1u) & ~((uint32_t)(w) - 1u))
#define CRYO_PROJECT_ROW_BYTES(end) (((uint32_t)(end) + 7u) & ~7u)
/* Device buffers.  The structs *f and *prj are host memory; f->atts, f->keys and prj->cols are DEVICE arrays (4-byte / 8-byte /
 * 8-byte aligned).  The host validates the descriptors before anything is queued: it reads the three arrays back on the handle's
 * stream (one wait for what the stream held before the call; with a byte-string key the filter's two more), then puts the
 * kernel's column table -- 64 bytes: att, width and offset per column -- into handle workspace (one more wait); from there on the
 * call is asynchronous, with no host wait between its internal chunks.  d_rows (row_cap rows of row_bytes), d_rec (rec_cap
 * records) and d_total 8-byte, d_blocks (n_blocks rows) 16-byte aligned (CRYO_E_ARG otherwise); d_total has two entries and is also
 * where the two running totals live between the call's internal chunks.  Decode as in the filter: the automatic routes, handle
 * workspace, chunks within CRYO_OPT_WORKSPACE_MAX_BYTES (the workspace also holds a side area of 8 + row_bytes bytes per possible
 * item of a chunk: up to 290 per block); the device pool is neither read nor filled, nothing counts in cryo_codec_counters.
 * CRYO_E_ARG as for cryo_codec_filter_batch (the same block-size rule), a bad descriptor, a null prj, a null d_total, a null
 * d_blocks, a null d_rows with row_cap > 0 or a null d_rec with rec_cap > 0; n_blocks == 0: CRYO_OK, totals 0. */
int cryo_codec_project_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                             const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks, const cryo_filter *f,
                             const cryo_project *prj, void *d_rows, uint64_t row_cap, cryo_project_rec *d_rec,
                             uint64_t rec_cap, cryo_project_block *d_blocks, uint64_t *d_total);

/* ---- ordering a scan: stored streams -> decoded in handle workspace -> keys tested, each block's matches ranked by one or two
 *      columns -> a row per block, and of every block only its first `limit` matches come back: a 24-byte record and the
 *      projection's row each ----
 * The "latest rows" query: SELECT id, ts, revenue FROM t WHERE app_id IN (3, 17) AND ts >= a ORDER BY ts DESC LIMIT 100.  Through
 * the projection a block returns every match, up to 290 rows, and the host sorts them and keeps 100 of the whole relation.  A
 * block is the unit of visibility (one created_xid per block), so the exact answer under any snapshot is "the first N rows, in
 * order, of every visible block, merged": each block's first N are selected where the decoded block lies, and 24 + row_bytes bytes
 * per KEPT row leave the device (pg_cryogen_amd/host/topn.h walks a relation with it and merges).
 * A call names n_blocks stored streams as cryo_codec_check_batch does, the filter's descriptor *f and the projection *prj, both
 * unchanged, and an order *ord: nby order columns, each {att, type, flags}, and limit.
 * Out of scope: text, bytea or bucketed order columns; more than two order columns; WITH TIES and DISTINCT ON; a call-wide cut
 * across blocks on the device (visibility is the caller's, per block: the merge is the host's); OFFSET (the binder asks for
 * LIMIT + OFFSET and drops the first rows after the merge).
 *
 * Descriptor.  CRYO_E_ARG when: *f or *prj is refused by cryo_codec_project_batch; nby is 0 or above CRYO_ORDER_MAX_BY; limit is 0;
 * an order column breaks the aggregate column's rules (att outside 1 .. f->natts, attlen not the type's size, attalign below
 * attlen) or its type is not CRYO_KEY_INT2, _INT4, _INT8, _FLOAT4 or _FLOAT8; a flag bit other than CRYO_ORDER_DESC and
 * CRYO_ORDER_NULLS_FIRST is set; a column's rsv is not 0.  A column may be an order column, a projected column and carry a key at
 * once; the same column may be both order columns.
 *
 * Per block: statuses, the ITEM and TUPLE rules and n_items, n_match, n_bad exactly as in the projection, except that the walk
 * runs over the columns 1 .. max(highest key column, highest projected column, highest order column) for every tuple.  Bad and
 * undecided items count in n_bad and are in no ranking; the call writes no record for them (the aggregate's rule: the caller reads
 * such a block through the filter).
 *
 * Order of a block's matches: ascending by order column 1, then by order column 2, each under its own flags; ties are broken by
 * position, ascending, so the order is total and stable.  Within a column: CRYO_ORDER_DESC reverses the order of the values.
 * NULLs -- a clear bitmap bit, or a column beyond the tuple's natts -- sort after every value, or before every value with
 * CRYO_ORDER_NULLS_FIRST, whatever the direction; all NULLs are equal.  Integer columns compare as sign-extended 64-bit integers.
 * Float columns compare in PostgreSQL's order: -Inf < finite < +Inf < NaN, all NaNs equal, -0 = +0; a float4 is widened exactly.
 * That order is the signed order of the value's image: with b the bits of the (widened) double, the image is INT64_MAX for a NaN,
 * 0 for either zero, b for any other positive value and b ^ 0x7FFFFFFFFFFFFFFF for a negative one.
 * Kept rows: the first min(limit, n_match) matches of that order.  limit >= 290 is an ordered projection of every match.
 *
 * Results.  One cryo_topn_block per block, in call order: n_match is counted in full, n_rows is the kept rows, row_first the sum of
 * n_rows over the blocks before (a STREAM or HEADER block carries the value at which the next block starts).  One cryo_topn_rec and
 * one row per kept row, in rank order: the block's are entries row_first .. row_first + n_rows - 1 of both outputs, record r
 * belongs to row r, and row r lies at byte r * row_bytes of the rows.  key[j] is the signed 64-bit integer the order compared,
 * BEFORE the direction is applied: the sign-extended value, or a float column's image; 0 when the column is NULL or j >= nby.  Bit j
 * of key_nulls is set when order column j is NULL, and no other bit is.  So a merge of blocks needs nothing but integer compares
 * and the descriptor's flags.  pos and nulls are cryo_project_rec's; the row is the projection's row, bit for bit.
 * *total (one entry) = the kept rows of the whole call, counted in full even where row_cap cuts the writing off: no record and no
 * row at or beyond row_cap, and nothing at or beyond the total, is written.  row_cap >= min(limit, 290) * n_blocks always suffices.
 * The output of a call is defined byte for byte. */
#define CRYO_ORDER_DESC        1u   /* cryo_order_col.flags */
#define CRYO_ORDER_NULLS_FIRST 2u
#define CRYO_ORDER_MAX_BY      2u
typedef struct { uint16_t att; uint8_t type, flags; uint32_t rsv; } cryo_order_col;           /* att 1-based; 8 bytes */
typedef struct { uint32_t nby, limit; const cryo_order_col *by; } cryo_order;                  /* 16 bytes */
typedef struct { uint32_t status, n_items, n_match, n_bad; uint32_t n_rows, rsv; uint64_t row_first; } cryo_topn_block; /* 32 bytes */
typedef struct { int64_t key[2]; uint16_t pos, key_nulls; uint32_t nulls; } cryo_topn_rec;    /* 24 bytes */
/* Device buffers.  The structs *f, *ord and *prj are host memory; f->atts, f->keys, ord->by and prj->cols are DEVICE arrays (4-byte
 * / 8-byte / 8-byte / 8-byte aligned).  The host validates the descriptors before anything is queued, as the projection does (the
 * same waits), then puts the kernel's table -- 80 bytes: the order columns, then the projection's column table -- into handle
 * workspace (one more wait); from there on the call is asynchronous, with no host wait between its internal chunks.  d_rows
 * (row_cap rows of row_bytes), d_rec (row_cap records) and d_total 8-byte, d_blocks (n_blocks rows) 16-byte aligned (CRYO_E_ARG
 * otherwise); d_total has one entry and is also where the running total lives between the call's internal chunks.  Decode as in
 * the projection (the workspace also holds a side area of 28 + row_bytes bytes per possible item of a chunk); the device pool is
 * neither read nor filled, nothing counts in cryo_codec_counters.  CRYO_E_ARG as for cryo_codec_project_batch, a bad descriptor, a
 * null ord or prj, a null d_total, a null d_blocks, a null d_rows or d_rec with row_cap > 0; n_blocks == 0: CRYO_OK, total 0. */
int cryo_codec_topn_batch(cryo_codec *c, int method, const void *d_src, const uint64_t *d_src_off,
                          const uint32_t *d_src_size, uint32_t block_size, uint64_t n_blocks, const cryo_filter *f,
                          const cryo_order *ord, const cryo_project *prj, void *d_rows, cryo_topn_rec *d_rec, uint64_t row_cap,
                          cryo_topn_block *d_blocks, uint64_t *d_total);

/* ---- single block, HOST buffers: what cryo_compress()/cryo_decompress()
 *      (compression.c:125-159) call.  Synchronous: H2D, kernel, D2H. ---- */
int cryo_codec_compress_block(cryo_codec *c, int method, int param,
                              const void *h_src, size_t block_size,
                              void *h_dst, size_t dst_cap, size_t *out_size);
int cryo_codec_decompress_block(cryo_codec *c, int method,
                                const void *h_src, size_t src_size,
                                void *h_dst, size_t block_size);

/* ---- K blocks at once, HOST buffers: what the batch write/read staging calls
 *      (write-behind of K full blocks from multi_insert, read-ahead of K block chains;
 *      reference one-at-a-time equivalents: pg_cryogen.c:726 and cache.c:178).
 *      Synchronous: one H2D, one kernel launch, one D2H for the whole batch; device buffers and a pinned
 *      staging buffer are kept in the handle (grow-only). ---- */
/* block i: h_src + i*block_size  ->  h_dst + i*dst_stride, size in h_out_size[i].  dst_stride >= bound;
 * the whole slot (up to bound bytes) may be written, only the first h_out_size[i] bytes are meaningful */
int cryo_codec_compress_blocks(cryo_codec *c, int method, int param,
                               const void *h_src, size_t block_size, size_t n_blocks,
                               void *h_dst, size_t dst_stride, uint32_t *h_out_size);
/* block i: h_src[i] (h_src_size[i] bytes) -> h_dst + i*block_size; h_status[i] = CRYO_OK / CRYO_E_CORRUPT.
 * Returns CRYO_OK when the batch ran, even if some blocks are corrupt. */
int cryo_codec_decompress_blocks(cryo_codec *c, int method,
                                 const void *const *h_src, const uint32_t *h_src_size, size_t n_blocks,
                                 void *h_dst, size_t block_size, int32_t *h_status);
/* the same with one destination pointer per block (the slots of the decompressed-block cache, reference
 * cache.c:46,178: `out` is a cache entry's data[]): block i -> h_dst[i]; a block whose status is not CRYO_OK
 * leaves its destination untouched */
int cryo_codec_decompress_blocks_to(cryo_codec *c, int method,
                                    const void *const *h_src, const uint32_t *h_src_size, size_t n_blocks,
                                    void *const *h_dst, size_t block_size, int32_t *h_status);
/* cryo_codec_check_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes), synchronous: the streams are staged
 * and uploaded as by cryo_codec_decompress_blocks (pinned buffers, pipelined chunks from CRYO_OPT_PIPE_MIN_BYTES on);
 * only the n_blocks * 8 bytes of h_result come back (the transfer counters: h2d_bytes what was uploaded, d2h_bytes
 * exactly 8 * n_blocks).  Returns CRYO_OK when the batch ran, whatever the blocks' verdicts. */
int cryo_codec_check_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                            size_t n_blocks, size_t block_size, cryo_check_result *h_result);

/* cryo_codec_recode_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes), synchronous.  Only compressed bytes
 * cross PCIe, in both directions: the streams are staged and uploaded as by cryo_codec_check_blocks (h2d_bytes grows by the
 * same amount for the same streams); on the device the new streams are packed (recode.hip) and only the packed bytes, a size
 * and a status per block come back: d2h_bytes grows by exactly packed_total + 8 * n_blocks.
 *   Packing  output stream i is the h_out_size[i] bytes at h_dst + h_out_off[i]; h_out_off[0] = 0, h_out_off[i + 1] =
 *            h_out_off[i] + align16(h_out_size[i]); the pad bytes behind a stream are written as zero, and nothing beyond the
 *            packed total is written: a caller may pass untouched virtual memory of the worst-case size.  A packed total above
 *            dst_cap: CRYO_E_DSTSIZE, and h_dst holds nothing to rely on; dst_cap >= n_blocks * align16(bound) always suffices.
 *   Status   h_status[i] as d_status[i] above; a block that failed has h_out_size[i] = 0 and takes no room.  Returns CRYO_OK
 *            when the batch ran, whatever the per-block statuses (as cryo_codec_decompress_blocks).
 * The host needs a chunk's sizes before it can size the copy of its packed bytes: two waits per internal chunk.  The upload is
 * not pipelined: a call stages all its streams in the handle's pinned buffer, which grows to the call's compressed size
 * (plus a quarter) and stays with the handle until cryo_codec_trim. */
int cryo_codec_recode_blocks(cryo_codec *c, int src_method, const void *const *h_src, const uint32_t *h_src_size,
                             size_t n_blocks, size_t block_size, int dst_method, int dst_param,
                             void *h_dst, size_t dst_cap, uint64_t *h_out_off, uint32_t *h_out_size, int32_t *h_status);

/* cryo_codec_fetch_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes; n_req = h_req_first[n_blocks]), synchronous.
 * Only compressed bytes and the request table travel towards the device, only records and tuples come back.
 *   Upload   the streams are staged and uploaded as by cryo_codec_recode_blocks (one copy from pinned memory, not pipelined:
 *            h2d_bytes grows by what cryo_codec_check_blocks uploads for the same streams in one copy), then the request table
 *            in a second copy: h2d_bytes grows by another align16(8 * (n_blocks + 1)) + align16(2 * n_req).
 *   Return   per internal chunk the chunk's records come back, then its packed bytes straight into h_dst (two waits per chunk;
 *            the host derives a chunk's total from its last record): d2h_bytes grows by exactly *h_total + 16 * n_req.
 *   Errors   a packed total above dst_cap: CRYO_E_DSTSIZE; the call stops at the chunk that does not fit, and *h_total, h_dst
 *            and h_result hold nothing to rely on (dst_cap >= n_blocks * block_size always fits).  CRYO_E_ARG: as
 *            cryo_codec_fetch_batch, and an h_req_first that does not start at 0 or that decreases.
 * Returns CRYO_OK when the batch ran, whatever the records say. */
int cryo_codec_fetch_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                            size_t n_blocks, size_t block_size, const uint64_t *h_req_first, const uint16_t *h_pos,
                            void *h_dst, size_t dst_cap, cryo_fetch_result *h_result, uint64_t *h_total);

/* cryo_codec_filter_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes; f->atts and f->keys are HOST arrays),
 * synchronous.  Only compressed bytes and the descriptor travel towards the device, only the block table, records and matching
 * tuples come back.
 *   Upload   the streams staged and uploaded as by cryo_codec_fetch_blocks, then the descriptor in a second copy: h2d_bytes grows
 *            by another align16(4 * natts) + 16 * nkeys.
 *   Return   per internal chunk the chunk's rows of the block table come back first, then exactly the chunk's records, then
 *            exactly its packed bytes straight into h_dst (the host takes the record count from the table and the byte count from
 *            the table and the last block's records: up to three waits per chunk): d2h_bytes grows by exactly
 *            32 * n_blocks + 8 * h_total[1] + h_total[0]; with CRYO_FILTER_COUNT_ONLY by 32 * n_blocks.
 *   Errors   packed bytes above dst_cap or records above rec_cap: CRYO_E_DSTSIZE; the call stops at the chunk that does not fit
 *            and the outputs hold nothing to rely on (dst_cap >= n_blocks * block_size and rec_cap >= n_blocks * 290 always
 *            fit).  CRYO_E_ARG as cryo_codec_filter_batch; a bad descriptor is refused before a device is touched.
 * h_total has two entries.  Returns CRYO_OK when the batch ran, whatever the table says. */
int cryo_codec_filter_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                             size_t n_blocks, size_t block_size, const cryo_filter *f,
                             void *h_dst, size_t dst_cap, cryo_filter_rec *h_rec, size_t rec_cap,
                             cryo_filter_block *h_blocks, uint64_t *h_total);

/* cryo_codec_agg_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes; f->atts, f->keys and agg->cols are HOST arrays),
 * synchronous.  Only compressed bytes and the descriptors travel towards the device, only rows and cells come back.
 *   Upload   the streams staged and uploaded as by cryo_codec_filter_blocks, then the descriptors in a second copy: h2d_bytes
 *            grows by another align16(4 * natts) + 16 * nkeys + align16(8 * ncols).
 *   Return   rows and cells of the whole call in two copies after the last chunk, one wait: d2h_bytes grows by exactly
 *            16 * n_blocks + 40 * n_blocks * ncols.
 * CRYO_E_ARG as cryo_codec_agg_batch; a bad descriptor is refused before a device is touched.  Returns CRYO_OK when the batch
 * ran, whatever the rows say. */
int cryo_codec_agg_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                          size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_agg *agg,
                          cryo_agg_block *h_blocks, cryo_agg_cell *h_cells);

/* cryo_codec_group_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes; f->atts, f->keys, grp->by and agg->cols are
 * HOST arrays), synchronous.  Only compressed bytes and the descriptors travel towards the device, only rows, records and cells
 * come back.
 *   Upload   the streams staged and uploaded as by cryo_codec_agg_blocks, then the descriptors in a second copy: h2d_bytes grows
 *            by another align16(4 * natts) + 16 * nkeys + 48 (the six column slots of the kernel).
 *   Return   after the last chunk the rows of the whole call, then -- their number known from the last row -- exactly the call's
 *            records and cells (two waits): d2h_bytes grows by exactly 32 * n_blocks + (24 + 40 * ncols) * *h_total.
 *   Errors   more groups than group_cap: CRYO_E_DSTSIZE, and the outputs hold nothing to rely on (group_cap >= 290 * n_blocks
 *            always fits).  CRYO_E_ARG as cryo_codec_group_batch (h_cells may be NULL only when ncols == 0 -- under CRYO_GROUP_TEXT, when ncols + ntext == 0); a bad descriptor is
 *            refused before a device is touched.  n_blocks == 0: CRYO_OK, *h_total = 0.
 * Returns CRYO_OK when the batch ran, whatever the rows say. */
int cryo_codec_group_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                            size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_group *grp,
                            const cryo_agg *agg, cryo_group_block *h_blocks, cryo_group_rec *h_groups, size_t group_cap,
                            cryo_agg_cell *h_cells, uint64_t *h_total);

/* cryo_codec_project_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes; f->atts, f->keys and prj->cols are HOST
 * arrays), synchronous.  Only compressed bytes and the descriptors travel towards the device, only the block table, records and
 * rows come back.
 *   Upload   the streams staged and uploaded as by cryo_codec_filter_blocks, then the descriptors in a second copy: h2d_bytes
 *            grows by another align16(4 * natts) + 16 * nkeys + align16(8 * ncols) (plus, as everywhere, the constants of
 *            byte-string keys).
 *   Return   after the last chunk the rows of the block table of the whole call, then -- their numbers known from the last row of
 *            the table -- exactly the call's records and rows (two waits): d2h_bytes grows by exactly
 *            32 * n_blocks + 8 * h_total[1] + row_bytes * h_total[0].
 *   Errors   more rows than row_cap or more records than rec_cap: CRYO_E_DSTSIZE, and h_rows and h_rec hold nothing to rely on
 *            (row_cap >= 290 * n_blocks and rec_cap >= 290 * n_blocks always fit).  CRYO_E_ARG as cryo_codec_project_batch; a bad
 *            descriptor is refused before a device is touched.  n_blocks == 0: CRYO_OK, totals 0.
 * h_total has two entries.  Returns CRYO_OK when the batch ran, whatever the table says. */
int cryo_codec_project_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                              size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_project *prj,
                              void *h_rows, size_t row_cap, cryo_project_rec *h_rec, size_t rec_cap,
                              cryo_project_block *h_blocks, uint64_t *h_total);

/* cryo_codec_topn_batch on host buffers (stream i: h_src[i], h_src_size[i] bytes; f->atts, f->keys, ord->by and prj->cols are HOST
 * arrays), synchronous.  Only compressed bytes and the descriptors travel towards the device, only the block table and the kept
 * rows' records and rows come back.
 *   Upload   the streams staged and uploaded as by cryo_codec_filter_blocks, then the descriptors in a second copy: h2d_bytes
 *            grows by another align16(4 * natts) + 16 * nkeys + 80 (plus, as everywhere, the constants of byte-string keys).
 *   Return   after the last chunk the rows of the block table of the whole call, then -- their number known from the last row of
 *            the table -- exactly the call's records and rows (two waits): d2h_bytes grows by exactly
 *            32 * n_blocks + (24 + row_bytes) * *h_total.
 *   Errors   more kept rows than row_cap: CRYO_E_DSTSIZE, *h_total is the full count and h_rows and h_rec hold nothing to rely on
 *            (row_cap >= min(limit, 290) * n_blocks always fits).  CRYO_E_ARG as cryo_codec_topn_batch; a bad descriptor is
 *            refused before a device is touched.  n_blocks == 0: CRYO_OK, total 0.
 * h_total has one entry.  Returns CRYO_OK when the batch ran, whatever the table says. */
int cryo_codec_topn_blocks(cryo_codec *c, int method, const void *const *h_src, const uint32_t *h_src_size,
                           size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_order *ord,
                           const cryo_project *prj, void *h_rows, cryo_topn_rec *h_rec, size_t row_cap,
                           cryo_topn_block *h_blocks, uint64_t *h_total);

/* ---- device-resident block pool ("optional device-resident compressed/decompressed pool so
 *      repeated scans skip PCIe"; the reference's cache is host-only: cache.c:17-50).
 *      With CRYO_OPT_POOL_BYTES > 0 the decoded blocks of keyed calls stay in HBM (first in, first out).  A key is the
 *      caller's identity of a block -- the host cache passes (relation oid << 32 | first block number), the key of
 *      reference cache.c:37-47 -- and 0 means "do not keep".  A block found in the pool with the same compressed size and
 *      the same 64-bit hash of its whole compressed stream is copied back from HBM: nothing travels towards the
 *      device and no kernel decodes it.  A relation that is rewritten or truncated must be dropped with
 *      cryo_codec_pool_invalidate (reference: the relcache callback, pg_cryogen.c:163-167). ---- */
int cryo_codec_decompress_blocks_keyed(cryo_codec *c, int method, const uint64_t *keys,
                                       const void *const *h_src, const uint32_t *h_src_size, size_t n_blocks,
                                       void *const *h_dst, size_t block_size, int32_t *h_status);
/* drop the entries whose key's upper 32 bits equal key_hi; all entries when all_entries != 0 */
int cryo_codec_pool_invalidate(cryo_codec *c, uint32_t key_hi, int all_entries);
typedef struct {
    uint64_t h2d_bytes, d2h_bytes;       /* bytes the host-buffer calls moved across PCIe, each direction */
    uint64_t pool_hits, pool_misses;     /* keyed blocks served from HBM / decoded                       */
    uint64_t pool_blocks, pool_capacity; /* blocks held now / slots                                      */
} cryo_codec_transfer_counters;
int cryo_codec_get_transfer_counters(const cryo_codec *c, cryo_codec_transfer_counters *out);

/* the block that made the handle's last host-buffer compress call return CRYO_E_VERIFY (index within that call) and its
 * first differing byte (0xFFFFFFFF: the decoders rejected its stream).  1 when that call failed verification, 0 when it
 * did not, or a negative cryo_status. */
int cryo_codec_last_verify_failure(const cryo_codec *c, uint64_t *block, uint32_t *first_mismatch);

/* ---- several GPUs behind one call: the dispatcher of BASELINE's "independent cryo blocks from a COPY multi_insert
 *      or a seq-scan shard embarrassingly across the 8 GPUs of one node (round-robin dispatch, no collective)".
 *      One codec handle per listed device (a device may be listed more than once), block i of a call goes to
 *      handle i mod G, one host thread per handle drives its share through the K-block calls above; results land
 *      where the single-handle calls would have put them.  The reference has no counterpart (one block, one core:
 *      pg_cryogen.c:726, cache.c:178). ---- */
typedef struct cryo_multi cryo_multi;
int cryo_multi_open(const int *devices, int n_devices, cryo_multi **out);
void cryo_multi_close(cryo_multi *m);
int cryo_multi_count(const cryo_multi *m);
const char *cryo_multi_last_error(const cryo_multi *m);
int cryo_multi_compress_blocks(cryo_multi *m, int method, int param,
                               const void *h_src, size_t block_size, size_t n_blocks,
                               void *h_dst, size_t dst_stride, uint32_t *h_out_size);
int cryo_multi_decompress_blocks(cryo_multi *m, int method,
                                 const void *const *h_src, const uint32_t *h_src_size, size_t n_blocks,
                                 void *h_dst, size_t block_size, int32_t *h_status);
/* one destination per block (cryo_codec_decompress_blocks_to across the devices): what the decompressed-block cache
 * binds, its slots are the destinations (reference cache.c:46,178) */
int cryo_multi_decompress_blocks_to(cryo_multi *m, int method,
                                    const void *const *h_src, const uint32_t *h_src_size, size_t n_blocks,
                                    void *const *h_dst, size_t block_size, int32_t *h_status);
/* keyed (pool) variant: a keyed block goes to handle (key mod G), so that it finds its pool entry again; options and
 * invalidation reach every handle; the counters are summed */
int cryo_multi_decompress_blocks_keyed(cryo_multi *m, int method, const uint64_t *keys,
                                       const void *const *h_src, const uint32_t *h_src_size, size_t n_blocks,
                                       void *const *h_dst, size_t block_size, int32_t *h_status);
int cryo_multi_set_option(cryo_multi *m, int option, int64_t value);
int cryo_multi_pool_invalidate(cryo_multi *m, uint32_t key_hi, int all_entries);
int cryo_multi_trim(cryo_multi *m);
int cryo_multi_get_transfer_counters(const cryo_multi *m, cryo_codec_transfer_counters *out);
/* cryo_codec_last_verify_failure of the last cryo_multi_compress_blocks call (block: the index within the whole call; the
 * lowest one when several handles failed) */
int cryo_multi_last_verify_failure(const cryo_multi *m, uint64_t *block, uint32_t *first_mismatch);
/* cryo_codec_check_blocks across the devices: block i -> handle i mod G */
int cryo_multi_check_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                            size_t n_blocks, size_t block_size, cryo_check_result *h_result);

/* cryo_codec_recode_blocks across the devices: block i -> handle i mod G.  Handle g packs its share, in block order, into
 * the g-th of G equal regions of h_dst (each dst_cap / G rounded down to a multiple of 16 bytes, the g-th starting at g times
 * that); the offsets are absolute within h_dst.  Requires dst_cap >= G * ceil(n_blocks / G) * align16(bound), else
 * CRYO_E_DSTSIZE.  One handle: exactly cryo_codec_recode_blocks. */
int cryo_multi_recode_blocks(cryo_multi *m, int src_method, const void *const *h_src, const uint32_t *h_src_size,
                             size_t n_blocks, size_t block_size, int dst_method, int dst_param,
                             void *h_dst, size_t dst_cap, uint64_t *h_out_off, uint32_t *h_out_size, int32_t *h_status);

/* cryo_codec_fetch_blocks across the devices: block i -> handle i mod G.  Handle g packs the tuples of its share, in block
 * order, into a region of its own: block_size * (blocks dealt to handle g) bytes, the regions laid out in handle order from
 * h_dst on (a region that reaches beyond dst_cap is cut there), so dst_cap >= n_blocks * block_size always suffices.  The
 * records come back in call order and their `off` counts from h_dst, but the tuples of different handles do NOT interleave in
 * call order: with more than one handle `off` is not the running sum of the placement rule, within one handle's blocks it is
 * (from the region's start).  *h_total is the end of the last byte used (0: none).  One handle: exactly
 * cryo_codec_fetch_blocks. */
int cryo_multi_fetch_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                            size_t n_blocks, size_t block_size, const uint64_t *h_req_first, const uint16_t *h_pos,
                            void *h_dst, size_t dst_cap, cryo_fetch_result *h_result, uint64_t *h_total);

/* cryo_codec_filter_blocks across the devices: block i -> handle i mod G.  Handle g, whose share is the blocks g, g + G, ..., has
 * one tuple region of block_size * share bytes and one record region of 290 * share records, the regions laid out in handle order
 * from h_dst and h_rec on (a region that reaches beyond its cap is cut there, so dst_cap >= n_blocks * block_size and rec_cap >=
 * n_blocks * 290 always suffice).  The block table comes back in call order and finds everything: `off` counts from h_dst and
 * rec_first from h_rec, but with more than one handle they are running sums only within one handle's blocks (from its regions'
 * starts).  h_total[0] / h_total[1]: the end of the last byte / record used (0: none); with CRYO_FILTER_COUNT_ONLY both are 0.
 * One handle: exactly cryo_codec_filter_blocks. */
int cryo_multi_filter_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                             size_t n_blocks, size_t block_size, const cryo_filter *f,
                             void *h_dst, size_t dst_cap, cryo_filter_rec *h_rec, size_t rec_cap,
                             cryo_filter_block *h_blocks, uint64_t *h_total);

/* cryo_codec_agg_blocks across the devices: block i -> handle i mod G.  Rows and cells have a fixed size per block and land in
 * call order (block i's row at h_blocks[i], its cells from h_cells[i * ncols] on), so no per-handle regions are needed.  One
 * handle: exactly cryo_codec_agg_blocks. */
int cryo_multi_agg_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                          size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_agg *agg,
                          cryo_agg_block *h_blocks, cryo_agg_cell *h_cells);

/* cryo_codec_group_blocks across the devices: block i -> handle i mod G.  The host lays each handle's records and cells back into
 * call order and rebases first_group, so rows, records, cells and *h_total are byte for byte the single-handle call's and no
 * per-handle regions are needed; more groups than group_cap: CRYO_E_DSTSIZE.  One handle: exactly cryo_codec_group_blocks. */
int cryo_multi_group_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                            size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_group *grp,
                            const cryo_agg *agg, cryo_group_block *h_blocks, cryo_group_rec *h_groups, size_t group_cap,
                            cryo_agg_cell *h_cells, uint64_t *h_total);

/* cryo_codec_project_blocks across the devices: block i -> handle i mod G.  Regions as in cryo_multi_filter_blocks: handle g, whose
 * share is the blocks g, g + G, ..., has one row region of 290 * share rows and one record region of 290 * share records, the
 * regions laid out in handle order from h_rows and h_rec on (a region that reaches beyond its cap is cut there, so row_cap >= 290
 * * n_blocks and rec_cap >= 290 * n_blocks always suffice).  The block table comes back in call order and finds everything:
 * row_first counts from h_rows and rec_first from h_rec, but with more than one handle they are running sums only within one
 * handle's blocks (from its regions' starts).  h_total[0] / h_total[1]: the end of the last row / record used (0: none).  One
 * handle: exactly cryo_codec_project_blocks. */
int cryo_multi_project_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                              size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_project *prj,
                              void *h_rows, size_t row_cap, cryo_project_rec *h_rec, size_t rec_cap,
                              cryo_project_block *h_blocks, uint64_t *h_total);

/* cryo_codec_topn_blocks across the devices: block i -> handle i mod G.  cryo_multi_project_blocks' scheme with min(limit, 290)
 * entries per block: handle g, whose share is the blocks g, g + G, ..., owns one region of min(limit, 290) * share entries of
 * h_rows and of h_rec alike, the regions laid out in handle order (a region that reaches beyond row_cap is cut there, so row_cap
 * >= min(limit, 290) * n_blocks always suffices).  The block table comes back in call order and finds everything: row_first
 * counts from h_rows / h_rec, but with more than one handle it is a running sum only within one handle's blocks (from its
 * region's start).  *h_total: the end of the last entry used (0: none).  One handle: exactly cryo_codec_topn_blocks. */
int cryo_multi_topn_blocks(cryo_multi *m, int method, const void *const *h_src, const uint32_t *h_src_size,
                           size_t n_blocks, size_t block_size, const cryo_filter *f, const cryo_order *ord,
                           const cryo_project *prj, void *h_rows, cryo_topn_rec *h_rec, size_t row_cap,
                           cryo_topn_block *h_blocks, uint64_t *h_total);

/* ---- batch helpers used by staging, tests and the benchmark ---- */

/* synthetic cryo blocks (include/cryo_synth.h) on device: slot k holds job block
 * first_block + k*block_step (block_step = N, first_block = rank gives rank's round-robin share) */
int cryo_codec_synth_batch(cryo_codec *c, uint64_t seed, uint64_t first_block, uint64_t block_step,
                           uint64_t n_blocks, uint32_t block_size, int dist, void *d_dst, uint64_t dst_stride);
/* The LZ4 sequence index read back (test support: a wrong row only costs decode speed, so no decode result shows it).
 * cryo_codec_lz4_index_cap: 16-bit entries per row of the one-walker index of a block size (0: block_size is 0).
 * cryo_codec_lz4_index_rows: builds the one-walker-per-block index of the batch (streams as for
 * cryo_codec_decompress_batch) with the form asked for (1 or 2 of CRYO_OPT_LZ4_INDEX_FORM; 0 = what automatic takes)
 * in handle workspace and copies it into the caller's device buffers: d_entries[i * cap + j] = low 16 bits of the offset
 * of token j of block i for j < d_counts[i]; entries behind the count are unspecified.  Asynchronous on the handle's stream. */
uint32_t cryo_codec_lz4_index_cap(uint32_t block_size);
int cryo_codec_lz4_index_rows(cryo_codec *c, const void *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                              uint32_t block_size, uint64_t n_blocks, int form, uint16_t *d_entries, uint32_t *d_counts);
/* per-block 64-bit checksum (same function as cryo_checksum64() below) */
int cryo_codec_checksum_batch(cryo_codec *c, const void *d_src, uint64_t src_stride,
                              const uint32_t *d_sizes /* or NULL: fixed_size */, uint32_t fixed_size,
                              uint64_t n_blocks, uint64_t *d_sums);
/* number of blocks whose bytes differ between two batches -> *d_mismatch (device u64, accumulated) */
int cryo_codec_compare_batch(cryo_codec *c, const void *d_a, uint64_t a_stride,
                             const void *d_b, uint64_t b_stride, uint32_t block_size,
                             uint64_t n_blocks, uint64_t *d_mismatch);
/* host-side reference of the checksum, for tests */
uint64_t cryo_checksum64(const void *p, size_t n);
/* Every handle-owned buffer filled with one byte over its whole capacity (test support: a handle's buffers are grow-only, never
 * cleared and shared between very different calls, so a call is correct only if it writes what it reads; a test fills them with
 * a hostile byte between two calls and compares the second call's results with the reference).  Waits for all the handle's
 * streams (main, transfer, zstd lanes and sides, the LZ4 side stream), fills the device buffers with hipMemsetAsync on the main stream and, once
 * that stream is idle again, the pinned staging buffers with a host memset: nothing is pending when it returns.  *out (may be NULL): the bytes filled per buffer, 0 for one that is not
 * allocated; a capacity that differs between two reports means the buffer was reallocated in between.  Not filled: the keyed
 * pool (it holds valid blocks by contract).  The device copies of set-key lists and byte-string constants are not cached: the
 * device-resident scan calls rebuild them in d_keytab at every call, the host-buffer calls in the pinned and meta staging, so
 * they are filled with the rest.  Allocates nothing, frees nothing, changes no option; on no production path. */
typedef struct {
    uint64_t d_ws, d_vfy, d_rec;          /* kernels' workspace, verification / scan chunk, recode chunk */
    uint64_t hb_src, hb_dst, hb_meta;     /* device staging of the host-buffer calls */
    uint64_t d_in, d_out, d_scalars;      /* single-block scratch; d_scalars: its offset, size and status words (16 bytes) */
    uint64_t d_keytab;                    /* key table of the device-resident scan calls */
    uint64_t pin, pipe_pin[4];            /* pinned host staging */
} cryo_codec_fill_report;
int cryo_codec_debug_fill(cryo_codec *c, int value, cryo_codec_fill_report *out);

/* ---- timing on the handle's stream (HIP events) ---- */
int cryo_codec_timer_start(cryo_codec *c);
/* records the end event, waits for it, returns elapsed milliseconds */
int cryo_codec_timer_stop(cryo_codec *c, float *ms);

/* ---- counters (SURVEY.md section 5 "metrics") ---- */
typedef struct {
    uint64_t blocks_compressed, blocks_decompressed;
    uint64_t bytes_in, bytes_out;   /* uncompressed bytes through compress / decompress */
    uint64_t launches;
} cryo_codec_counters;
int cryo_codec_get_counters(const cryo_codec *c, cryo_codec_counters *out);

#ifdef __cplusplus
}
#endif
#endif /* CRYO_CODEC_H */
