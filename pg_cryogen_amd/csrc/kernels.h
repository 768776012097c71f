/*
 * kernels.h -- internal launcher interface between the C-ABI host code
 * (cryo_codec.cpp) and the gfx950 kernels.  Not installed; the public surface
 * is include/cryo_codec.h.
 */
#ifndef CRYO_KERNELS_H
#define CRYO_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "cryo_codec.h"
#include "heap_block.h"

/* Tuning and debugging switches read from the environment exist in -DCRYO_DEBUG builds only (the A/B builds under
 * profiles/): the product library reads no environment variable but CRYO_HOST_THREADS (cryo_codec.cpp); what a
 * deployment may change is a per-handle option (cryo_codec_set_option). */
static inline const char *cryo_tuning_env(const char *name)
{
#ifdef CRYO_DEBUG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

namespace cryo {

/* synthetic cryo blocks, include/cryo_synth.h */
hipError_t launch_synth(hipStream_t s, uint64_t seed, uint64_t first_block, uint64_t block_step, uint64_t n_blocks,
                        uint32_t block_size, int dist, uint8_t *d_dst, uint64_t dst_stride);

hipError_t launch_checksum(hipStream_t s, const uint8_t *d_src, uint64_t src_stride,
                           const uint32_t *d_sizes, uint32_t fixed_size, uint64_t n_blocks,
                           uint64_t *d_sums);

hipError_t launch_compare(hipStream_t s, const uint8_t *d_a, uint64_t a_stride, const uint8_t *d_b,
                          uint64_t b_stride, uint32_t block_size, uint64_t n_blocks,
                          uint64_t *d_mismatch);

/* device-resident pool: up to 64 blocks per launch from pool slots (by value: no transfer towards the device) to
 * slots first .. first+count-1 of a contiguous staging area */
struct GatherSlots { uint32_t slot[64]; };
hipError_t launch_gather_blocks(hipStream_t s, const uint8_t *d_pool, const GatherSlots &slots, uint32_t count, uint8_t *d_dst,
                                uint32_t block_size, uint32_t first);

/* LZ4 block format */
constexpr uint32_t kLz4IndexResidentLanes = 65536u;
/* per-handle options (include/cryo_codec.h: CRYO_OPT_LZ4_DECODE_PATH, CRYO_OPT_LZ4_INDEX_WALKERS); 0 = automatic */
struct Lz4DecodeOpts {
    int path = 0;    /* 1: in-wave parse kernel, 2: sequence index + indexed decoder, 3: few blocks, every output byte in parallel (lz4_lat.hip) */
    int walkers = 0; /* walkers per block of the index pass (power of two, 1..64) */
    int waves = 0;   /* waves per block of the indexed decoder: 1 = k_lz4_dec_seq, 2 = k_lz4_dec_dual, 0 = by the batch size */
    int index_form = 0; /* index pass of a one-walker plan: 1 = k_lz4_index, 2 = k_lz4_idx_pair (lz4_index_pair.hip), 0 = automatic */
    /* a low-priority side stream with its events (created by the handle, may be null): the last, partial round of a batch
     * that fills the chip once or a few times is decoded there with two waves per block (lz4_dec2.hip, launch_dec_seq) */
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int cus = 0;     /* compute units of the handle's device (hipDeviceProp.multiProcessorCount; 0: an MI355X's 256) */
};
hipError_t launch_lz4_decompress(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off,
                                 const uint32_t *d_src_size, uint8_t *d_dst, uint64_t dst_stride,
                                 uint32_t block_size, uint64_t n_blocks, int32_t *d_status, void *d_workspace,
                                 size_t workspace_bytes, const Lz4DecodeOpts &opts);
/* bytes of workspace the sequence-index pass of this batch wants (0: the batch is decoded without one) */
size_t lz4_decompress_workspace(uint64_t n_blocks, uint32_t block_size, const Lz4DecodeOpts &opts);
/* which path a batch takes: 0 = in-wave parse kernel (k_lz4_dec_ring), else the walkers per block of the index pass */
uint32_t lz4_decode_plan(uint64_t n_blocks, uint32_t block_size, const Lz4DecodeOpts &opts);
/* lz4_index.hip: the sequence index.  Workspace layout: n_blocks rows of `cap` 16-bit entries; a row = S sub-rows of
 * [ext entries: extension of the left neighbour][cap_main entries: the segment's own records]; 64 x 32 bytes of dummy
 * slots; one uint2 descriptor per (block, segment): x = entries used in the extension | first valid own record << 16,
 * y = valid own records */
struct Lz4IndexLayout {
    uint32_t logS, cap_main, ext, cap;
    size_t dummy_off, seg_off, bytes;
};
Lz4IndexLayout lz4_index_layout(uint64_t n_blocks, uint32_t block_size, uint32_t walkers);
hipError_t launch_lz4_index(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                            uint64_t n_blocks, uint32_t block_size, void *d_workspace, const Lz4IndexLayout &L);
/* lz4_index_pair.hip: the same rows and descriptors for L.logS == 0, by pairs of waves (a walker and a feeder on the same rings) */
hipError_t launch_lz4_index_pair(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                                 uint64_t n_blocks, uint32_t block_size, void *d_workspace, const Lz4IndexLayout &L);
/* which of the two a one-walker plan takes: `form` as CRYO_OPT_LZ4_INDEX_FORM.  Automatic is the pair for batches that are
 * resident at once (one wave of 64 walkers per SIMD: 256 blocks per compute unit); a batch of several rounds loses with it
 * (131 072 x 128 KiB: 15.6 -> 16.3 ms, profiles/lz4_index_pair.txt) and keeps k_lz4_index */
inline bool lz4_index_use_pair(const Lz4IndexLayout &L, int form, uint64_t n_blocks, int cus)
{
    if (L.logS != 0u || form == 1) return false;
    return form == 2 || n_blocks <= (uint64_t)(cus > 0 ? cus : 256) * 256u;
}
hipError_t launch_lz4_index_form(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                                 uint64_t n_blocks, uint32_t block_size, void *d_workspace, const Lz4IndexLayout &L, int form, int cus);
/* test support (cryo_codec_lz4_index_rows): the counts of a one-walker index, out of its descriptors */
hipError_t launch_lz4_index_counts(hipStream_t s, const void *d_workspace, const Lz4IndexLayout &L, uint64_t n_blocks, uint32_t *d_counts);
/* few blocks per call: a workgroup of up to 1 024 walkers per block, direct loads (lz4_index.hip, k_lz4_index_few) */
Lz4IndexLayout lz4_index_layout_few(uint64_t n_blocks, uint32_t block_size);
const uint32_t *lz4_index_few_failed(const void *d_workspace, const Lz4IndexLayout &L, uint64_t n_blocks); /* one word per block: 1 = no index */
hipError_t launch_lz4_index_few(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                                uint64_t n_blocks, uint32_t block_size, void *d_workspace, const Lz4IndexLayout &L);
/* Per-block routing of batches indexed with several walkers per block: a block that compressed to more than 15/16 of
 * its size is almost all literal runs -- a walker that starts at a guessed position inside one hops through it ~7 bytes at
 * a time where the true chain takes one hop, and the copy is one long run either way -- so such blocks are left to the
 * in-wave parser (k_lz4_dec_ring, launched over the same batch with the opposite filter).  Measured at 16 384 x 128 KiB:
 * incompressible blocks 961 GB/s through the index, 2 203 through the parser; acceleration-50 streams (ratio 1.05) 309
 * against 378 at 8 192 blocks; the headline data (ratio 1.29, a token every 16 bytes) 920 against 529
 * (profiles/r03_lz4_decode_batch_shapes.txt). */
__host__ __device__ inline bool lz4_literal_heavy(uint32_t csize, uint32_t block_size) { return csize > block_size - (block_size >> 4); }
/* A stream of less than 16 KiB gets ONE index walker whatever the batch: it is walked in ~0.3 ms at most, and such streams are
 * the highly periodic ones (blocks of fixed-width rows: a token every 3-5 bytes, every sequence alike) on which chains started
 * at guessed positions run beside the true one for ever -- the hand-over fails and the block is walked again by one walker
 * anyway (8 192 x 1 MiB `int4`: 1.0-1.1 ms of index pass; profiles/r05_index_run255.txt).  Used by k_lz4_index, k_lz4_few_* and
 * lz4_lat.hip alike: they must cut a block into the same segments. */
__host__ __device__ inline bool lz4_index_one_walker(uint32_t csize) { return csize < 16384u; }
hipError_t launch_lz4_dec_ring(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                               uint8_t *d_dst, uint64_t dst_stride, uint32_t block_size, uint64_t n_blocks, int32_t *d_status,
                               bool only_literal_heavy, const uint32_t *d_done = nullptr /* blocks marked there are skipped */);
/* lz4_dec2.hip: index pass + the decoder that consumes it */
hipError_t launch_lz4_decompress_indexed(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off,
                                         const uint32_t *d_src_size, uint8_t *d_dst, uint64_t dst_stride,
                                         uint32_t block_size, uint64_t n_blocks, int32_t *d_status, void *d_workspace,
                                         size_t workspace_bytes, uint32_t walkers, int waves = 0, const Lz4DecodeOpts *opts = nullptr);

/* lz4_lat.hip: few blocks per call (the reference's own call shapes) */
bool lz4_latency_eligible(uint64_t n_blocks, uint32_t block_size);
size_t lz4_latency_workspace(uint64_t n_blocks, uint32_t block_size);
hipError_t launch_lz4_decompress_latency(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off,
                                         const uint32_t *d_src_size, uint8_t *d_dst, uint64_t dst_stride,
                                         uint32_t block_size, uint64_t n_blocks, int32_t *d_status, void *d_workspace,
                                         size_t workspace_bytes);

hipError_t launch_lz4_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_stride,
                               uint32_t block_size, uint64_t n_blocks, uint8_t *d_dst,
                               uint64_t dst_stride, int accel, uint32_t *d_out_size,
                               int32_t *d_status);

hipError_t launch_lz4_compress_batch64(hipStream_t s, const uint8_t *d_src, uint64_t src_stride,
                                       uint32_t block_size, uint64_t n_blocks, uint8_t *d_dst,
                                       uint64_t dst_stride, int accel, uint32_t *d_out_size, int32_t *d_status);

/* zstd frames.  `aux` (optional): two side streams + events the batch pipeline alternates its tiles on;
 * the work is ordered after everything already queued on `s`, and `s` waits for it before returning. */
constexpr int kZstdLanes = 8; /* side streams a decode call may spread its tiles over */
struct ZstdAux {
    hipStream_t lane[kZstdLanes];
    hipEvent_t fork, join[kZstdLanes];
    /* inside a tile the Huffman stage (k_zhufw, k_zmove, k_zhuf) and the sequence stage (k_zchain4, k_zmat) depend on
     * k_zplan only and meet in k_zexec: calls of few tiles run them side by side (round 5) */
    hipStream_t side[kZstdLanes];
    hipEvent_t planned[kZstdLanes], seqs_done[kZstdLanes];
};
hipError_t launch_zstd_decompress(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off,
                                  const uint32_t *d_src_size, uint8_t *d_dst, uint64_t dst_stride,
                                  uint32_t block_size, uint64_t n_blocks, int32_t *d_status,
                                  void *d_workspace, size_t workspace_bytes, const ZstdAux *aux, int path);
/* max_bytes: the most the call may use; the pipeline plans fewer tiles in flight to fit (one at least) */
size_t zstd_decompress_workspace(uint64_t n_blocks, uint32_t block_size, int path, size_t max_bytes = ~(size_t)0);
/* fused one-wave-per-frame decoder (zstd_dec.hip): small batches, and the pipeline's irregular frames
 * (d_list != nullptr: decode blocks list_base + d_list[0 .. *d_list_n), n_blocks only sizes the grid) */
hipError_t launch_zstd_fused(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off,
                             const uint32_t *d_src_size, uint8_t *d_dst, uint64_t dst_stride,
                             uint32_t block_size, uint64_t n_blocks, int32_t *d_status,
                             void *d_workspace, size_t workspace_bytes, const uint32_t *d_list,
                             const uint32_t *d_list_n, uint64_t list_base);
size_t zstd_fused_workspace(uint64_t n_blocks);

hipError_t launch_zstd_compress(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                uint64_t n_blocks, uint8_t *d_dst, uint64_t dst_stride, int level,
                                uint32_t *d_out_size, int32_t *d_status, void *d_workspace, size_t workspace_bytes);
size_t zstd_compress_workspace(uint64_t n_blocks, int level, uint32_t block_size);
bool zstd_compress_supported(int level, uint32_t block_size);

/* segment-parallel encode (CRYO_OPT_ENCODE_SEGMENT_BYTES; enc_seg.hip): ceil(block_size / seg_bytes) waves per block, one
 * valid stream per block that is not the libraries' own output */
uint32_t enc_seg_count(uint32_t block_size, uint32_t seg_bytes);
size_t lz4_compress_segmented_workspace(uint64_t n_blocks, uint32_t block_size, uint32_t seg_bytes);
hipError_t launch_lz4_compress_segmented(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                         uint64_t n_blocks, uint8_t *d_dst, uint64_t dst_stride, int accel, uint32_t seg_bytes,
                                         uint32_t *d_out_size, int32_t *d_status, void *d_ws, size_t ws_bytes);
/* the level's strategy lies in 1 (`fast`) .. max_strategy (at most 6, `btlazy2`; CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY) */
bool zstd_segment_supported(int level, uint32_t block_size, int max_strategy);
size_t zstd_compress_segmented_workspace(uint64_t n_blocks, int level, uint32_t block_size, uint32_t seg_bytes);
/* trailer: bytes the frame must leave room for behind its last block within the bound (4: a content checksum follows) */
hipError_t launch_zstd_compress_segmented(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                          uint64_t n_blocks, uint8_t *d_dst, uint64_t dst_stride, int level, uint32_t seg_bytes,
                                          uint32_t *d_out_size, int32_t *d_status, void *d_workspace, size_t workspace_bytes,
                                          uint32_t trailer = 0);
/* enc_seg.hip internals shared with zstd_enc.hip */
size_t zstd_seg_scratch_bytes(uint64_t items, uint32_t seg_bytes);
uint64_t zstd_seg_slot_stride(uint32_t seg_bytes);
hipError_t launch_zstd_seg_concat(hipStream_t s, uint64_t n_blocks, uint32_t nseg, uint32_t seg_bytes, const uint8_t *d_seg,
                                  const uint32_t *d_seg_size, uint32_t *d_seg_off, const uint8_t *head, uint32_t head_len,
                                  uint32_t bound, uint32_t trailer, uint8_t *d_dst, uint64_t dst_stride, uint32_t *d_out_size,
                                  int32_t *d_status);

/* content checksums of zstd frames (xxh64.hip, CRYO_OPT_ZSTD_CHECKSUM): for every block whose status is CRYO_OK, the frame's
 * checksum flag, XXH64 of its B input bytes (low 32 bits) at d_dst + out_size[i], and out_size[i] + 4 */
hipError_t launch_zstd_checksum_append(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                       uint64_t n_blocks, uint8_t *d_dst, uint64_t dst_stride, uint32_t *d_out_size,
                                       int32_t *d_status);

/* write verification (verify.hip): the stream table of a chunk's decode, the compare, the per-block verdict.  e0 / e1: the
 * "edge" blocks whose slots were copied into padded workspace (~0: none) */
hipError_t launch_verify_prep(hipStream_t s, uint64_t lo, uint32_t cnt, const uint64_t *d_comp_off, uint64_t comp_stride,
                              const uint32_t *d_comp_size, const int32_t *d_enc_status, uint64_t e0, uint64_t e1,
                              uint64_t edge_stride, uint64_t *d_off, uint32_t *d_size, uint32_t *d_first);
hipError_t launch_verify_compare(hipStream_t s, const uint8_t *d_raw, uint64_t raw_stride, const uint8_t *d_dec,
                                 uint64_t dec_stride, uint32_t block_size, uint64_t lo, uint32_t cnt, const uint32_t *d_size,
                                 const int32_t *d_dec_status, uint64_t e0, uint64_t e1, uint32_t *d_first);
hipError_t launch_verify_fold(hipStream_t s, uint64_t lo, uint32_t cnt, const uint32_t *d_size, const int32_t *d_dec_status,
                              uint64_t e0, uint64_t e1, bool has_enc_status, int32_t *d_status, uint32_t *d_first);

/* the stored-block check (check.hip) on one decoded chunk of cnt blocks (block k at d_dec + k * dec_stride, 16-byte aligned
 * rows; its decoder status in d_dec_status[k]): k_check_items, k_check_zero, k_check_fold.  d_verdict, d_gap, d_first: cnt
 * entries of scratch; d_result[k] = {reason, offset} (cryo_check_result) */
hipError_t launch_check(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                        const int32_t *d_dec_status, uint2 *d_verdict, uint2 *d_gap, uint32_t *d_first, uint2 *d_result);

/* recompression (recode.hip) on one chunk of cnt encoded blocks in slots of slot_stride bytes (a multiple of 16, 16-byte
 * aligned).  k_recode_offsets: d_status[k] (in: the encoder's) and d_size[k] become the block's final status and size (0 unless
 * the decoder's status and the encoder's are both CRYO_OK); d_off[k] = base + the sum of align16(d_size[j]), j < k; d_off[cnt]
 * = base + *d_total.  k_recode_pack: stream k to d_packed + d_off[k], pad bytes zero; d_packed holds base + *d_total bytes
 * (at most base + cnt * slot_stride).  cus: compute units of the device (0: an MI355X's 256) */
hipError_t launch_recode_offsets(hipStream_t s, uint32_t cnt, uint64_t slot_stride, const int32_t *d_dec_status, int32_t *d_status,
                                 uint32_t *d_size, uint64_t base, uint64_t *d_off, uint64_t *d_total);
hipError_t launch_recode_pack(hipStream_t s, uint32_t cnt, const uint8_t *d_slots, uint64_t slot_stride, const uint32_t *d_size,
                              const uint64_t *d_off, const uint64_t *d_total, uint8_t *d_packed, int cus);

/* the tuple fetch (fetch.hip) on one decoded chunk of cnt blocks (block k at d_dec + k * dec_stride, 16-byte aligned rows; its
 * decoder status in d_dec_status[k]): k_fetch_items, k_fetch_offsets, k_fetch_copy.  Block k owns requests d_req_first[k] ..
 * d_req_first[k + 1] - 1 of d_pos / d_result / d_side (indices within the whole call, cut to n_req); d_result[r] = {status, len,
 * off} (cryo_fetch_result, 16-byte aligned), d_side: 8 bytes per request of scratch; d_sum: cnt, d_base: cnt + 1 entries of
 * scratch; *d_running: the packed total before the chunk in, after it out.  The chunk's tuples go to d_dst (8-byte aligned) at
 * their offset within the call, or -- chunk_relative -- at that offset less the chunk's first; a tuple that would end beyond
 * dst_cap is not written.  cus: compute units of the device (0: an MI355X's 256) */
hipError_t launch_fetch(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                        const int32_t *d_dec_status, const uint64_t *d_req_first, const uint16_t *d_pos, uint64_t n_req,
                        uint4 *d_result, uint2 *d_side, uint64_t *d_sum, uint64_t *d_base, uint64_t *d_running, uint8_t *d_dst,
                        uint64_t dst_cap, bool chunk_relative, int cus);

/* ---- the five scan calls: filter (filter.hip), aggregate (agg.hip), group (group.hip), project (project.hip), top-N (topn.hip) ----
 * Each works on one decoded chunk (ScanChunk) under one descriptor (ScanDesc) and takes what is its own in a struct of its
 * own; a call site names the fields it sets.  The caller (cryo_codec.cpp, *_desc_ok) has validated the descriptor; X_launch_ok
 * below is what launch_X asks of its arguments beyond that.  Which block kernel runs is scan_route's and group_route's; the
 * block-kernel launch itself is stated once per call, where the call's units share it (scan_sweep.h: scan_block_launch,
 * filter_launch, agg_launch, project_launch; group_lds.h: group_launch; topn.hip: topn_launch). */

/* what a launcher is told about the decoded chunk and the device: cnt blocks, block k at d_dec + k * dec_stride (16-byte aligned
 * rows), its decoder status in d_dec_status[k]; cus: compute units of the device (0: an MI355X's 256) */
struct ScanChunk {
    hipStream_t stream = nullptr;
    const uint8_t *d_dec = nullptr;
    uint64_t dec_stride = 0;
    uint32_t block_size = 0, cnt = 0;
    const int32_t *d_dec_status = nullptr;
    int cus = 0;
};

/* what every scan call tells its kernels about the relation and the keys (the host fills it: cryo_codec.cpp, scan_desc_device,
 * key_table_device).  d_atts: natts entries of {i16 attlen, u8 attalign, u8 0}; d_keys: nkeys <= 4 entries of cryo_scan_key.  A key
 * may have type CRYO_KEY_BYTES, a float type, or be a set key or a pattern key when d_keys is the library's key table
 * (key_table_fill): its value is then the mapped constant (float_map) or the device address of its constant, its sorted members
 * or its compiled pattern, 8-byte aligned and zero-padded to a multiple of 8 */
struct ScanDesc {
    const void *d_atts = nullptr, *d_keys = nullptr; /* device */
    uint32_t nkeys = 0, max_att = 0;                 /* max_att: the highest column the walk has to reach */
    uint32_t truth = 0;                              /* 0: the keys are ANDed by the kernels' <false> instantiation; otherwise the
                                                        truth table of the <true> one (scan_truth), at most 16 bits */
    bool floats = false;                             /* a float key or a float aggregate column: the float kernels, which have
                                                        the truth table's verdict path alone (truth is not 0 then) */
    bool like = false;                               /* a pattern key (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE): the pattern kernels, which
                                                        also do what the float kernels do (truth is not 0 then) */
    const void *d_buckets = nullptr;                 /* device: the grouping's bucket table under CRYO_GROUP_BUCKETS (truth is not 0
                                                        then), else null: two entries of 24 bytes (cryo_bucket; a list's n its distinct
                                                        boundaries and value the device address of the library's sorted copy) */
    uint32_t text = 0;                               /* the grouping's: bit j set when group column j is a byte string
                                                        (CRYO_GROUP_TEXT; truth is not 0 then) */
};

/* The block kernel a descriptor reaches.  like goes over floats goes over a table: a pattern kernel also does what the float
 * kernel does, a float kernel what the <true> one does.  The pattern kernels have names of their own and live, each with its
 * launcher (launch_*l_*), in a unit of their own -- the source of the float sibling compiled a second time with CRYO_LIKE_UNIT
 * (the Makefile's %_like.o) --, so that a descriptor without such a key runs the code it ran.
 *   route        filter                 aggregate           project                 top-N
 *   kRoutePlain  k_filter_match<false>  k_agg_block<false>  k_project_block<false>  k_topn_block<false>   truth == 0
 *   kRouteTable  k_filter_match<true>   k_agg_block<true>   k_project_block<true>   k_topn_block<true>    truth != 0
 *   kRouteFloat  k_filterf_match        k_aggf_block        k_projectf_block        k_topnf_block         floats
 *   kRouteLike   k_filterl_match        k_aggl_block        k_projectl_block        k_topnl_block         like */
enum ScanRoute { kRoutePlain, kRouteTable, kRouteFloat, kRouteLike };
inline ScanRoute scan_route(uint32_t truth, bool floats, bool like)
{
    return like ? kRouteLike : floats ? kRouteFloat : truth ? kRouteTable : kRoutePlain;
}
/* The grouped scan's: a byte-string group column (text) goes over buckets, and either over the four routes above.
 *   route                                                 text    buckets  floats  like
 *   kGroupPlain / kGroupTable  k_group_block<false> / <true>  0   no       no      no    (truth == 0 / != 0)
 *   kGroupFloat        k_groupf_block                     0       no       yes     no
 *   kGroupLike         k_groupl_block                     0       no       any     yes
 *   kGroupBucket       k_groupb_block<false>              0       yes      no      no
 *   kGroupBucketFloat  k_groupb_block<true>               0       yes      yes     no
 *   kGroupBucketLike   k_groupbl_block                    0       yes      any     yes
 *   kGroupText         k_groupt_block<false>              not 0   any      no      no
 *   kGroupTextFloat    k_groupt_block<true>               not 0   any      yes     no
 *   kGroupTextLike     k_grouptl_block                    not 0   any      any     yes
 * (text with buckets never gets here: group_launch_ok) */
enum GroupRoute {
    kGroupPlain, kGroupTable, kGroupFloat, kGroupLike, kGroupBucket, kGroupBucketFloat, kGroupBucketLike, kGroupText, kGroupTextFloat,
    kGroupTextLike
};
inline GroupRoute group_route(uint32_t text, bool has_buckets, uint32_t truth, bool floats, bool like)
{
    if (text) return like ? kGroupTextLike : floats ? kGroupTextFloat : kGroupText;
    if (has_buckets) return like ? kGroupBucketLike : floats ? kGroupBucketFloat : kGroupBucket;
    return like ? kGroupLike : floats ? kGroupFloat : truth ? kGroupTable : kGroupPlain;
}

/* the block kernels' nkeys argument: the key count below the truth table, which the <true>, float and pattern kernels find in
 * its high half (filter_walk.h, walk_tuple) */
inline uint32_t scan_nkeys_arg(uint32_t nkeys, uint32_t truth) { return nkeys | truth << 16; }

/* the grid of a call's copy kernel: four workgroups per compute unit (256 units when cus is 0), at most cap, at least one */
inline uint32_t scan_copy_grid(int cus, uint64_t cap)
{
    const uint64_t grid = (uint64_t)(cus > 0 ? cus : 256) * 4u;
    return (uint32_t)(grid > cap ? (cap > 0u ? cap : 1u) : grid);
}

/* a block's row of every side area: the items it can hold */
inline uint32_t filter_side_stride(uint32_t block_size)
{
    const uint32_t fit = (block_size - 8u) / 8u; /* lower <= B: no more item ids than this */
    return fit < kHeapMaxItems ? fit : kHeapMaxItems;
}

/* what the launchers of the five scan calls ask of their arguments alike: the chunk and the block table 16-byte aligned, the
 * keys and -- eight: the call's other 8-byte tables and outputs, ORed -- 8-byte aligned, the column descriptor 4-byte aligned, a
 * block that holds a header and an item, at most four keys, a table of 16 bits, and a table wherever a float or pattern kernel runs */
inline bool scan_launch_ok(const ScanChunk &c, const ScanDesc &d, const void *d_blocks, uintptr_t eight)
{
    return (c.dec_stride & 15u) == 0 && (((uintptr_t)c.d_dec | (uintptr_t)d_blocks) & 15u) == 0 && (((uintptr_t)d.d_keys | eight) & 7u) == 0 &&
           ((uintptr_t)d.d_atts & 3u) == 0 && c.block_size >= 16u && d.nkeys <= 4u && d.truth <= 0xFFFFu &&
           !((d.floats || d.like) && d.truth == 0u);
}

/* the scan filter: k_filter_match, k_filter_offsets, k_filter_copy.  An undecided tuple gets a record {pos, 9, 0} and counts in
 * n_bad.  d_blocks: the chunk's rows of the block table (cryo_filter_block).  Scratch: d_side 16 bytes per possible item (cnt *
 * filter_side_stride(block_size) entries, 16-byte aligned), d_sum 2 * cnt and d_base 2 * (cnt + 1) entries.  d_running: the two
 * totals {bytes, records} before the chunk in, after it out.  The chunk's tuples go to d_dst and its records to d_rec at their
 * places within the call, or -- chunk_relative -- at those less the chunk's first; a tuple that would end beyond dst_cap and a
 * record at or beyond rec_cap are not written.  count_only: k_filter_match alone; rec_first and off of the table are 0 and
 * nothing else is written */
struct FilterLaunch {
    bool count_only = false;
    uint4 *d_blocks = nullptr, *d_side = nullptr;
    uint64_t *d_sum = nullptr, *d_base = nullptr, *d_running = nullptr;
    uint8_t *d_dst = nullptr;
    uint64_t dst_cap = 0;
    uint2 *d_rec = nullptr;
    uint64_t rec_cap = 0;
    bool chunk_relative = false;
};
inline bool filter_launch_ok(const ScanChunk &c, const ScanDesc &d, const FilterLaunch &f)
{
    return scan_launch_ok(c, d, f.d_blocks, (uintptr_t)f.d_dst | (uintptr_t)f.d_rec) && ((uintptr_t)f.d_side & 15u) == 0;
}
hipError_t launch_filter(const ScanChunk &c, const ScanDesc &d, const FilterLaunch &f);
hipError_t launch_filterl_match(const ScanChunk &c, const ScanDesc &d, const FilterLaunch &f); /* filter_like.o */

/* the scan aggregate: the block kernel alone.  d_cols: ncols (1 .. 4) entries of cryo_agg_col; ScanDesc::max_att reaches the
 * highest aggregate column too; an undecided tuple counts in n_bad and is in no cell.  d_blocks: the chunk's rows
 * (cryo_agg_block); d_cells: its cnt * ncols cells (cryo_agg_cell), block k's at k * ncols.  No workspace: the kernel keeps
 * everything in registers and writes only the rows and the cells */
struct AggLaunch {
    const void *d_cols = nullptr;
    uint32_t ncols = 0;
    uint4 *d_blocks = nullptr;
    void *d_cells = nullptr;
};
inline bool agg_launch_ok(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a)
{
    return scan_launch_ok(c, d, a.d_blocks, (uintptr_t)a.d_cells | (uintptr_t)a.d_cols) && a.ncols != 0u && a.ncols <= CRYO_AGG_MAX_COLS;
}
hipError_t launch_agg(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a);
hipError_t launch_aggf(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a); /* agg_float.o */
hipError_t launch_aggl(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a); /* agg_float_like.o */

/* the grouped scan: the block kernel, k_group_offsets, k_group_copy.  d_slots: six entries of cryo_agg_col, the nby (1 .. 2)
 * group columns in entries 0 .. 1, the ncols (0 .. 4) aggregate columns in entries 2 .. 5, every unused entry all zero; an
 * undecided tuple counts in n_bad and is in no group.  d_blocks: the chunk's rows (cryo_group_block).  A group has cpg = ncols +
 * popcount(ScanDesc::text) cells, the aggregate cells first.  Scratch: d_side_rec 24 bytes and d_side_cell 40 * cpg bytes per
 * possible group (cnt * filter_side_stride(block_size) groups).  *d_running: the groups before the chunk in, after it out.  The
 * chunk's records go to d_rec and its cells to d_cells at first_group within the call; nothing at or beyond group_cap groups is
 * written */
struct GroupLaunch {
    const void *d_slots = nullptr;
    uint32_t nby = 0, ncols = 0;
    uint4 *d_blocks = nullptr;
    void *d_side_rec = nullptr, *d_side_cell = nullptr;
    uint64_t *d_running = nullptr;
    void *d_rec = nullptr, *d_cells = nullptr;
    uint64_t group_cap = 0;
};
inline bool group_launch_ok(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g)
{
    const uint32_t cpg = g.ncols + (uint32_t)__builtin_popcount(d.text); /* a group's cells: ncols unless it has key cells */
    return scan_launch_ok(c, d, g.d_blocks,
                          (uintptr_t)g.d_rec | (uintptr_t)g.d_cells | (uintptr_t)g.d_slots | (uintptr_t)g.d_side_rec |
                              (uintptr_t)g.d_side_cell | (uintptr_t)g.d_running | (uintptr_t)d.d_buckets) &&
           !(g.nby == 0u || g.nby > CRYO_GROUP_MAX_BY || g.ncols > CRYO_AGG_MAX_COLS || (d.text >> g.nby) != 0u || (d.text != 0u && d.d_buckets) ||
             ((d.text != 0u || d.d_buckets) && d.truth == 0u) || !g.d_slots || !g.d_side_rec || !g.d_running || (cpg > 0u && !g.d_side_cell) ||
             (g.group_cap > 0u && (!g.d_rec || (cpg > 0u && !g.d_cells))));
}
hipError_t launch_group(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g);
/* launch_group's block kernels in other units, on arguments it has checked */
hipError_t launch_groupf_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g);  /* group_float.o */
hipError_t launch_groupl_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g);  /* group_float_like.o */
hipError_t launch_groupb_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g);  /* group_bucket.o: <d.floats> */
hipError_t launch_groupbl_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g); /* group_bucket_like.o */
hipError_t launch_groupt_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g);  /* group_text.o: <d.floats> */
hipError_t launch_grouptl_block(const ScanChunk &c, const ScanDesc &d, const GroupLaunch &g); /* group_text_like.o */

/* the projecting scan: the block kernel, k_project_offsets, k_project_copy.  d_cols: the staged column table, ncols (1 .. 8)
 * entries of 8 bytes {u16 att, u8 width (the column's attlen: 1, 2, 4, 8), u8 offset within the row (a multiple of the width,
 * below row_bytes), u32 0} -- the walk reads it as cryo_agg_col and looks at att alone; row_bytes the row's size, 8 .. 64 and a
 * multiple of 8 (both from CRYO_PROJECT_COL_OFFSET / CRYO_PROJECT_ROW_BYTES); an undecided tuple gets a record {pos, 9, 0},
 * counts in n_bad and has no row.  d_blocks: the chunk's rows of the block table (cryo_project_block).  Scratch: d_side_rec 8
 * bytes and d_side_rows row_bytes bytes per possible item (cnt * filter_side_stride(block_size) items).  d_running: the two
 * totals {rows, records} before the chunk in, after it out.  The chunk's records go to d_rec and its rows to d_rows at rec_first
 * / row_first within the call; no record at or beyond rec_cap and no row at or beyond row_cap is written */
struct ProjectLaunch {
    const void *d_cols = nullptr;
    uint32_t ncols = 0, row_bytes = 0;
    uint4 *d_blocks = nullptr;
    void *d_side_rec = nullptr, *d_side_rows = nullptr;
    uint64_t *d_running = nullptr;
    void *d_rec = nullptr;
    uint64_t rec_cap = 0;
    void *d_rows = nullptr;
    uint64_t row_cap = 0;
};
inline bool project_launch_ok(const ScanChunk &c, const ScanDesc &d, const ProjectLaunch &p)
{
    return scan_launch_ok(c, d, p.d_blocks,
                          (uintptr_t)p.d_rec | (uintptr_t)p.d_rows | (uintptr_t)p.d_cols | (uintptr_t)p.d_side_rec | (uintptr_t)p.d_side_rows |
                              (uintptr_t)p.d_running) &&
           !(p.ncols == 0u || p.ncols > CRYO_PROJECT_MAX_COLS || p.row_bytes < 8u || p.row_bytes > 8u * CRYO_PROJECT_MAX_COLS ||
             (p.row_bytes & 7u) != 0 || !p.d_cols || !p.d_side_rec || !p.d_side_rows || !p.d_running || (p.rec_cap > 0u && !p.d_rec) ||
             (p.row_cap > 0u && !p.d_rows));
}
hipError_t launch_project(const ScanChunk &c, const ScanDesc &d, const ProjectLaunch &p);
hipError_t launch_projectl_block(const ScanChunk &c, const ScanDesc &d, const ProjectLaunch &p); /* project_like.o */

/* the ordered scan: the block kernel, k_topn_offsets, k_topn_copy.  d_slots: the staged table, ten entries of 8 bytes: entries
 * 0 .. 1 the nby (1 .. 2) order columns {u16 att, u8 type (CRYO_KEY_INT2 .. _INT8, _FLOAT4, _FLOAT8), u8 flags (CRYO_ORDER_*),
 * u32 0}, entries 2 .. 9 ProjectLaunch's column table of ncols (1 .. 8) columns, every unused entry all zero; h_slots: the host's
 * copy of the ten (topn_pack); row_bytes as ProjectLaunch's; limit >= 1; an undecided tuple counts in n_bad and is in no ranking.
 * d_blocks: the chunk's rows of the block table (cryo_topn_block).  Scratch, per possible item (cnt *
 * filter_side_stride(block_size) items): d_side_rec 24 bytes, d_side_rows row_bytes bytes, d_side_ord 4 bytes.  *d_running: the
 * kept rows before the chunk in, after it out.  The chunk's records go to d_rec and its rows to d_rows at row_first within the
 * call; nothing at or beyond row_cap is written */
struct TopnLaunch {
    const void *d_slots = nullptr, *h_slots = nullptr;
    uint32_t nby = 0, ncols = 0, row_bytes = 0, limit = 0;
    uint4 *d_blocks = nullptr;
    void *d_side_rec = nullptr, *d_side_rows = nullptr, *d_side_ord = nullptr;
    uint64_t *d_running = nullptr;
    void *d_rec = nullptr, *d_rows = nullptr;
    uint64_t row_cap = 0;
};
inline bool topn_launch_ok(const ScanChunk &c, const ScanDesc &d, const TopnLaunch &t)
{
    return scan_launch_ok(c, d, t.d_blocks,
                          (uintptr_t)t.d_rec | (uintptr_t)t.d_rows | (uintptr_t)t.d_slots | (uintptr_t)t.d_side_rec | (uintptr_t)t.d_side_rows |
                              (uintptr_t)t.d_running) &&
           !(t.nby == 0u || t.nby > CRYO_ORDER_MAX_BY || t.limit == 0u || t.ncols == 0u || t.ncols > CRYO_PROJECT_MAX_COLS || t.row_bytes < 8u ||
             t.row_bytes > 8u * CRYO_PROJECT_MAX_COLS || (t.row_bytes & 7u) != 0 || !t.d_slots || !t.h_slots || !t.d_side_rec || !t.d_side_rows ||
             !t.d_side_ord || ((uintptr_t)t.d_side_ord & 3u) != 0 || !t.d_running || (t.row_cap > 0u && (!t.d_rec || !t.d_rows)));
}
/* What the top-N block kernel needs of its table after the walk rides in two arguments, packed from the host's copy (topn.hip:
 * why).  ord_bits: byte j (j = 0, 1) describes order column j with the bits below, byte 2 is the mask of the projected columns;
 * row_map: byte j is projected column j's place in the row, its offset (0 .. 56) in bits 0 .. 5 and log2 of its width above.
 * False: a projected column whose width is not 1, 2, 4 or 8, whose offset is no multiple of it, or that ends beyond the row */
constexpr uint32_t kOrdPresent = 1u, kOrdFloat = 2u, kOrdFloat4 = 4u, kOrdNullsFirst = 8u, kOrdDesc = 16u;
inline bool topn_pack(const TopnLaunch &t, uint32_t &ord_bits, uint64_t &row_map)
{
    const cryo_agg_col *h_slots = (const cryo_agg_col *)t.h_slots;
    ord_bits = ((1u << t.ncols) - 1u) << 16;
    row_map = 0;
    for (uint32_t j = 0; j < t.nby; j++) {
        const cryo_agg_col &q = h_slots[j];
        const bool f4 = q.type == CRYO_KEY_FLOAT4, f8 = q.type == CRYO_KEY_FLOAT8;
        ord_bits |= (kOrdPresent | (f4 || f8 ? kOrdFloat : 0u) | (f4 ? kOrdFloat4 : 0u) | ((q.rsv & CRYO_ORDER_NULLS_FIRST) ? kOrdNullsFirst : 0u) |
                     ((q.rsv & CRYO_ORDER_DESC) ? kOrdDesc : 0u))
                    << (8u * j);
    }
    for (uint32_t j = 0; j < t.ncols; j++) {
        const cryo_agg_col &q = h_slots[CRYO_ORDER_MAX_BY + j];
        const uint32_t w = q.type, o = q.rsv;
        if ((w != 1u && w != 2u && w != 4u && w != 8u) || (o & (w - 1u)) != 0 || o + w > t.row_bytes) return false;
        row_map |= (uint64_t)(o | (w == 8u ? 3u : w == 4u ? 2u : w == 2u ? 1u : 0u) << 6) << (8u * j);
    }
    return true;
}
hipError_t launch_topn(const ScanChunk &c, const ScanDesc &d, const TopnLaunch &t);
hipError_t launch_topnl_block(const ScanChunk &c, const ScanDesc &d, const TopnLaunch &t); /* topn_like.o */

} // namespace cryo

#define CRYO_WAVE 64
#define CRYO_ST_OK 0
#define CRYO_ST_CORRUPT (-4)

#endif
