/*
 * cryo_oracle.h -- CPU ORACLE for the cryo-block codec path.
 *
 * THIS IS TEST INFRASTRUCTURE.  Only tests/, __graft_entry__.smoke() and the
 * cpu_baseline leg of bench.py may load it.  The product path
 * (pg_cryogen_amd/, include/) never links, loads or calls anything here.
 *
 * What it restates: the arithmetic behind the reference's codec boundary
 *   compression.c:61-77   lz4_compress   -> LZ4_compress_fast(src,dst,B,LZ4_compressBound(B),accel)
 *   compression.c:79-91   lz4_decompress -> LZ4_decompress_safe(src,dst,csize,B)
 *   compression.c:93-109  zstd_compress  -> ZSTD_compress(dst,ZSTD_compressBound(B),src,B,level)
 *   compression.c:111-123 zstd_decompress-> ZSTD_decompress(dst,B,src,csize)
 * The reference itself holds no codec arithmetic: it links the un-vendored,
 * un-pinned third-party libraries liblz4 / libzstd (reference Makefile:5).
 * Pinned versions for encoder byte-parity: liblz4 1.9.3, libzstd 1.4.8/1.4.9
 * (the versions installed in the build image).  The algorithms restated are
 * the published LZ4 block format and the Zstandard format (RFC 8878), plus the
 * greedy LZ4 "fast" parser and the zstd "fast" strategy as those library
 * versions implement them.
 *
 * Pinning: tests/golden/ holds vectors produced by the real liblz4 1.9.3 /
 * libzstd 1.4.9 on this generator's blocks (tests/golden/make_golden.py is the
 * generating script); tests/test_oracle_*.py check every function here against
 * them and, where the libraries can be dlopen'ed, against the live libraries.
 */
#ifndef CRYO_ORACLE_H
#define CRYO_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* synthetic block generator (spec: include/cryo_synth.h) */
void cryo_oracle_synth_block(uint64_t seed, uint64_t block_index, uint32_t block_size, int dist,
                             uint8_t *out);

/* LZ4 block codec (liblz4 1.9.3 semantics) */
size_t cryo_oracle_lz4_bound(size_t n);
/* returns compressed size, 0 on failure (dst too small for the bound path) */
size_t cryo_oracle_lz4_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, int accel);
/* returns decoded size (>=0) or -1 on malformed input, like LZ4_decompress_safe */
long cryo_oracle_lz4_decompress(const uint8_t *src, size_t csize, uint8_t *dst, size_t cap);

/* zstd (libzstd 1.4.x semantics) */
size_t cryo_oracle_zstd_bound(size_t n);
/* returns decoded size or -1 on malformed input, like ZSTD_decompress */
long cryo_oracle_zstd_decompress(const uint8_t *src, size_t csize, uint8_t *dst, size_t cap);
/* returns frame size; every level -5…22 (all nine strategies, see zstd_enc_oracle.c; sources up to 1 MiB at the
 * optimal-parser levels), 0 if unsupported */
size_t cryo_oracle_zstd_compress(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, int level);
/* the strategy (1 fast .. 9 btultra2) the encoder above takes for a source of n bytes at a level; 0 if unsupported */
int cryo_oracle_zstd_enc_strategy(int level, size_t n);

/* Branch counters of the encoder's entropy stage (literals, Huffman, sequence tables, sequence bitstream): how often each
 * branch was taken since the last reset, over all blocks of all cryo_oracle_zstd_compress calls.  They show what no frame
 * shows (the depth clip, the secondary normalisation, HUF_validateCTable, the thresholds) and change no byte of output.
 * seq_bits_*: one sequence's bits in the stream (three state fields, three extra-bit fields) are more than 64, or with
 * their bit offset in a 32-bit word more than 64 / 96: they spread over three / four words.
 * The names are declared here, once: X(name) per counter, index = position in the list. */
#define CRYO_ZSTD_ENC_TRACE(X)                                                                                          \
    X(lit_disabled) X(lit_le63_raw) X(lit_rle) X(lit_flat_raw) X(lit_huf_raw) X(lit_mingain_raw) X(lit_compressed)      \
    X(lit_treeless) X(lit_single_stream) X(lit_four_streams)                                                            \
    X(huf_validate_fail) X(huf_prefer_repeat) X(huf_treeless_by_cost) X(huf_new_table_over_old) X(huf_hsz12_treeless)   \
    X(huf_hsz12_raw) X(huf_undescribable) X(huf_weights_direct) X(huf_weights_fse) X(huf_weights_fse_above_128)          \
    X(huf_streams_too_big)                                                                                              \
    X(huf_clip) X(huf_clip_by_2_or_more) X(huf_clip_overshoot)                                                          \
    X(seq_count_1byte) X(seq_count_2bytes) X(seq_count_3bytes)                                                          \
    X(ll_basic) X(ll_rle) X(ll_compressed) X(ll_repeat) X(of_basic) X(of_rle) X(of_compressed) X(of_repeat)             \
    X(ml_basic) X(ml_rle) X(ml_compressed) X(ml_repeat)                                                                 \
    X(sel_one_code_basic) X(sel_one_code_rle) X(sel_below_dyn_min) X(sel_below_most) X(sel_threshold_compressed)        \
    X(sel_cost_basic) X(sel_cost_repeat) X(sel_cost_compressed) X(sel_default_disallowed)                               \
    X(tab_low_prob) X(tab_no_low_prob) X(tab_norm_m2) X(tab_norm_fail) X(tab_zero_run_3) X(tab_zero_run_24)             \
    X(seq_long_ll) X(seq_long_ml) X(seq_bits_3_dwords) X(seq_bits_over_64) X(seq_bits_4_dwords) X(seq_over_cap)         \
    X(seq_last_ncount_raw) X(block_mingain_raw) X(block_compressed)
int cryo_oracle_zstd_enc_trace_count(void);
const char *cryo_oracle_zstd_enc_trace_name(int i);    /* NULL outside 0 .. count - 1 */
void cryo_oracle_zstd_enc_trace_reset(void);
void cryo_oracle_zstd_enc_trace_from_block(int k);     /* count from a frame's block k on (0, the default: every block) */
void cryo_oracle_zstd_enc_trace_get(uint64_t *out);    /* count values */

#ifdef __cplusplus
}
#endif
#endif
