/*
 * host_stage.h -- the two rules the host-buffer codec calls share: where the streams of a call (or of a subset of one) lie in
 * the staging area that goes to the device, and how a large call is cut into the chunks of the pipelined staging.  Plain integer
 * code: no HIP, nothing of cryo_codec, so a host-only program can include it (tests/host_stage_check.cpp does).
 */
#ifndef CRYO_HOST_STAGE_H
#define CRYO_HOST_STAGE_H

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cryo {

/* ---- the chunk cut: a call of n blocks goes through the pipeline in chunks of K -- an eighth of the call, at least 8 MiB + 1
 * block, rounded up to 64 blocks ---- */
struct ChunkCut {
    size_t n, K;
    ChunkCut(size_t n_, size_t block_size) : n(n_), K((std::max((n_ + 7) / 8, ((size_t)8 << 20) / block_size + 1) + 63) & ~(size_t)63) {}
    size_t chunks() const { return (n + K - 1) / K; }
    size_t lo(size_t ch) const { return ch * K; }
    size_t hi(size_t ch) const { return lo(ch) + K < n ? lo(ch) + K : n; }
    size_t cnt(size_t ch) const { return hi(ch) - lo(ch); }
};
/* one block is one wavefront's serial job: a launch needs thousands of blocks to fill the chip, so kernels run per chunk only
 * when a chunk still has that many (LZ4 decode of 128 KiB blocks); otherwise the transfers are chunked around ONE launch over the
 * whole call (the encoders took 8 x longer cut in eight) */
inline bool kernel_per_chunk(size_t chunk_blocks, bool lz4, bool encode) { return !encode && lz4 && chunk_blocks >= 512; }

/* ---- the staged streams: [offsets u64 x m][sizes u32 x m][streams, each padded to 16], the streams from o_data on.  size_of(k)
 * is the size of stream k of the m -- of a whole call, or of the subset its caller indexes ---- */
struct StreamLayout {
    size_t m, o_off = 0, o_sz, o_data, total; /* total: the padded streams together */
    std::vector<uint64_t> pos;                /* pos[k]: where stream k begins behind o_data; pos[m] = total */
    template <class SizeOf> StreamLayout(size_t m_, SizeOf size_of) : m(m_), o_sz(m_ * 8), o_data((m_ * 12 + 63) & ~(size_t)63), pos(m_ + 1)
    {
        for (size_t k = 0; k < m; k++) pos[k + 1] = pos[k] + (((uint64_t)size_of(k) + 15) & ~(uint64_t)15);
        total = (size_t)pos[m];
    }
    /* tables and streams together: what one copy of the whole sends */
    size_t bytes() const { return o_data + total; }
    /* where stream k begins in the whole: what its table entry says */
    uint64_t offset(size_t k) const { return o_data + pos[k]; }
    /* the padded streams of entries lo .. hi-1 */
    size_t span(size_t lo, size_t hi) const { return (size_t)(pos[hi] - pos[lo]); }
    /* the most any chunk of the cut brings in */
    size_t max_chunk_in(const ChunkCut &cut) const
    {
        size_t most = 0;
        for (size_t ch = 0; ch < cut.chunks(); ch++)
            if (span(cut.lo(ch), cut.hi(ch)) > most) most = span(cut.lo(ch), cut.hi(ch));
        return most;
    }
    /* the two tables of the whole that begins at `base` (8-byte aligned) */
    template <class SizeOf> void fill_tables(uint8_t *base, SizeOf size_of) const
    {
        for (size_t k = 0; k < m; k++) {
            ((uint64_t *)(base + o_off))[k] = offset(k);
            ((uint32_t *)(base + o_sz))[k] = size_of(k);
        }
    }
};

} // namespace cryo

#endif
