/*
 * heap_block.h -- the decoded heap block as the scan kernels see it (check.hip, fetch.hip, filter.hip, agg.hip, group.hip, project.hip): the
 * rules of the stored-block format (cryo_init_page / cryo_storage_insert, host/storage.c; include/cryo_codec.h: HEADER, ITEM)
 * and the small pieces the kernels that place and copy tuples share.  One copy of each, so that a rule is fixed in one place:
 *   kHeapMaxItems        the items a block can hold
 *   heap_header          the HEADER rule: {lower, upper} and B in, n and upper out, or "bad"
 *   heap_item            the ITEM rule: the item id, upper and B in, the tuple's place and length out, or "bad"
 *   offsets_tile         one 256-thread tile of an exclusive scan of uint64_t: the k_*_offsets kernels run it per tile and
 *                        carry the running total themselves
 *   offsets_of_rows      the whole scan of the two kernels whose blocks bring one count each, in their `blocks` rows
 *   find_last_le         the last index of an ascending uint64_t array with v[i] <= x (the block of a packed byte)
 *   mask_tuple_tail      zeroes the pad in the 8-byte word that holds a tuple's last byte
 * Everything is plain C++; the functions take their inputs by value, so a wave-uniform header stays in scalar registers in
 * the kernels that derive the block from readfirstlane (k_filter_match, k_agg_block, k_group_block, k_project_block).
 */
#ifndef CRYO_HEAP_BLOCK_H
#define CRYO_HEAP_BLOCK_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cryo {

constexpr uint32_t kHeapMaxItems = 290u; /* MaxHeapTuplesPerPage - 1 (host/storage.c) */

/* hdr = {lower, upper}, the block's first 8 bytes.  True: n item ids lie in [8, lower) and the tuples in [upper, B) */
__device__ inline bool heap_header(uint2 hdr, uint32_t B, uint32_t &n, uint32_t &upper)
{
    const uint32_t lower = hdr.x;
    upper = hdr.y;
    n = (lower - 8u) >> 3;
    return !(lower < 8u || (lower & 7u) != 0u || n > kHeapMaxItems || lower > upper || upper > B || (n == 0u && upper != B));
}

/* it = {offset, length}, an item id of a block whose header passed.  True: the tuple lies at [src, src + MAXALIGN(len)) within
 * [upper, B); false: src and len are left as they were */
__device__ inline bool heap_item(uint2 it, uint32_t upper, uint32_t B, uint32_t &src, uint32_t &len)
{
    const uint64_t off = it.x, ln = it.y;
    if (ln == 0 || (off & 7u) != 0 || off < upper || off + ((ln + 7u) & ~(uint64_t)7u) > B) return false;
    src = it.x;
    len = it.y;
    return true;
}

/* One tile of the offset scan over N arrays at once, called by all 256 threads of the workgroup: thread i brings a[j]_i and
 * gets before[j], the sum of a[j] over the threads below i, and tile[j], the sum over all 256.  An inclusive wave scan by
 * __shfl_up, then the four waves' sums through wave_sum[4 * N] (LDS, the caller's: 32 bytes per array); the closing barrier
 * lets the caller write wave_sum again in its next tile. */
template <uint32_t N>
__device__ inline void offsets_tile(const uint64_t (&a)[N], uint64_t *wave_sum, uint64_t (&before)[N], uint64_t (&tile)[N])
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc[N];
#pragma unroll
    for (uint32_t j = 0; j < N; j++) inc[j] = a[j];
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
#pragma unroll
        for (uint32_t j = 0; j < N; j++) {
            const uint64_t up = __shfl_up((unsigned long long)inc[j], d);
            if (lane >= d) inc[j] += up;
        }
    }
    if (lane == 63u) {
#pragma unroll
        for (uint32_t j = 0; j < N; j++) wave_sum[4u * j + wave] = inc[j];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < N; j++) {
        before[j] = inc[j] - a[j];
        tile[j] = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            const uint64_t s = wave_sum[4u * j + w];
            if (w < wave) before[j] += s;
            tile[j] += s;
        }
    }
    __syncthreads();
}

/* The offset scan of a chunk whose blocks bring one count each (k_group_offsets, k_topn_offsets), called by the one workgroup of
 * 256 threads: block k's count is x of its second row in `blocks`; the row becomes {count, 0, first} with first, in 64 bits, the
 * counts before block k from the call's start.  *running: the total before the chunk in, after it out.  wave_sum: four words of
 * LDS, the kernel's */
__device__ inline void offsets_of_rows(uint32_t cnt, uint64_t *__restrict__ running, uint4 *__restrict__ blocks, uint64_t *wave_sum)
{
    uint64_t run = running[0]; /* the same in every thread; written again only after the tiles' barriers */
    for (uint32_t t = 0; t < cnt; t += 256u) {
        const uint32_t k = t + threadIdx.x;
        const uint64_t a[1] = {k < cnt ? blocks[2u * k + 1u].x : 0u};
        uint64_t before[1], tile[1];
        offsets_tile(a, wave_sum, before, tile);
        if (k < cnt) {
            const uint64_t first = run + before[0];
            blocks[2u * k + 1u] = make_uint4((uint32_t)a[0], 0u, (uint32_t)first, (uint32_t)(first >> 32));
        }
        run += tile[0];
    }
    if (threadIdx.x == 0) running[0] = run;
}

/* the last k in [lo, hi] with v[k] <= x; v[lo] <= x is the caller's */
__device__ inline uint32_t find_last_le(const uint64_t *__restrict__ v, uint32_t lo, uint32_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (v[mid] <= x) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

/* v: 8 bytes of a tuple of which `keep` bytes are left from v's first on.  In the tuple's last word (keep < 8) the pad
 * [len, MAXALIGN(len)) becomes zero whatever the block holds there */
__device__ inline uint2 mask_tuple_tail(uint2 v, uint32_t keep)
{
    if (keep < 8u) {
        if (keep <= 4u) { v.y = 0u; if (keep < 4u) v.x &= (1u << (8u * keep)) - 1u; }
        else v.y &= (1u << (8u * (keep - 4u))) - 1u;
    }
    return v;
}

} // namespace cryo

#endif
