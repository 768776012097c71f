/*
 * filter.hip -- the device side of the scan filter (cryo_codec_filter_batch / _blocks, include/cryo_codec.h: the rules).
 *
 * The host (cryo_codec.cpp, filter_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); these kernels look into every heap tuple of the decoded chunk, test up to four scan keys on it and pack the
 * tuples that pass, so that only matches leave the device:
 *   k_filter_match    one wave per block, four blocks per workgroup, as k_fetch_items: the sweep of scan_sweep.h, whose walk runs over
 *                     the columns 1 .. the highest key column and captures nothing.  A descriptor with a byte-string key
 *                     (CRYO_KEY_BYTES) runs k_filter_match<true>, every other k_filter_match<false>; a descriptor with a float
 *                     key (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8) runs k_filterf_match, the same body with the walk's FLOATS
 *                     parameter set.
 *                     OVERLAP is a verdict on the block that is known only after the last turn, so -- as in the fetch -- a first
 *                     sweep sums and a second one writes (items and tuples come from L2 then): per record {offset inside the
 *                     block's output, the tuple's place in the decoded block, len, pos | status << 16} into a side table in
 *                     position order, the first half of the block's row of the table, and the block's two sums.
 *   k_filter_offsets  one workgroup per chunk: the tiled scan of heap_block.h (offsets_tile) over two arrays at once (bytes, records),
 *                     from the two running totals the chunk before left in device memory; it also writes {rec_first, off} of every row.
 *   k_filter_copy     walks the PACKED side as k_fetch_copy does (2 KiB pieces, a binary search for the block -- find_last_le --, one
 *                     for the record in the block's side table; bad items share their offset with the next tuple, so "the last entry at
 *                     or below the byte" is the match that owns it), then the same grid strides over the blocks and writes the
 *                     8-byte records to their final places.
 * The fetch's kernels are not reused: k_fetch_offsets scans one array and its copy finds requests through the caller's CSR table,
 * which a filter does not have; what the two have in common -- the block rules, the scan's tile, the block search, the mask of a
 * tuple's last word -- is heap_block.h's.  Every device write is a vector store in plain C++.  No LDS beyond the scan's eight words, no
 * scratch.
 */
#include "kernels.h"
#include "scan_sweep.h"

namespace cryo {

/* One sweep over a block's items.  WRITE = false: the sums {MAXALIGNed bytes of the matches, matches, bad items}.  WRITE = true:
 * the side table's entries in position order; `overlap` drops the matches.  An undecided tuple is a bad item: counted, and listed
 * with its status and no bytes. */
template <bool WRITE, bool BYTES, bool FLOATS = false, bool LIKE = false>
__device__ inline void filter_sweep(const uint8_t *__restrict__ p, uint32_t B, uint32_t n, uint32_t upper, uint32_t lane,
                                    const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                                    uint32_t max_att, bool overlap, uint4 *__restrict__ side, uint64_t &bytes, uint32_t &n_match,
                                    uint32_t &n_bad)
{
    uint64_t run = 0;
    uint32_t recs = 0, matches = 0, bads = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        const uint32_t i = t0 + lane;
        const SweepItem it = sweep_turn<false, kAggMaxCols, BYTES, false, FLOATS, false, LIKE>(p, B, n, upper, i, atts, keys, nkeys, max_att,
                                                                                              nullptr, 0u, nullptr); /* the walk without capture */
        const uint32_t status = it.verdict, len = it.len, src = it.src;
        const bool match = it.match, bad = it.bad;
        const unsigned long long mm = __ballot(match), mb = __ballot(bad);
        if (WRITE) {
            const bool rec = bad || (match && !overlap);
            const unsigned long long mr = overlap ? mb : (mm | mb);
            const uint32_t a = match && !overlap ? (len + 7u) & ~7u : 0u;
            uint32_t inc = a; /* a block's matches sum to at most B - upper here: 32 bits */
#pragma unroll
            for (uint32_t d = 1; d < 64u; d <<= 1) {
                const uint32_t v = __shfl_up(inc, d);
                if (lane >= d) inc += v;
            }
            if (rec) {
                const uint32_t j = recs + (uint32_t)__popcll(mr & ((1ull << lane) - 1ull));
                side[j] = make_uint4((uint32_t)run + inc - a, match ? src : 0u, match ? len : 0u, (i + 1u) | (match ? 0u : status << 16));
            }
            run += __shfl(inc, 63);
            recs += (uint32_t)__popcll(mr);
        } else {
            uint64_t a = match ? ((uint64_t)len + 7u) & ~(uint64_t)7u : 0u;
#pragma unroll
            for (uint32_t d = 32; d >= 1u; d >>= 1) a += __shfl_xor((unsigned long long)a, d);
            run += a;
        }
        matches += (uint32_t)__popcll(mm);
        bads += (uint32_t)__popcll(mb);
    }
    bytes = run;
    n_match = matches;
    n_bad = bads;
}

/* the body of k_filter_match, of k_filterf_match, the kernel of descriptors with a float key, and of k_filterl_match, the kernel
 * of descriptors with a pattern key */
template <bool BYTES, bool FLOATS, bool LIKE = false>
__device__ inline void filter_block_body(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
                                         const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts,
                                         const FilterKey *__restrict__ keys, uint32_t nkeys, uint32_t max_att, uint32_t count_only,
                                         uint32_t side_stride, uint4 *__restrict__ blocks, uint4 *__restrict__ side,
                                         uint64_t *__restrict__ sum)
{
    uint32_t k, lane;
    sweep_wave(4u, k, lane);
    if (k >= cnt) return;
    uint32_t n_match = 0, n_bad = 0;
    uint64_t bytes = 0;
    const uint8_t *__restrict__ p;
    uint32_t n, upper; /* lower <= B: n <= side_stride */
    uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    if (status == 0u) {
        filter_sweep<false, BYTES, FLOATS, LIKE>(p, B, n, upper, lane, atts, keys, nkeys, max_att, false, nullptr, bytes, n_match, n_bad);
        if (!count_only) {
            const bool overlap = bytes > (uint64_t)(B - upper);
            uint64_t b2;
            uint32_t m2, x2;
            filter_sweep<true, BYTES, FLOATS, LIKE>(p, B, n, upper, lane, atts, keys, nkeys, max_att, overlap, side + (uint64_t)k * side_stride, b2,
                                              m2, x2);
            if (overlap) { status = kFilterOverlap; n_match = 0; bytes = 0; }
        }
    }
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n, n_match, n_bad);
        if (count_only) blocks[2u * k + 1u] = make_uint4(0u, 0u, 0u, 0u);
        else {
            sum[k] = bytes;
            sum[cnt + k] = (uint64_t)n_match + n_bad;
        }
    }
}

#ifndef CRYO_LIKE_UNIT
constexpr uint32_t kFilterPiece = 256u * 8u;  /* packed bytes one workgroup copies per turn */

template <bool BYTES>
__global__ void __launch_bounds__(256)
k_filter_match(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
               const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys,
               uint32_t nkeys, uint32_t max_att, uint32_t count_only, uint32_t side_stride, uint4 *__restrict__ blocks,
               uint4 *__restrict__ side, uint64_t *__restrict__ sum)
{
    filter_block_body<BYTES, false>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, max_att, count_only, side_stride, blocks,
                                    side, sum);
}

/* k_filter_match<true> whose walk also maps the columns of float keys: the one verdict path, the truth table's */
__global__ void __launch_bounds__(256)
k_filterf_match(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
                const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys,
                uint32_t nkeys, uint32_t max_att, uint32_t count_only, uint32_t side_stride, uint4 *__restrict__ blocks,
                uint4 *__restrict__ side, uint64_t *__restrict__ sum)
{
    filter_block_body<true, true>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, max_att, count_only, side_stride, blocks,
                                  side, sum);
}

/* base[k], base[cnt + 1 + k]: the bytes / records before block k of the chunk, counted from the call's start; entries cnt of both:
 * the chunk's ends */
__global__ void __launch_bounds__(256)
k_filter_offsets(uint32_t cnt, const uint64_t *__restrict__ sum, uint64_t *__restrict__ base, uint64_t *__restrict__ running,
                 uint4 *__restrict__ blocks)
{
    __shared__ uint64_t wave_sum[8];
    uint64_t run_b = running[0], run_r = running[1]; /* the same in every thread; written again only after the tiles' barriers */
    for (uint32_t t = 0; t < cnt; t += 256u) {
        const uint32_t k = t + threadIdx.x;
        const uint64_t a[2] = {k < cnt ? sum[k] : 0u, k < cnt ? sum[cnt + k] : 0u}; /* bytes, records */
        uint64_t before[2], tile[2];
        offsets_tile(a, wave_sum, before, tile);
        if (k < cnt) {
            const uint64_t off = run_b + before[0], first = run_r + before[1];
            base[k] = off;
            base[cnt + 1u + k] = first;
            blocks[2u * k + 1u] = make_uint4((uint32_t)first, (uint32_t)(first >> 32), (uint32_t)off, (uint32_t)(off >> 32));
        }
        run_b += tile[0];
        run_r += tile[1];
    }
    if (threadIdx.x == 0) {
        base[cnt] = run_b;
        base[2u * cnt + 1u] = run_r;
        running[0] = run_b;
        running[1] = run_r;
    }
}

/* the last j in [lo, hi] with side[j].x <= x; side[lo].x <= x is the caller's */
__device__ inline uint32_t filter_find_rec(const uint4 *__restrict__ side, uint32_t lo, uint32_t hi, uint32_t x)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (side[mid].x <= x) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
k_filter_copy(uint32_t cnt, const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t side_stride,
              const uint64_t *__restrict__ base, const uint4 *__restrict__ side, uint8_t *__restrict__ dst, uint64_t dst_cap,
              uint2 *__restrict__ rec, uint64_t rec_cap, uint32_t chunk_relative)
{
    const uint64_t *base_r = base + cnt + 1u;
    const uint64_t begin = base[0], end = base[cnt];
    const uint64_t bias = chunk_relative ? begin : 0u, bias_r = chunk_relative ? base_r[0] : 0u;
    for (uint64_t p0 = begin + (uint64_t)blockIdx.x * kFilterPiece; p0 < end; p0 += (uint64_t)gridDim.x * kFilterPiece) {
        const uint64_t x = p0 + threadIdx.x * 8u;
        if (x >= end) continue;
        /* base[cnt] = end > p0: the block of the piece's first byte lies in [0, cnt - 1]; a block without room is never found
         * (its successor starts at the same base) */
        const uint32_t k0 = find_last_le(base, 0u, cnt - 1u, p0);
        const uint32_t k = base[k0 + 1u] > x ? k0 : find_last_le(base, k0 + 1u, cnt - 1u, x);
        const uint32_t xr = (uint32_t)(x - base[k]); /* below the block's sum, which is below the block size */
        const uint32_t nrec = (uint32_t)(base_r[k + 1u] - base_r[k]);
        if (nrec == 0u || nrec > side_stride) continue; /* a block with room has records */
        const uint4 *sk = side + (uint64_t)k * side_stride;
        const uint4 e = sk[filter_find_rec(sk, 0u, nrec - 1u, xr)];
        const uint32_t at = xr - e.x, len = e.z;
        if ((e.w >> 16) != 0u || at >= len) continue; /* cannot happen for a byte below the block's sum */
        const uint64_t tuple_end = base[k] + e.x + (((uint64_t)len + 7u) & ~(uint64_t)7u) - bias;
        if (tuple_end > dst_cap) continue;
        const uint2 v = *reinterpret_cast<const uint2 *>(dec + (uint64_t)k * dec_stride + e.y + at);
        const uint32_t keep = len - at; /* bytes of the tuple from here on */
        *reinterpret_cast<uint2 *>(dst + (x - bias)) = mask_tuple_tail(v, keep); /* the tuple's last word: its pad zero */
    }
    /* the records, from the side table to their places within the call */
    for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
        const uint64_t first = base_r[k] - bias_r;
        uint32_t nrec = (uint32_t)(base_r[k + 1u] - base_r[k]);
        if (nrec > side_stride) nrec = side_stride;
        const uint4 *sk = side + (uint64_t)k * side_stride;
        for (uint32_t j = threadIdx.x; j < nrec; j += 256u) {
            if (first + j >= rec_cap) break;
            const uint4 e = sk[j];
            rec[first + j] = make_uint2(e.w, e.z); /* {u16 pos, u16 status}, len */
        }
    }
}

hipError_t launch_filter(const ScanChunk &c, const ScanDesc &d, const FilterLaunch &f)
{
    if (c.cnt == 0) return hipSuccess;
    if (!filter_launch_ok(c, d, f)) return hipErrorInvalidValue;
    /* the integer-only descriptor keeps its own instantiation: the code it had before byte-string keys; a float key has a kernel
     * of its own, and a pattern key one in a unit of its own (below) */
    hipError_t e = hipErrorInvalidValue;
    switch (scan_route(d.truth, d.floats, d.like)) {
    case kRouteLike: e = launch_filterl_match(c, d, f); break;
    case kRouteFloat: e = filter_launch(k_filterf_match, true, c, d, f); break;
    case kRouteTable: e = filter_launch(k_filter_match<true>, true, c, d, f); break;
    case kRoutePlain: e = filter_launch(k_filter_match<false>, false, c, d, f); break;
    }
    if (e != hipSuccess || f.count_only) return e;
    hipLaunchKernelGGL(k_filter_offsets, dim3(1), dim3(256), 0, c.stream, c.cnt, f.d_sum, f.d_base, f.d_running, f.d_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    /* never more workgroups than the chunk's worst case has pieces (or blocks, for the records) */
    const uint64_t worst = ((uint64_t)c.cnt * c.block_size + kFilterPiece - 1u) / kFilterPiece;
    hipLaunchKernelGGL(k_filter_copy, dim3(scan_copy_grid(c.cus, worst)), dim3(256), 0, c.stream, c.cnt, c.d_dec, c.dec_stride,
                       filter_side_stride(c.block_size), f.d_base, f.d_side, f.d_dst, f.dst_cap, f.d_rec, f.rec_cap, f.chunk_relative ? 1u : 0u);
    return hipGetLastError();
}

#else /* CRYO_LIKE_UNIT */
/* k_filterf_match whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like): a kernel of its own
 * name, because the matcher inlined costs the walk registers -- k_filter_match<true> and k_filterf_match would fall from eight
 * waves per SIMD to seven -- and a descriptor without such a key must run what it ran.  It is built from this source compiled
 * a second time with CRYO_LIKE_UNIT (filter_like.o, the Makefile's rule), which holds this kernel and its launcher alone */
__global__ void __launch_bounds__(256)
k_filterl_match(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
                const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys,
                uint32_t nkeys, uint32_t max_att, uint32_t count_only, uint32_t side_stride, uint4 *__restrict__ blocks,
                uint4 *__restrict__ side, uint64_t *__restrict__ sum)
{
    filter_block_body<true, true, true>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, max_att, count_only, side_stride, blocks,
                                        side, sum);
}

hipError_t launch_filterl_match(const ScanChunk &c, const ScanDesc &d, const FilterLaunch &f)
{
    return filter_launch(k_filterl_match, true, c, d, f);
}
#endif

} // namespace cryo
