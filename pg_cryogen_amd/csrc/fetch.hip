/*
 * fetch.hip -- the device side of the tuple fetch (cryo_codec_fetch_batch / _blocks, include/cryo_codec.h).
 *
 * The host (cryo_codec.cpp, fetch_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); these kernels gather the tuples a caller asked for, by item position, out of the decoded chunk and pack them,
 * so that only tuples leave the device:
 *   k_fetch_items    one wave per block, four blocks per workgroup.  A block the decoders rejected gets STREAM without a
 *                    load.  Otherwise the wave reads lower / upper, applies the header rule (heap_header), and takes its requests 64 per
 *                    turn: a lane loads its position, compares it with its left neighbour's (lane 0 with the last of the turn
 *                    before: strictly ascending from 0, which also rejects position 0), loads its 8-byte item and applies
 *                    NOITEM / ITEM (heap_item).  A wave scan of MAXALIGN(len) places every request inside the block's output.  BADREQ and
 *                    OVERLAP are verdicts on the whole block that are known only after the last turn, so the records are
 *                    written in a second sweep over the requests (positions and items come from L2 then).  It writes one
 *                    16-byte record per request with the offset INSIDE the block's output, the same offset and the tuple's
 *                    place in the decoded block into a side table (8 bytes per request, workspace), and the block's sum.
 *   k_fetch_offsets  one workgroup per chunk: an exclusive scan over the blocks' sums in tiles of 256 (offsets_tile), starting
 *                    from the running total the chunk before left in device memory; writes every block's base, the chunk's
 *                    end, and the new running total.  (Two levels on purpose: a chunk can hold millions of requests but only K blocks.)
 *   k_fetch_copy     walks the PACKED side as k_recode_pack does: a fixed grid strides over the 2 KiB pieces of [base[0],
 *                    base[cnt]); a piece finds the block of its first byte by binary search in the bases (find_last_le), then the request
 *                    by binary search in the block's side table; a lane whose bytes belong to a later block searches on
 *                    from there.  Offsets never decrease and a failed request shares its offset with the next tuple, so "the
 *                    last entry at or below the byte" is always the OK request that owns it.  8 bytes per lane (tuples start
 *                    at multiples of 8 on both sides); the pad [len, MAXALIGN(len)) is masked to zero in registers (mask_tuple_tail).  The
 *                    same grid then strides over the blocks and writes base + offset into the records' `off` (an 8-byte store
 *                    to a field the copy never reads: the copy reads {status, len} and the side table only).
 * A request-side mapping of the copy (a quarter wave per tuple) was considered: it idles on the one-byte tuples and
 * serialises on the tuple that fills a block, both of which the packed side balances; it has not been measured.
 * The block rules, the scan's tile, the search and the mask are heap_block.h's, shared with the other scan kernels.
 * Every device write is a vector store.  No LDS beyond the scan's four words, no scratch.
 */
#include "kernels.h"

namespace cryo {

constexpr uint32_t kFetchOk = 0, kFetchStream = 1, kFetchHeader = 2, kFetchItem = 3, kFetchNoItem = 5, kFetchBadReq = 6,
                   kFetchOverlap = 7;              /* cryo_fetch_status */
constexpr uint32_t kFetchPiece = 256u * 8u;        /* packed bytes one workgroup copies per turn */

__device__ inline void fetch_put(uint4 *__restrict__ result, uint2 *__restrict__ side, uint64_t r, uint32_t status, uint32_t len,
                                 uint32_t at, uint32_t src)
{
    result[r] = make_uint4(status, len, at, 0u);
    side[r] = make_uint2(at, src);
}

/* every request of the block gets `status`, no length and no room */
__device__ inline void fetch_fill(uint4 *__restrict__ result, uint2 *__restrict__ side, uint64_t r0, uint64_t nreq, uint32_t lane,
                                  uint32_t status)
{
    for (uint64_t i = lane; i < nreq; i += 64u) fetch_put(result, side, r0 + i, status, 0u, 0u, 0u);
}

/* One sweep over a block's requests.  WRITE = false: returns the sum of MAXALIGN(len) over the requests that pass NOITEM and
 * ITEM, and whether the positions break the ascending rule.  WRITE = true: writes the records; `overlap` turns every OK request
 * into OVERLAP and gives no request any room. */
template <bool WRITE>
__device__ inline uint64_t fetch_sweep(const uint8_t *__restrict__ p, uint32_t B, uint32_t n, uint32_t upper,
                                       const uint16_t *__restrict__ pos, uint64_t r0, uint64_t nreq, uint32_t lane, bool &badreq,
                                       bool overlap, uint4 *__restrict__ result, uint2 *__restrict__ side)
{
    uint64_t run = 0;
    uint32_t carry = 0; /* the position before this turn's first: 0 before the first request, so that position 0 fails too */
    bool bad = false;
    for (uint64_t t = 0; t < nreq; t += 64u) {
        const uint64_t i = t + lane;
        const bool valid = i < nreq;
        const uint32_t q = valid ? (uint32_t)pos[r0 + i] : 0u;
        const uint32_t up = __shfl_up(q, 1);
        const uint32_t prev = lane == 0 ? carry : up;
        carry = __shfl(q, 63);
        if (__ballot(valid && q <= prev)) bad = true;
        uint32_t status = kFetchOk, len = 0, src = 0;
        if (valid) {
            if (q == 0u || q > n) status = kFetchNoItem; /* q == 0 is BADREQ for the whole block; no item is loaded for it */
            else {
                const uint2 it = *reinterpret_cast<const uint2 *>(p + 8u + 8u * (q - 1u));
                if (!heap_item(it, upper, B, src, len)) status = kFetchItem;
            }
        }
        const uint64_t a = valid && status == kFetchOk ? ((uint64_t)len + 7u) & ~(uint64_t)7u : 0u;
        uint64_t inc = a;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t v = __shfl_up((unsigned long long)inc, d);
            if (lane >= d) inc += v;
        }
        if (WRITE && valid) {
            if (overlap) fetch_put(result, side, r0 + i, status == kFetchOk ? kFetchOverlap : status, 0u, 0u, 0u);
            else fetch_put(result, side, r0 + i, status, len, (uint32_t)(run + inc - a), src);
        }
        run += __shfl((unsigned long long)inc, 63);
    }
    badreq = bad;
    return run;
}

__global__ void __launch_bounds__(256)
k_fetch_items(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
              const int32_t *__restrict__ dec_status, const uint64_t *__restrict__ req_first, const uint16_t *__restrict__ pos,
              uint64_t n_req, uint4 *__restrict__ result, uint2 *__restrict__ side, uint64_t *__restrict__ sum)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (k >= cnt) return;
    /* the request table is the caller's: whatever it holds, no request beyond n_req is touched */
    uint64_t r1 = req_first[k + 1u], r0 = req_first[k];
    if (r1 > n_req) r1 = n_req;
    if (r0 > r1) r0 = r1;
    const uint64_t nreq = r1 - r0;
    uint64_t total = 0;
    if (dec_status[k] != 0) { /* the decoders rejected the stream: nothing decoded to look at */
        fetch_fill(result, side, r0, nreq, lane, kFetchStream);
    } else {
        const uint8_t *p = dec + (uint64_t)k * dec_stride;
        const uint2 hdr = *reinterpret_cast<const uint2 *>(p);
        uint32_t n, upper;
        if (!heap_header(hdr, B, n, upper)) {
            fetch_fill(result, side, r0, nreq, lane, kFetchHeader);
        } else {
            bool badreq = false, unused = false;
            const uint64_t s = fetch_sweep<false>(p, B, n, upper, pos, r0, nreq, lane, badreq, false, nullptr, nullptr);
            if (badreq) {
                fetch_fill(result, side, r0, nreq, lane, kFetchBadReq);
            } else {
                const bool overlap = s > (uint64_t)(B - upper);
                (void)fetch_sweep<true>(p, B, n, upper, pos, r0, nreq, lane, unused, overlap, result, side);
                if (!overlap) total = s;
            }
        }
    }
    if (lane == 0) sum[k] = total;
}

__global__ void __launch_bounds__(256)
k_fetch_offsets(uint32_t cnt, const uint64_t *__restrict__ sum, uint64_t *__restrict__ base, uint64_t *__restrict__ running)
{
    __shared__ uint64_t wave_sum[4];
    uint64_t run = *running; /* the same in every thread; written again only after the tiles' barriers */
    for (uint32_t t = 0; t < cnt; t += 256u) {
        const uint32_t k = t + threadIdx.x;
        const uint64_t a[1] = {k < cnt ? sum[k] : 0u};
        uint64_t before[1], tile[1];
        offsets_tile(a, wave_sum, before, tile);
        if (k < cnt) base[k] = run + before[0];
        run += tile[0];
    }
    if (threadIdx.x == 0) {
        base[cnt] = run;
        *running = run;
    }
}

/* the last r in [lo, hi] with side[r].x <= x; side[lo].x <= x is the caller's */
__device__ inline uint64_t fetch_find_req(const uint2 *__restrict__ side, uint64_t lo, uint64_t hi, uint32_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo + 1u) >> 1);
        if (side[mid].x <= x) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

/* dst_bias: the packed offset that d_dst's first byte stands for (0: the caller's buffer holds the whole call; a chunk's own
 * staging area starts at the chunk's first base, read from base[0] when chunk_relative is set).  A tuple that would end beyond
 * dst_cap bytes of d_dst is not written. */
__global__ void __launch_bounds__(256)
k_fetch_copy(uint32_t cnt, const uint8_t *__restrict__ dec, uint64_t dec_stride, const uint64_t *__restrict__ req_first,
             uint64_t n_req, const uint64_t *__restrict__ base, const uint2 *__restrict__ side, uint4 *__restrict__ result,
             uint8_t *__restrict__ dst, uint64_t dst_cap, uint32_t chunk_relative)
{
    const uint64_t begin = base[0], end = base[cnt];
    const uint64_t bias = chunk_relative ? begin : 0u;
    for (uint64_t p0 = begin + (uint64_t)blockIdx.x * kFetchPiece; p0 < end; p0 += (uint64_t)gridDim.x * kFetchPiece) {
        const uint64_t x = p0 + threadIdx.x * 8u;
        if (x >= end) continue;
        /* base[cnt] = end > p0: the block of the piece's first byte lies in [0, cnt - 1]; a block without room is never found
         * (its successor starts at the same base) */
        const uint32_t k0 = find_last_le(base, 0u, cnt - 1u, p0);
        const uint32_t k = base[k0 + 1u] > x ? k0 : find_last_le(base, k0 + 1u, cnt - 1u, x);
        const uint32_t xr = (uint32_t)(x - base[k]); /* below the block's sum, which is below the block size */
        uint64_t r1 = req_first[k + 1u], r0 = req_first[k];
        if (r1 > n_req) r1 = n_req;
        if (r0 >= r1) continue; /* a block with room has requests */
        const uint64_t r = fetch_find_req(side, r0, r1 - 1u, xr);
        const uint2 sd = side[r];
        const uint2 rec = *reinterpret_cast<const uint2 *>(result + r); /* {status, len}: never written by this kernel */
        const uint32_t at = xr - sd.x;
        const uint32_t len = rec.y;
        if (rec.x != kFetchOk || at >= len) continue; /* cannot happen for a byte below the block's sum */
        const uint64_t tuple_end = base[k] + sd.x + (((uint64_t)len + 7u) & ~(uint64_t)7u) - bias;
        if (tuple_end > dst_cap) continue;
        const uint2 v = *reinterpret_cast<const uint2 *>(dec + (uint64_t)k * dec_stride + sd.y + at);
        const uint32_t keep = len - at; /* bytes of the tuple from here on */
        *reinterpret_cast<uint2 *>(dst + (x - bias)) = mask_tuple_tail(v, keep); /* the tuple's last word: its pad zero */
    }
    /* the records' offsets: inside the block so far, within the call from here on */
    for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
        uint64_t r1 = req_first[k + 1u], r0 = req_first[k];
        if (r1 > n_req) r1 = n_req;
        const uint64_t b = base[k];
        for (uint64_t r = r0 + threadIdx.x; r < r1; r += 256u)
            *reinterpret_cast<uint64_t *>(reinterpret_cast<uint8_t *>(result + r) + 8u) = b + side[r].x;
    }
}

hipError_t launch_fetch(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                        const int32_t *d_dec_status, const uint64_t *d_req_first, const uint16_t *d_pos, uint64_t n_req,
                        uint4 *d_result, uint2 *d_side, uint64_t *d_sum, uint64_t *d_base, uint64_t *d_running, uint8_t *d_dst,
                        uint64_t dst_cap, bool chunk_relative, int cus)
{
    if (cnt == 0) return hipSuccess;
    if ((dec_stride & 15u) != 0 || (((uintptr_t)d_dec | (uintptr_t)d_result) & 15u) != 0 || ((uintptr_t)d_dst & 7u) != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fetch_items, dim3((cnt + 3u) / 4u), dim3(256), 0, s, d_dec, dec_stride, block_size, cnt, d_dec_status,
                       d_req_first, d_pos, n_req, d_result, d_side, d_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fetch_offsets, dim3(1), dim3(256), 0, s, cnt, d_sum, d_base, d_running);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    /* four workgroups per compute unit, but never more than the chunk's worst case has pieces (or blocks, for the records) */
    const uint64_t worst = ((uint64_t)cnt * block_size + kFetchPiece - 1u) / kFetchPiece;
    uint64_t grid = (uint64_t)(cus > 0 ? cus : 256) * 4u;
    if (grid > worst) grid = worst;
    if (grid < 1u) grid = 1u;
    hipLaunchKernelGGL(k_fetch_copy, dim3((uint32_t)grid), dim3(256), 0, s, cnt, d_dec, dec_stride, d_req_first, n_req, d_base,
                       d_side, d_result, d_dst, dst_cap, chunk_relative ? 1u : 0u);
    return hipGetLastError();
}

} // namespace cryo
