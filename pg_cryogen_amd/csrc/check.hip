/*
 * check.hip -- the device side of the stored-block check (cryo_codec_check_batch, include/cryo_codec.h).
 *
 * The host (cryo_codec.cpp, check_pass) decodes a batch with the automatic decode routes into handle workspace, the shared
 * decode loop of write verification (decode_pass); on every decoded chunk these kernels apply the layout rules of
 * cryo_init_page / cryo_storage_insert (host/storage.c) to each block:
 *   k_check_items  one wave per block, one lane per item (up to five items per lane): the header rule (heap_block.h), the chain rule of
 *                  every item against its stored predecessor (the predecessor's offset comes from the neighbouring lane,
 *                  so each item is read once), the lowest failing item by ballot; when both pass, each tuple's pad is
 *                  checked in the one 8-byte word that holds the tuple's last byte.  It writes the block's verdict, the
 *                  gap [lower, upper) for the next kernel, and the block's lowest nonzero pad byte
 *   k_check_zero   one workgroup per 16 KiB piece of a block, cut to the gap: 16 bytes per lane with four loads in flight
 *                  (8-byte halves at the gap's edges, which are multiples of 8 once the header and items passed); the
 *                  wave's lowest nonzero byte by ballot, folded into the block's word with a vector atomicMin
 *   k_check_fold   one lane per block: {reason, offset} from the decoder's status, the verdict and the nonzero word
 * Only the item array, the gap and the pad words are read.  Tuple bodies are never checked: a pad word also holds up to 7
 * bytes of its tuple's tail, which are loaded with it and ignored; no other tuple byte is loaded.  Every device write is a
 * vector store or a vector atomic.
 */
#include "kernels.h"

namespace cryo {

constexpr uint32_t kCheckNone = 0xffffffffu;
constexpr uint32_t kCheckOk = 0, kCheckStream = 1, kCheckHeader = 2, kCheckItem = 3, kCheckNonzero = 4; /* cryo_check_reason */
constexpr uint32_t kCheckItemTurns = (kHeapMaxItems + 63u) / 64u;
constexpr uint32_t kCheckLoads = 4;
constexpr uint32_t kCheckPiece = 256u * 16u * kCheckLoads; /* bytes of a block one workgroup of k_check_zero covers */

__global__ void __launch_bounds__(256)
k_check_items(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
              const int32_t *__restrict__ dec_status, uint2 *__restrict__ verdict, uint2 *__restrict__ gap,
              uint32_t *__restrict__ first)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (k >= cnt) return;
    if (dec_status[k] != 0) { /* the decoders rejected the stream: nothing decoded to look at */
        if (lane == 0) { verdict[k] = make_uint2(kCheckStream, kCheckNone); gap[k] = make_uint2(0u, 0u); first[k] = kCheckNone; }
        return;
    }
    const uint8_t *p = dec + (uint64_t)k * dec_stride;
    const uint2 hdr = *reinterpret_cast<const uint2 *>(p);
    const uint32_t lower = hdr.x;
    uint32_t n, upper;
    if (!heap_header(hdr, B, n, upper)) {
        if (lane == 0) { verdict[k] = make_uint2(kCheckHeader, 0u); gap[k] = make_uint2(0u, 0u); first[k] = kCheckNone; }
        return;
    }
    /* item i = t * 64 + lane; every load first, then the checks */
    uint2 it[kCheckItemTurns];
#pragma unroll
    for (uint32_t t = 0; t < kCheckItemTurns; t++) {
        const uint32_t i = t * 64u + lane;
        it[t] = i < n ? *reinterpret_cast<const uint2 *>(p + 8u + 8u * i) : make_uint2(0u, 0u);
    }
    uint32_t carry = B; /* offset stored in item t * 64 - 1: lane 63's of the turn before (B before item 0) */
    int32_t bad_item = -1;
    bool bad_any = false;
#pragma unroll
    for (uint32_t t = 0; t < kCheckItemTurns; t++) {
        const uint32_t i = t * 64u + lane;
        const uint32_t up = __shfl(it[t].x, (int)((lane + 63u) & 63u));
        const uint64_t prev = lane == 0 ? carry : up;
        carry = __shfl(it[t].x, 63);
        const uint64_t off = it[t].x, len = it[t].y;
        const bool bad = i < n && (len == 0 || off + ((len + 7u) & ~(uint64_t)7u) != prev || (i == n - 1u && off != upper));
        const unsigned long long m = __ballot(bad);
        if (m && !bad_any) { bad_any = true; bad_item = (int32_t)(t * 64u + (uint32_t)__builtin_ctzll(m)); }
    }
    if (bad_any) {
        if (lane == 0) {
            verdict[k] = make_uint2(kCheckItem, 8u + 8u * (uint32_t)bad_item);
            gap[k] = make_uint2(0u, 0u);
            first[k] = kCheckNone;
        }
        return;
    }
    /* the chain is whole: tuple i occupies [off_i, off_i + MAXALIGN(len_i)), every offset a multiple of 8, item i + 1 below
     * item i.  Its pad is the top (8 - len_i % 8) % 8 bytes of the word that ends its slot. */
    uint32_t pad_at[kCheckItemTurns];
#pragma unroll
    for (uint32_t t = 0; t < kCheckItemTurns; t++) {
        const uint32_t i = t * 64u + lane;
        pad_at[t] = kCheckNone;
        const uint32_t r = it[t].y & 7u;
        if (i < n && r != 0u) {
            const uint32_t w = it[t].x + ((it[t].y + 7u) & ~7u) - 8u;
            const uint2 v = *reinterpret_cast<const uint2 *>(p + w);
            const uint64_t q = ((uint64_t)v.y << 32 | v.x) >> (8u * r);
            if (q) pad_at[t] = w + r + ((uint32_t)__builtin_ctzll(q) >> 3);
        }
    }
    /* the lowest bad pad byte is in the highest item that has one */
    uint32_t lowest = kCheckNone;
#pragma unroll
    for (int t = (int)kCheckItemTurns - 1; t >= 0; t--) {
        const unsigned long long m = __ballot(pad_at[t] != kCheckNone);
        if (m) {
            lowest = __shfl(pad_at[t], 63 - __builtin_clzll(m));
            break;
        }
    }
    if (lane == 0) { verdict[k] = make_uint2(kCheckOk, kCheckNone); gap[k] = make_uint2(lower, upper); first[k] = lowest; }
}

/* first nonzero byte of a 16-byte piece (16: none) */
__device__ inline uint32_t first_nonzero16(const uint4 &a)
{
    const uint32_t d[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int w = 0; w < 4; w++)
        if (d[w]) return (uint32_t)w * 4u + ((uint32_t)__builtin_ctz(d[w]) >> 3);
    return 16u;
}

__global__ void __launch_bounds__(256)
k_check_zero(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t pieces, const uint2 *__restrict__ gap,
             uint32_t *__restrict__ first)
{
    const uint32_t k = blockIdx.x / pieces, pc = blockIdx.x - k * pieces;
    const uint2 g = gap[k];
    const uint32_t p0 = pc * kCheckPiece;
    const uint64_t p1 = (uint64_t)p0 + kCheckPiece;
    const uint32_t lo = g.x > p0 ? g.x : p0;
    const uint32_t hi = (uint64_t)g.y < p1 ? g.y : (uint32_t)p1;
    if (lo >= hi) return; /* no gap in this piece, or the block already failed (empty gap) */
    const uint8_t *p = dec + (uint64_t)k * dec_stride;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t base = p0 + threadIdx.x * 16u;
    uint32_t at[kCheckLoads];
    if (lo == p0 && (uint64_t)hi == p1) {
        uint4 x[kCheckLoads];
#pragma unroll
        for (uint32_t j = 0; j < kCheckLoads; j++) x[j] = *reinterpret_cast<const uint4 *>(p + base + j * 4096u);
#pragma unroll
        for (uint32_t j = 0; j < kCheckLoads; j++) at[j] = first_nonzero16(x[j]);
    } else {
        /* the gap's edges are multiples of 8: a 16-byte piece is in, out, or in by one 8-byte half */
        uint4 x[kCheckLoads];
#pragma unroll
        for (uint32_t j = 0; j < kCheckLoads; j++) {
            const uint32_t o = base + j * 4096u;
            x[j] = make_uint4(0u, 0u, 0u, 0u);
            if (o >= lo && o + 16u <= hi) {
                x[j] = *reinterpret_cast<const uint4 *>(p + o);
            } else if (o >= lo && o + 8u <= hi) { /* the lower half */
                const uint2 h = *reinterpret_cast<const uint2 *>(p + o);
                x[j].x = h.x; x[j].y = h.y;
            } else if (o + 8u >= lo && o + 16u <= hi) { /* the upper half */
                const uint2 h = *reinterpret_cast<const uint2 *>(p + o + 8u);
                x[j].z = h.x; x[j].w = h.y;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kCheckLoads; j++) at[j] = first_nonzero16(x[j]);
    }
    /* load j of a wave covers 1 KiB before load j + 1's, lanes in order inside it (as k_verify) */
#pragma unroll
    for (uint32_t j = 0; j < kCheckLoads; j++) {
        const unsigned long long m = __ballot(at[j] < 16u);
        if (m) {
            if (lane == (uint32_t)__builtin_ctzll(m)) atomicMin(first + k, base + j * 4096u + at[j]);
            return;
        }
    }
}

__global__ void __launch_bounds__(256)
k_check_fold(uint32_t cnt, const uint2 *__restrict__ verdict, const uint32_t *__restrict__ first, uint2 *__restrict__ result)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint2 v = verdict[k];
    const uint32_t f = first[k];
    result[k] = v.x == kCheckOk && f != kCheckNone ? make_uint2(kCheckNonzero, f) : v;
}

hipError_t launch_check(hipStream_t s, const uint8_t *d_dec, uint64_t dec_stride, uint32_t block_size, uint32_t cnt,
                        const int32_t *d_dec_status, uint2 *d_verdict, uint2 *d_gap, uint32_t *d_first, uint2 *d_result)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_check_items, dim3((cnt + 3u) / 4u), dim3(256), 0, s, d_dec, dec_stride, block_size, cnt, d_dec_status,
                       d_verdict, d_gap, d_first);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const uint32_t pieces = (block_size + kCheckPiece - 1u) / kCheckPiece;
    const uint64_t grid = (uint64_t)cnt * pieces;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_check_zero, dim3((uint32_t)grid), dim3(256), 0, s, d_dec, dec_stride, pieces, d_gap, d_first);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_check_fold, dim3((cnt + 255u) / 256u), dim3(256), 0, s, cnt, d_verdict, d_first, d_result);
    return hipGetLastError();
}

} // namespace cryo
