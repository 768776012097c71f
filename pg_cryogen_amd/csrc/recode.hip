/*
 * recode.hip -- the device side of recompression (cryo_codec_recode_batch / _blocks, include/cryo_codec.h).
 *
 * The host (cryo_codec.cpp, recode_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass) and encodes the decoded blocks with cryo_codec_compress_batch into slots of a fixed stride, as every compress
 * call does.  These kernels turn the chunk's slots into what travels back:
 *   k_recode_offsets  one workgroup per chunk: folds the decoder's and the encoder's status of every block into its final
 *                     status and size (size 0 unless both are CRYO_OK; a size that does not fit its slot is an error, so that
 *                     the pack below never leaves a slot), and places the streams: off[k] = base + the sum of
 *                     align16(size[j]) for j < k, off[cnt] = base + the chunk's packed total, also written to *total
 *   k_recode_pack     walks the PACKED side: a fixed grid strides over the 4 KiB pieces of [base, base + total), total read
 *                     from device memory (no host round trip between the encode and the pack); a piece finds the block of its
 *                     first byte by binary search in off[] (sorted), a lane whose 16 bytes lie in a later block -- small
 *                     streams, or a 100:1 pair of neighbours -- searches on from there.  16-byte loads and stores (slots and
 *                     offsets are 16-byte aligned); the bytes from size[k] to align16(size[k]) are written as zero, and no
 *                     slot is read beyond align16(size[k])
 * Every device write is a vector store.
 */
#include "kernels.h"

namespace cryo {

constexpr int32_t kRecodeStCorrupt = -4; /* CRYO_E_CORRUPT */
constexpr int32_t kRecodeStHip = -2;     /* CRYO_E_HIP: an encoder reported a size beyond its slot */
constexpr uint32_t kRecodePiece = 4096u; /* 256 lanes x 16 bytes */

__device__ inline uint64_t recode_align16(uint32_t x) { return ((uint64_t)x + 15u) & ~(uint64_t)15u; }

__global__ void __launch_bounds__(256)
k_recode_offsets(uint32_t cnt, uint64_t slot_stride, const int32_t *__restrict__ dec_status, int32_t *__restrict__ status,
                 uint32_t *__restrict__ size, uint64_t base, uint64_t *__restrict__ off, uint64_t *__restrict__ total)
{
    __shared__ uint64_t wave_sum[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t run = base; /* offset of the tile's first block: the same in every thread */
    for (uint32_t t = 0; t < cnt; t += 256u) {
        const uint32_t k = t + threadIdx.x;
        uint64_t a = 0;
        if (k < cnt) {
            int32_t st = status[k];
            uint32_t sz = size[k];
            if (dec_status[k] != 0) st = kRecodeStCorrupt;
            else if (st == 0 && (sz == 0u || (uint64_t)sz > slot_stride)) st = kRecodeStHip;
            if (st != 0) sz = 0u;
            status[k] = st;
            size[k] = sz;
            a = recode_align16(sz);
        }
        /* inclusive scan inside the wave, then across the four waves through LDS */
        uint64_t inc = a;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t up = __shfl_up((unsigned long long)inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63u) wave_sum[wave] = inc;
        __syncthreads();
        uint64_t before = 0, tile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4u; w++) {
            const uint64_t s = wave_sum[w];
            if (w < wave) before += s;
            tile += s;
        }
        if (k < cnt) off[k] = run + before + inc - a;
        run += tile;
        __syncthreads(); /* wave_sum is written again in the next turn */
    }
    if (threadIdx.x == 0) {
        off[cnt] = run;
        *total = run - base;
    }
}

/* the last k in [lo, hi] with off[k] <= x; off[lo] <= x is the caller's */
__device__ inline uint32_t recode_find(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (off[mid] <= x) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
k_recode_pack(uint32_t cnt, const uint8_t *__restrict__ slots, uint64_t slot_stride, const uint32_t *__restrict__ size,
              const uint64_t *__restrict__ off, const uint64_t *__restrict__ total, uint8_t *__restrict__ packed)
{
    const uint64_t base = off[0], end = base + *total;
    for (uint64_t p0 = base + (uint64_t)blockIdx.x * kRecodePiece; p0 < end; p0 += (uint64_t)gridDim.x * kRecodePiece) {
        const uint64_t x = p0 + threadIdx.x * 16u;
        if (x >= end) continue;
        /* off[cnt] = end > p0: the block of the piece's first byte lies in [0, cnt - 1]; a block that failed has no room and
         * is never found (its successor starts at the same offset) */
        const uint32_t k0 = recode_find(off, 0u, cnt - 1u, p0);
        const uint32_t k = off[k0 + 1u] > x ? k0 : recode_find(off, k0 + 1u, cnt - 1u, x);
        const uint64_t at = x - off[k];            /* < align16(size[k]), a multiple of 16 */
        const uint32_t sz = size[k];
        uint4 v = *reinterpret_cast<const uint4 *>(slots + (uint64_t)k * slot_stride + at);
        if (at + 16u > (uint64_t)sz) {             /* the stream's last piece: zero its pad */
            const uint32_t keep = (uint32_t)((uint64_t)sz - at); /* 1 .. 15 bytes */
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t lo = j * 4u;
                if (keep <= lo) w[j] = 0u;
                else if (keep < lo + 4u) w[j] &= (1u << (8u * (keep - lo))) - 1u;
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(packed + x) = v;
    }
}

hipError_t launch_recode_offsets(hipStream_t s, uint32_t cnt, uint64_t slot_stride, const int32_t *d_dec_status, int32_t *d_status,
                                 uint32_t *d_size, uint64_t base, uint64_t *d_off, uint64_t *d_total)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_recode_offsets, dim3(1), dim3(256), 0, s, cnt, slot_stride, d_dec_status, d_status, d_size, base, d_off,
                       d_total);
    return hipGetLastError();
}

hipError_t launch_recode_pack(hipStream_t s, uint32_t cnt, const uint8_t *d_slots, uint64_t slot_stride, const uint32_t *d_size,
                              const uint64_t *d_off, const uint64_t *d_total, uint8_t *d_packed, int cus)
{
    if (cnt == 0) return hipSuccess;
    if ((slot_stride & 15u) != 0 || (((uintptr_t)d_slots | (uintptr_t)d_packed) & 15u) != 0) return hipErrorInvalidValue;
    /* four workgroups per compute unit, but never more than the chunk's worst case has pieces */
    const uint64_t worst = ((uint64_t)cnt * slot_stride + kRecodePiece - 1u) / kRecodePiece;
    uint64_t grid = (uint64_t)(cus > 0 ? cus : 256) * 4u;
    if (grid > worst) grid = worst;
    hipLaunchKernelGGL(k_recode_pack, dim3((uint32_t)grid), dim3(256), 0, s, cnt, d_slots, slot_stride, d_size, d_off, d_total,
                       d_packed);
    return hipGetLastError();
}

} // namespace cryo
