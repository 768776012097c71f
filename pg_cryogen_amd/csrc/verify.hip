/*
 * verify.hip -- the device side of write verification (CRYO_OPT_ENCODE_VERIFY, cryo_codec_verify_batch).
 *
 * The host (cryo_codec.cpp, verify_pass) decodes the compressed blocks of a call with the normal automatic decode
 * routes into handle workspace; these kernels set the decode up and compare what came out with the raw blocks:
 *   k_verify_prep  one lane per block: the stream table the decoders read (offset, size; size 0 for a block whose
 *                  encode already failed or whose size does not fit its slot), the first-mismatch word set to "none"
 *   k_verify       one workgroup per 16 KiB piece of a block: 16 bytes per lane, four loads of each stream in flight;
 *                  the first differing byte of a wave is found with a ballot and folded into the block's word with a
 *                  vector atomicMin (every store here is a vector store)
 *   k_verify_fold  one lane per block: the block's status (CRYO_OK / CRYO_E_VERIFY / the encode error it had)
 */
#include "kernels.h"

namespace cryo {

constexpr uint32_t kVerifyNone = 0xffffffffu;
constexpr int32_t kStVerify = -8; /* CRYO_E_VERIFY */
constexpr uint32_t kVerifyLoads = 4;
constexpr uint32_t kVerifyPiece = 256u * 16u * kVerifyLoads; /* bytes one workgroup compares */

__global__ void __launch_bounds__(256)
k_verify_prep(uint64_t lo, uint32_t cnt, const uint64_t *__restrict__ comp_off, uint64_t comp_stride,
              const uint32_t *__restrict__ comp_size, const int32_t *__restrict__ enc_status, uint64_t e0, uint64_t e1,
              uint64_t edge_stride, uint64_t *__restrict__ off, uint32_t *__restrict__ size, uint32_t *__restrict__ first)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint64_t i = lo + k;
    uint32_t sz = comp_size[i];
    if (enc_status && enc_status[i] != 0) sz = 0;               /* not decoded: it keeps its encode error */
    if (!comp_off && (uint64_t)sz > comp_stride) sz = 0;        /* a size beyond its slot is never read */
    off[k] = comp_off ? comp_off[i] : i * comp_stride;
    size[k] = sz;
    first[i] = kVerifyNone;
    /* the edge blocks (their slots copied into padded workspace: e0's copy first, e1's edge_stride bytes later) have their
     * own two entries behind the chunk's */
    if (i == e0) { off[cnt] = 0; size[cnt] = sz; }
    if (i == e1) { off[cnt + 1] = edge_stride; size[cnt + 1] = sz; }
}

/* first differing byte of two 16-byte pieces (16: none) */
__device__ inline uint32_t first_diff16(const uint4 &a, const uint4 &b)
{
    const uint32_t d[4] = {a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w};
#pragma unroll
    for (int w = 0; w < 4; w++)
        if (d[w]) return (uint32_t)w * 4u + ((uint32_t)__builtin_ctz(d[w]) >> 3);
    return 16u;
}

/* the decoder's status of chunk entry k: the edge blocks were decoded by a call of their own, into the entries behind the chunk's */
__device__ inline int32_t verify_dec_status(const int32_t *dec_status, uint64_t lo, uint32_t k, uint32_t cnt, uint64_t e0, uint64_t e1)
{
    const uint64_t i = lo + k;
    return i == e0 ? dec_status[cnt] : i == e1 ? dec_status[cnt + 1] : dec_status[k];
}

__global__ void __launch_bounds__(256)
k_verify(const uint8_t *__restrict__ raw, uint64_t raw_stride, const uint8_t *__restrict__ dec, uint64_t dec_stride,
         uint32_t B, uint64_t lo, uint32_t cnt, uint32_t pieces, const uint32_t *__restrict__ size,
         const int32_t *__restrict__ dec_status, uint64_t e0, uint64_t e1, uint32_t *__restrict__ first)
{
    const uint32_t k = blockIdx.x / pieces, pc = blockIdx.x - k * pieces;
    if (size[k] == 0 || verify_dec_status(dec_status, lo, k, cnt, e0, e1) != 0) return; /* not decoded, or the decoder rejected it: nothing to compare */
    const uint8_t *pr = raw + (lo + k) * raw_stride;
    const uint8_t *pd = dec + (uint64_t)k * dec_stride;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t base = pc * kVerifyPiece + threadIdx.x * 16u;
    uint32_t at[kVerifyLoads];
    const bool full = pc * kVerifyPiece + kVerifyPiece <= B;
    if (full && (((uintptr_t)pr | (uintptr_t)pd) & 15u) == 0) {
        uint4 x[kVerifyLoads], y[kVerifyLoads];
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) {
            x[j] = *reinterpret_cast<const uint4 *>(pr + base + j * 4096u);
            y[j] = *reinterpret_cast<const uint4 *>(pd + base + j * 4096u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) at[j] = first_diff16(x[j], y[j]);
    } else if (full && ((uintptr_t)pd & 15u) == 0 && ((uintptr_t)pr & 3u) == 0) {
        /* raw rows 4-byte aligned only (a block size that is a multiple of 4 but not of 16): four dword loads per piece */
        uint4 x[kVerifyLoads], y[kVerifyLoads];
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(pr + base + j * 4096u);
            x[j] = make_uint4(q[0], q[1], q[2], q[3]);
            y[j] = *reinterpret_cast<const uint4 *>(pd + base + j * 4096u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) at[j] = first_diff16(x[j], y[j]);
    } else if (full && ((uintptr_t)pd & 15u) == 0) {
        /* raw rows at any byte offset (odd block sizes): the decoded row in 16-byte loads, the raw bytes shifted into words
         * from the two aligned dwords around each one (five aligned dword loads per 16 bytes, all in flight) */
        const uint32_t sh = (uint32_t)((uintptr_t)pr & 3u) * 8u;
        const uint32_t *qa = reinterpret_cast<const uint32_t *>((uintptr_t)pr & ~(uintptr_t)3u);
        uint4 x[kVerifyLoads], y[kVerifyLoads];
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) {
            const uint32_t *q = qa + ((base + j * 4096u) >> 2);
            const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4];
            x[j] = make_uint4(__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh),
                              __builtin_amdgcn_alignbit(w3, w2, sh), __builtin_amdgcn_alignbit(w4, w3, sh));
            y[j] = *reinterpret_cast<const uint4 *>(pd + base + j * 4096u);
        }
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) at[j] = first_diff16(x[j], y[j]);
    } else {
        /* the block's last piece (or an unaligned decoded row, which the host never hands over): byte by byte */
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLoads; j++) {
            at[j] = 16u;
            const uint32_t o = base + j * 4096u;
            for (uint32_t b = 0; b < 16u && o + b < B; b++)
                if (pr[o + b] != pd[o + b]) { at[j] = b; break; }
        }
    }
    /* load j of a wave covers 1 KiB that comes before load j + 1's, lanes in order inside it: the wave's first mismatch is
     * that of the lowest lane in the first load whose ballot is not empty */
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLoads; j++) {
        const unsigned long long m = __ballot(at[j] < 16u);
        if (m) {
            if (lane == (uint32_t)__builtin_ctzll(m)) atomicMin(first + lo + k, base + j * 4096u + at[j]);
            return;
        }
    }
}

__global__ void __launch_bounds__(256)
k_verify_fold(uint64_t lo, uint32_t cnt, const uint32_t *__restrict__ size, const int32_t *__restrict__ dec_status,
              uint64_t e0, uint64_t e1, bool has_enc_status, int32_t *__restrict__ status, uint32_t *__restrict__ first)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cnt) return;
    const uint64_t i = lo + k;
    if (has_enc_status && status[i] != 0) return;                /* the encode error stands */
    const int32_t ds = verify_dec_status(dec_status, lo, k, cnt, e0, e1);
    if (size[k] == 0 || ds != 0) { first[i] = kVerifyNone; status[i] = kStVerify; return; }
    status[i] = first[i] == kVerifyNone ? 0 : kStVerify;
}

hipError_t launch_verify_prep(hipStream_t s, uint64_t lo, uint32_t cnt, const uint64_t *d_comp_off, uint64_t comp_stride,
                              const uint32_t *d_comp_size, const int32_t *d_enc_status, uint64_t e0, uint64_t e1,
                              uint64_t edge_stride, uint64_t *d_off, uint32_t *d_size, uint32_t *d_first)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_verify_prep, dim3((cnt + 255u) / 256u), dim3(256), 0, s, lo, cnt, d_comp_off, comp_stride, d_comp_size,
                       d_enc_status, e0, e1, edge_stride, d_off, d_size, d_first);
    return hipGetLastError();
}

hipError_t launch_verify_compare(hipStream_t s, const uint8_t *d_raw, uint64_t raw_stride, const uint8_t *d_dec,
                                 uint64_t dec_stride, uint32_t block_size, uint64_t lo, uint32_t cnt, const uint32_t *d_size,
                                 const int32_t *d_dec_status, uint64_t e0, uint64_t e1, uint32_t *d_first)
{
    if (cnt == 0) return hipSuccess;
    const uint32_t pieces = (block_size + kVerifyPiece - 1u) / kVerifyPiece;
    const uint64_t grid = (uint64_t)cnt * pieces;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_verify, dim3((uint32_t)grid), dim3(256), 0, s, d_raw, raw_stride, d_dec, dec_stride, block_size, lo,
                       cnt, pieces, d_size, d_dec_status, e0, e1, d_first);
    return hipGetLastError();
}

hipError_t launch_verify_fold(hipStream_t s, uint64_t lo, uint32_t cnt, const uint32_t *d_size, const int32_t *d_dec_status,
                              uint64_t e0, uint64_t e1, bool has_enc_status, int32_t *d_status, uint32_t *d_first)
{
    if (cnt == 0) return hipSuccess;
    hipLaunchKernelGGL(k_verify_fold, dim3((cnt + 255u) / 256u), dim3(256), 0, s, lo, cnt, d_size, d_dec_status, e0, e1,
                       has_enc_status, d_status, d_first);
    return hipGetLastError();
}

} // namespace cryo
