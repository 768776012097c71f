/*
 * xxh64.hip -- the content checksum of the zstd frames the encoders write (CRYO_OPT_ZSTD_CHECKSUM).
 *
 * The encoders write exactly libzstd's frames without a checksum.  libzstd's frames with one (ZSTD_c_checksumFlag = 1) differ
 * from those in two places only: bit 2 of the frame header descriptor (byte 4) is set, and the low 32 bits of XXH64 of the
 * block's input follow the last block, little-endian.  So one kernel after the encode makes the one from the other:
 *   k_zstd_ck_append  a quad of lanes per block, 16 blocks per wave (xxh64.h): XXH64 of the raw input (never of the output),
 *                     then, in the quad's first lane and for a block whose status is CRYO_OK, the descriptor bit, the four
 *                     bytes at dst + out_size[i], and out_size[i] + 4.
 * Every store is a vector store.
 */
#include "kernels.h"
#include "xxh64.h"

namespace cryo {

namespace {

constexpr int32_t kStDstSize = -5; /* CRYO_E_DSTSIZE */

__global__ void __launch_bounds__(64)
k_zstd_ck_append(const uint8_t *__restrict__ src, uint64_t src_stride, uint32_t B, uint64_t n_blocks, uint8_t *__restrict__ dst,
                 uint64_t dst_stride, uint32_t *__restrict__ out_size, int32_t *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kXxLdsPerWave];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kXxBlocksPerWave + (lane >> 2);
    const bool on = i < n_blocks && status[i] == CRYO_ST_OK;
    const uint64_t h = xxh64_quad(on ? src + i * src_stride : src, on ? B : 0u, lds, lane);
    if (!on || (lane & 3u) != 0u) return;
    uint8_t *d = dst + i * dst_stride;
    const uint32_t sz = out_size[i];
    if ((uint64_t)sz + 4u > dst_stride || sz < 5u) { status[i] = kStDstSize; out_size[i] = 0; return; } /* never: the bound leaves room */
    d[4] = (uint8_t)(d[4] | 0x04u);
    d[sz] = (uint8_t)h; d[sz + 1u] = (uint8_t)(h >> 8); d[sz + 2u] = (uint8_t)(h >> 16); d[sz + 3u] = (uint8_t)(h >> 24);
    out_size[i] = sz + 4u;
}

} // namespace

hipError_t launch_zstd_checksum_append(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                       uint64_t n_blocks, uint8_t *d_dst, uint64_t dst_stride, uint32_t *d_out_size,
                                       int32_t *d_status)
{
    if (n_blocks == 0) return hipSuccess;
    const uint64_t grid = (n_blocks + kXxBlocksPerWave - 1u) / kXxBlocksPerWave;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_zstd_ck_append, dim3((uint32_t)grid), dim3(64), 0, s, d_src, src_stride, block_size, n_blocks, d_dst,
                       dst_stride, d_out_size, d_status);
    return hipGetLastError();
}

} // namespace cryo
