/*
 * xxh64.h -- XXH64 (seed 0) of many blocks at once: the content checksum of a zstd frame is its low 32 bits, stored after
 * the frame's last block (RFC 8878 3.1.1).
 *
 * XXH64 runs four accumulators over 32-byte stripes, each of them serial, and merges them at the end.  Inside one block
 * there is no more parallelism than that, so it comes from the number of blocks: a quad of lanes hashes one block (lane a
 * carries accumulator a), 16 blocks per wave.
 *   - Every round a quad takes the next 512 bytes of its block with 16-byte loads, four lanes side by side, so each load
 *     instruction reads whole 64-byte lines of it.  They are loaded one round ahead, into registers, while the round
 *     before is hashed.
 *   - They are staged through LDS, where lane a reads the 8 bytes of each stripe that belong to its accumulator.  Blocks lie
 *     kXxPitch bytes apart there, 8 banks on from each other: the eight blocks of a half-wave read 64 different banks.
 *   - The 64-bit multiplies are written out of 32-bit ones (v_mad_u64_u32 for the low product, two v_mul_lo_u32 for the
 *     cross terms), so that no call to a 64-bit multiply helper can appear.
 *   - Merge, the last 0..31 bytes (8 / 4 / 1-byte steps) and the avalanche run in the quad's first lane.
 * A block of B bytes is B / 32 dependent rounds per lane (32 768 for 1 MiB), each two 64-bit multiplies.  Alone in a wave,
 * a 1 MiB block takes about 2 ms (profiles/r10_zstd_checksum.txt): one round of 512 bytes in flight per quad leaves it
 * waiting on memory latency.  Many blocks are bound by the reads instead: 65 536 x 128 KiB in about 1.4 ms.
 */
#ifndef CRYO_XXH64_H
#define CRYO_XXH64_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cryo {

constexpr uint32_t kXxChunk = 512;                  /* bytes of a block per round */
constexpr uint32_t kXxPitch = kXxChunk + 32;        /* LDS bytes per block */
constexpr uint32_t kXxBlocksPerWave = 16;
constexpr uint32_t kXxLdsPerWave = kXxBlocksPerWave * kXxPitch;

constexpr uint64_t kXP1 = 11400714785074694791ull, kXP2 = 14029467366897019727ull, kXP3 = 1609587929392839161ull,
                   kXP4 = 9650029242287828579ull, kXP5 = 2870177450012600261ull;

__device__ inline uint64_t xx_mul(uint64_t a, uint64_t b)
{
    const uint32_t al = (uint32_t)a, ah = (uint32_t)(a >> 32), bl = (uint32_t)b, bh = (uint32_t)(b >> 32);
    const uint64_t lo = (uint64_t)al * bl;
    const uint32_t hi = (uint32_t)(lo >> 32) + al * bh + ah * bl;
    return ((uint64_t)hi << 32) | (uint32_t)lo;
}
__device__ inline uint64_t xx_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ inline uint64_t xx_round(uint64_t acc, uint64_t v) { return xx_mul(xx_rotl(acc + xx_mul(v, kXP2), 31), kXP1); }
__device__ inline uint64_t xx_merge(uint64_t h, uint64_t v) { return xx_mul(h ^ xx_round(0, v), kXP1) + kXP4; }

/* 16 bytes at p + o: one load where the block starts 16-byte aligned, else from the aligned dwords around them (the fifth
 * only where the bytes reach into it) */
__device__ inline uint4 xx_ld16(const uint8_t *p, uint32_t o, bool al16)
{
    if (al16) return *reinterpret_cast<const uint4 *>(p + o);
    const uint32_t mis = (uint32_t)((uintptr_t)(p + o) & 3u), sh = mis * 8u;
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p + o - mis); /* (pointer arithmetic: the loads stay global ones) */
    const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = sh ? q[4] : 0u;
    return make_uint4(__builtin_amdgcn_alignbit(w1, w0, sh), __builtin_amdgcn_alignbit(w2, w1, sh),
                      __builtin_amdgcn_alignbit(w3, w2, sh), __builtin_amdgcn_alignbit(w4, w3, sh));
}

__device__ inline uint64_t xx_shfl64(uint64_t v, uint32_t from)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, (int)from, 64);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)from, 64);
    return ((uint64_t)hi << 32) | lo;
}

/* XXH64 of p[0 .. n) for the quad of `lane` (n = 0: the quad has no block).  Every lane of the wave calls it: the shuffles
 * of the merge need the whole wave.  lds: this wave's kXxLdsPerWave bytes, 16-byte aligned.  The hash is valid in the
 * quad's first lane (lane % 4 == 0). */
__device__ inline uint64_t xxh64_quad(const uint8_t *p, uint32_t n, uint8_t *lds, uint32_t lane)
{
    const uint32_t a = lane & 3u;
    uint8_t *mine = lds + (lane >> 2) * kXxPitch;
    const uint32_t body = n & ~31u; /* whole stripes */
    const bool al16 = ((uintptr_t)p & 15u) == 0u;
    uint64_t v = a == 0u ? kXP1 + kXP2 : (a == 1u ? kXP2 : (a == 2u ? 0ull : 0ull - kXP1));
    uint4 r[kXxChunk / 64u];
    auto load = [&](uint32_t c0) {
#pragma unroll
        for (uint32_t k = 0; k < kXxChunk / 64u; k++) {
            const uint32_t o = c0 + k * 64u + a * 16u;
            if (o + 16u <= body) r[k] = xx_ld16(p, o, al16);
        }
    };
    load(0);
    for (uint32_t c0 = 0; c0 < body; c0 += kXxChunk) {
#pragma unroll
        for (uint32_t k = 0; k < kXxChunk / 64u; k++) *reinterpret_cast<uint4 *>(mine + k * 64u + a * 16u) = r[k];
        __builtin_amdgcn_wave_barrier();
        load(c0 + kXxChunk);
        if (body - c0 >= kXxChunk) {
#pragma unroll
            for (uint32_t s = 0; s < kXxChunk / 32u; s++) {
                const uint2 w = *reinterpret_cast<const uint2 *>(mine + s * 32u + a * 8u);
                v = xx_round(v, (uint64_t)w.x | ((uint64_t)w.y << 32));
            }
        } else {
            for (uint32_t s = 0; s < (body - c0) / 32u; s++) {
                const uint2 w = *reinterpret_cast<const uint2 *>(mine + s * 32u + a * 8u);
                v = xx_round(v, (uint64_t)w.x | ((uint64_t)w.y << 32));
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    const uint32_t q0 = lane & ~3u;
    const uint64_t v1 = xx_shfl64(v, q0), v2 = xx_shfl64(v, q0 + 1u), v3 = xx_shfl64(v, q0 + 2u), v4 = xx_shfl64(v, q0 + 3u);
    uint64_t h = 0;
    if (a == 0u) {
        if (n >= 32u) {
            h = xx_rotl(v1, 1) + xx_rotl(v2, 7) + xx_rotl(v3, 12) + xx_rotl(v4, 18);
            h = xx_merge(h, v1); h = xx_merge(h, v2); h = xx_merge(h, v3); h = xx_merge(h, v4);
        } else h = kXP5;
        h += n;
        uint32_t o = body;
        for (; o + 8u <= n; o += 8u) {
            uint64_t x;
            __builtin_memcpy(&x, p + o, 8);
            h ^= xx_round(0, x);
            h = xx_mul(xx_rotl(h, 27), kXP1) + kXP4;
        }
        if (o + 4u <= n) {
            uint32_t x;
            __builtin_memcpy(&x, p + o, 4);
            h ^= xx_mul(x, kXP1);
            h = xx_mul(xx_rotl(h, 23), kXP2) + kXP3;
            o += 4u;
        }
        for (; o < n; o++) { h ^= xx_mul(p[o], kXP5); h = xx_mul(xx_rotl(h, 11), kXP1); }
        h ^= h >> 33; h = xx_mul(h, kXP2); h ^= h >> 29; h = xx_mul(h, kXP3); h ^= h >> 32;
    }
    return h;
}

} // namespace cryo

#endif
