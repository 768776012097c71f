/*
 * enc_seg.hip -- segment-parallel block encode (CRYO_OPT_ENCODE_SEGMENT_BYTES = S): the second half of it, which turns the
 * segments' pieces into one LZ4 block / one zstd frame per cryo block.
 *
 * A 1 MiB cryo block encoded by one wave takes 41 ms (LZ4) / 81 ms (zstd-1) -- the write path of the access method hands
 * the codec one block per call, so that latency is what a COPY sees (profiles/r06_crossover.txt).  With the option set,
 * a block of more than S bytes is cut into ceil(B / S) segments and every (block, segment) gets its own wave:
 *   - LZ4 (k_lz4_enc2<..., SEG = true>, lz4_enc2.hip): each segment is parsed over its own position table, seeded with
 *     positions of the bytes before it (matches reach back into earlier segments, offsets <= 65 535).  A segment's output
 *     is complete sequences plus a trailing literal run.  Here the trailing runs are carried forward: the first sequence
 *     of the next segment that has one absorbs every carried literal (its token and literal-length bytes are rewritten);
 *     the last segment's run, with whatever is carried into it, is the block's last literals.  A scan over the pieces'
 *     sizes places them and a copy pass (one wave per segment) moves them, the carried literals straight from the input.
 *   - zstd (k_zstd_enc in segment mode, zstd_enc.hip, strategy `fast`): each segment is one zstd block of the frame,
 *     encoded with fresh Huffman and FSE tables, repeat offsets used only once the block's own raw offsets have set them,
 *     the last-block bit only on the final one.  Here: the frame header (the byte-identical path's), a scan over the
 *     blocks' sizes, and a copy pass.
 * The result is a valid stream that liblz4 1.9.3 / libzstd 1.4.8 decode to the input, deterministic (a block's bytes do
 * not depend on the batch it is in), but not the libraries' own output.
 */
#include "lz_common.h"
#include "kernels.h"

namespace cryo {

hipError_t launch_lz4_enc_segments(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                   uint64_t n_blocks, uint32_t seg_bytes, uint32_t nseg, uint8_t *d_seg, uint64_t seg_stride,
                                   int accel, uint32_t *d_seg_size, uint2 *d_seg_rec);

namespace {

/* n bytes, the wave: 16 bytes per lane where a whole piece fits, the rest byte by byte (never reads behind src + n) */
__device__ inline void seg_copy(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t lane)
{
    uint32_t o = 0;
    for (; o + 4096u <= n; o += 4096u) {
        uint4 a, b, c, d;
        __builtin_memcpy(&a, src + o + 16u * lane, 16);
        __builtin_memcpy(&b, src + o + 1024u + 16u * lane, 16);
        __builtin_memcpy(&c, src + o + 2048u + 16u * lane, 16);
        __builtin_memcpy(&d, src + o + 3072u + 16u * lane, 16);
        __builtin_memcpy(dst + o + 16u * lane, &a, 16);
        __builtin_memcpy(dst + o + 1024u + 16u * lane, &b, 16);
        __builtin_memcpy(dst + o + 2048u + 16u * lane, &c, 16);
        __builtin_memcpy(dst + o + 3072u + 16u * lane, &d, 16);
    }
    for (; o + 1024u <= n; o += 1024u) {
        uint4 a;
        __builtin_memcpy(&a, src + o + 16u * lane, 16);
        __builtin_memcpy(dst + o + 16u * lane, &a, 16);
    }
    for (uint32_t i = o + lane; i < n; i += 64u) dst[i] = src[i];
}

__host__ __device__ inline uint32_t lz4_len_bytes(uint32_t len) { return len >= 15u ? (len - 15u) / 255u + 1u : 0u; }

/* token + literal-length bytes of a run of `len` literals, match nibble `mnib`, at dst */
__device__ inline void lz4_put_head(uint8_t *dst, uint32_t len, uint32_t mnib, uint32_t lane)
{
    const uint32_t nl = lz4_len_bytes(len);
    if (lane == 0) dst[0] = (uint8_t)(((len < 15u ? len : 15u) << 4) | mnib);
    if (nl) {
        for (uint32_t i = lane; i + 1u < nl; i += 64u) dst[1u + i] = 255;
        if (lane == 0) dst[nl] = (uint8_t)(len - 15u - 255u * (nl - 1u));
    }
}

/* the plan of one segment: where its pieces go */
enum : uint32_t { kSegHas = 1, kSegLast = 2, kSegHead = 4 };
struct SegPlan {
    uint32_t out_off;  /* (kSegHead) where the rewritten token + literal length go */
    uint32_t lit_len;  /* (kSegHead) the literal run that token announces */
    uint32_t hl;       /* (kSegHas) bytes of the segment's own first token + literal length (skipped) */
    uint32_t body_dst; /* (kSegHas) where its output from hl on goes (up to its trailing run, or to its end if last) */
    uint32_t lfrom, lto, ldst; /* input bytes [lfrom, lto) that are literals of a carried run, and where they land */
    uint32_t flags;
};
constexpr uint32_t kNoAbs = 0xFFFFFFFFu;

/* one wave per block: walks its segments in order (64 at a time: each lane reads one segment's record and parses its first
 * sequence's literal length, then the carries go through the 64 serially, wave-uniform) and writes their plans */
__global__ void __launch_bounds__(64)
k_lz4_seg_plan(uint32_t n, uint64_t n_blocks, uint32_t seg_bytes, uint32_t nseg, const uint8_t *__restrict__ d_seg,
               uint64_t seg_stride, const uint32_t *__restrict__ seg_size, const uint2 *__restrict__ seg_rec,
               SegPlan *__restrict__ plan, uint2 *__restrict__ absorb, uint32_t *__restrict__ out_size,
               int32_t *__restrict__ status)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t blk = blockIdx.x;
    if (blk >= n_blocks) return;
    const uint64_t first = blk * nseg;
    uint32_t cs = 0, off = 0; /* start of the literal run being carried; output bytes so far */
    for (uint32_t c0 = 0; c0 < nseg; c0 += 64u) {
        const uint32_t i = c0 + lane;
        const bool on = i < nseg;
        uint32_t tail = 0, anc = 0, size = 0, lit0 = 0, hl = 0, mnib = 0;
        if (on) {
            const uint2 r = seg_rec[first + i];
            tail = r.x; anc = r.y; size = seg_size[first + i];
            if (tail) { /* the first sequence's literal length */
                const uint8_t *p = d_seg + (first + i) * seg_stride;
                const uint32_t tok = p[0];
                mnib = tok & 15u;
                lit0 = tok >> 4;
                hl = 1;
                if (lit0 == 15u) {
                    uint32_t b;
                    do { b = p[hl++]; lit0 += b; } while (b == 255u);
                }
            }
        }
        SegPlan pl = {0, 0, 0, 0, 0, 0, 0, 0};
        uint2 ab = make_uint2(kNoAbs, 0);
        const uint32_t cn = nseg - c0 < 64u ? nseg - c0 : 64u;
        for (uint32_t k = 0; k < cn; k++) {
            const uint32_t si = c0 + k, s0 = si * seg_bytes, s1 = n - s0 > seg_bytes ? s0 + seg_bytes : n;
            const bool last = si + 1u == nseg;
            const uint32_t kt = lane_get(tail, k), ka = lane_get(anc, k), ks = lane_get(size, k), kl = lane_get(lit0, k),
                           kh = lane_get(hl, k);
            uint32_t sz;
            if (kt) {
                const uint32_t c = s0 - cs, L = c + kl, hn = 1u + lz4_len_bytes(L);
                if (lane == k) {
                    pl.out_off = off; pl.lit_len = L; pl.hl = kh; pl.body_dst = off + hn + c;
                    pl.flags = kSegHas | kSegHead | (last ? kSegLast : 0u);
                    if (!last) { pl.lfrom = ka; pl.lto = s1; }
                    ab = make_uint2(off + hn, cs);
                }
                sz = hn + c + (kt - kh) + (last ? ks - kt : 0u);
                cs = ka;
            } else if (last) {
                const uint32_t L = n - cs, hn = 1u + lz4_len_bytes(L);
                if (lane == k) {
                    pl.out_off = off; pl.lit_len = L; pl.flags = kSegHead | kSegLast; pl.lfrom = s0; pl.lto = s1;
                    ab = make_uint2(off + hn, cs);
                }
                sz = hn + L;
            } else {
                if (lane == k) { pl.lfrom = s0; pl.lto = s1; }
                sz = 0;
            }
            off += sz;
        }
        if (on) {
            pl.flags |= mnib << 8; /* the match nibble of the first token rides in the flags */
            plan[first + i] = pl;
            absorb[first + i] = ab;
        }
    }
    const uint32_t bound = n + n / 255u + 16u;
    if (off > bound) {
        /* cannot happen with the greedy parse (a sequence never costs more than the literals it replaces); kept so that the
         * bound holds whatever: the block goes out as one literal run */
        const uint32_t hn = 1u + lz4_len_bytes(n);
        for (uint32_t i = lane; i < nseg; i += 64u) {
            const uint32_t s0 = i * seg_bytes, s1 = n - s0 > seg_bytes ? s0 + seg_bytes : n;
            SegPlan pl = {0, n, 0, 0, s0, s1, hn + s0, i == 0u ? kSegHead : 0u};
            plan[first + i] = pl;
        }
        off = hn + n;
    } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        /* where each segment's carried literals land: in the run of the next segment that absorbs (the next one with a
         * sequence, else the last) -- a walk from the end */
        uint2 nxt = make_uint2(kNoAbs, 0);
        for (int64_t c0 = (int64_t)((nseg - 1u) & ~63u); c0 >= 0; c0 -= 64) {
            const uint32_t i = (uint32_t)c0 + lane;
            const bool on = i < nseg;
            const uint2 ab = on ? absorb[first + i] : make_uint2(kNoAbs, 0);
            const uint32_t fl = on ? plan[first + i].flags : 0u;
            const uint32_t cn = nseg - (uint32_t)c0 < 64u ? nseg - (uint32_t)c0 : 64u;
            uint2 mine = make_uint2(kNoAbs, 0);
            for (int k = (int)cn - 1; k >= 0; k--) {
                const uint32_t kx = lane_get(ab.x, (uint32_t)k), ky = lane_get(ab.y, (uint32_t)k), kf = lane_get(fl, (uint32_t)k);
                const bool has = (kf & kSegHas) != 0u, last = (kf & kSegLast) != 0u;
                if (!has && last) nxt = make_uint2(kx, ky); /* the last segment without a sequence takes its own bytes */
                if (lane == (uint32_t)k) mine = nxt;
                if (has) nxt = make_uint2(kx, ky);
            }
            if (on) {
                SegPlan pl = plan[first + i];
                if (pl.lto > pl.lfrom) pl.ldst = mine.x + (pl.lfrom - mine.y);
                plan[first + i] = pl;
            }
        }
    }
    if (lane == 0) { out_size[blk] = off; status[blk] = CRYO_ST_OK; }
}

/* one wave per (block, segment): its pieces to their places */
__global__ void __launch_bounds__(64)
k_lz4_seg_copy(const uint8_t *__restrict__ src_base, uint64_t src_stride, uint64_t n_blocks, uint32_t nseg,
               const uint8_t *__restrict__ d_seg, uint64_t seg_stride, const uint32_t *__restrict__ seg_size,
               const uint2 *__restrict__ seg_rec, const SegPlan *__restrict__ plan, uint8_t *__restrict__ dst_base,
               uint64_t dst_stride)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = blockIdx.x, blk = item / nseg;
    if (blk >= n_blocks) return;
    const SegPlan pl = plan[item];
    const uint8_t *src = src_base + blk * src_stride;
    uint8_t *dst = dst_base + blk * dst_stride;
    if (pl.flags & kSegHead) lz4_put_head(dst + pl.out_off, pl.lit_len, (pl.flags >> 8) & 15u, lane);
    if (pl.flags & kSegHas) {
        const uint32_t end = (pl.flags & kSegLast) ? seg_size[item] : seg_rec[item].x;
        seg_copy(dst + pl.body_dst, d_seg + item * seg_stride + pl.hl, end - pl.hl, lane);
    }
    if (pl.lto > pl.lfrom) seg_copy(dst + pl.ldst, src + pl.lfrom, pl.lto - pl.lfrom, lane);
}

/* zstd: one wave per block -- the frame header, and each block's place behind it */
struct ZHead { uint8_t b[16]; uint32_t len; };
__global__ void __launch_bounds__(64)
k_zstd_seg_plan(uint64_t n_blocks, uint32_t nseg, const uint32_t *__restrict__ seg_size, uint32_t *__restrict__ seg_off,
                ZHead head, uint32_t bound, uint32_t trailer, uint8_t *__restrict__ dst_base, uint64_t dst_stride, uint32_t *__restrict__ out_size,
                int32_t *__restrict__ status)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t blk = blockIdx.x;
    if (blk >= n_blocks) return;
    const uint64_t first = blk * nseg;
    if (lane < head.len) dst_base[blk * dst_stride + lane] = head.b[lane];
    uint32_t off = head.len;
    for (uint32_t c0 = 0; c0 < nseg; c0 += 64u) {
        const uint32_t i = c0 + lane;
        const uint32_t sz = i < nseg ? seg_size[first + i] : 0u;
        const uint32_t incl = scan64_incl(sz);
        if (i < nseg) seg_off[first + i] = off + incl - sz;
        off += lane_get(incl, 63u);
    }
    /* ceil(B / S) block headers of 3 bytes, raw blocks at worst, and a content checksum (trailer): always within bound */
    const bool fits = off + trailer <= bound;
    if (!fits)
        for (uint32_t i = lane; i < nseg; i += 64u) seg_off[first + i] = 0xFFFFFFFFu;
    if (lane == 0) { out_size[blk] = fits ? off : 0u; status[blk] = fits ? CRYO_ST_OK : -5 /* CRYO_E_DSTSIZE */; }
}

__global__ void __launch_bounds__(64)
k_zstd_seg_copy(uint64_t n_blocks, uint32_t nseg, const uint8_t *__restrict__ d_seg, uint64_t seg_stride,
                const uint32_t *__restrict__ seg_size, const uint32_t *__restrict__ seg_off, uint8_t *__restrict__ dst_base,
                uint64_t dst_stride)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t item = blockIdx.x, blk = item / nseg;
    if (blk >= n_blocks) return;
    const uint32_t o = seg_off[item];
    if (o == 0xFFFFFFFFu) return;
    seg_copy(dst_base + blk * dst_stride + o, d_seg + item * seg_stride, seg_size[item], lane);
}

/* per-segment scratch: a segment's own output (LZ4: at most its bound; zstd: a block header + at most its size + the 32
 * bytes of slack the entropy stage may write before it gives up) */
inline uint64_t lz4_seg_stride(uint32_t seg_bytes) { return ((uint64_t)seg_bytes + seg_bytes / 255u + 16u + 255u) & ~(uint64_t)255u; }
inline uint64_t zstd_seg_stride(uint32_t seg_bytes) { return (uint64_t)seg_bytes + 256u; }
inline size_t al256(size_t v) { return (v + 255u) & ~(size_t)255u; }

struct Lz4SegWs { size_t seg, size, rec, plan, absorb, bytes; };
Lz4SegWs lz4_seg_ws(uint64_t items, uint32_t seg_bytes)
{
    Lz4SegWs w;
    w.seg = 0;
    w.size = al256(items * lz4_seg_stride(seg_bytes));
    w.rec = w.size + al256(items * 4u);
    w.plan = w.rec + al256(items * sizeof(uint2));
    w.absorb = w.plan + al256(items * sizeof(SegPlan));
    w.bytes = w.absorb + al256(items * sizeof(uint2));
    return w;
}

} // namespace

uint32_t enc_seg_count(uint32_t block_size, uint32_t seg_bytes) { return (block_size + seg_bytes - 1u) / seg_bytes; }

size_t lz4_compress_segmented_workspace(uint64_t n_blocks, uint32_t block_size, uint32_t seg_bytes)
{
    return lz4_seg_ws(n_blocks * enc_seg_count(block_size, seg_bytes), seg_bytes).bytes;
}

hipError_t launch_lz4_compress_segmented(hipStream_t s, const uint8_t *d_src, uint64_t src_stride, uint32_t block_size,
                                         uint64_t n_blocks, uint8_t *d_dst, uint64_t dst_stride, int accel, uint32_t seg_bytes,
                                         uint32_t *d_out_size, int32_t *d_status, void *d_ws, size_t ws_bytes)
{
    if (n_blocks == 0) return hipSuccess;
    const uint32_t nseg = enc_seg_count(block_size, seg_bytes);
    const uint64_t items = n_blocks * nseg;
    const Lz4SegWs w = lz4_seg_ws(items, seg_bytes);
    if (ws_bytes < w.bytes || items > 0x7fffffffull) return hipErrorInvalidValue;
    uint8_t *ws = (uint8_t *)d_ws;
    uint8_t *seg = ws + w.seg;
    uint32_t *size = (uint32_t *)(ws + w.size);
    uint2 *rec = (uint2 *)(ws + w.rec);
    SegPlan *plan = (SegPlan *)(ws + w.plan);
    uint2 *absorb = (uint2 *)(ws + w.absorb);
    const uint64_t stride = lz4_seg_stride(seg_bytes);
    hipError_t e = launch_lz4_enc_segments(s, d_src, src_stride, block_size, n_blocks, seg_bytes, nseg, seg, stride, accel, size, rec);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lz4_seg_plan, dim3((uint32_t)n_blocks), dim3(64), 0, s, block_size, n_blocks, seg_bytes, nseg, seg, stride,
                       size, rec, plan, absorb, d_out_size, d_status);
    hipLaunchKernelGGL(k_lz4_seg_copy, dim3((uint32_t)items), dim3(64), 0, s, d_src, src_stride, n_blocks, nseg, seg, stride, size, rec,
                       plan, d_dst, dst_stride);
    return hipGetLastError();
}

/* zstd: the scratch the segment pass writes to lies behind the encoder's own workspace (zstd_enc.hip) */
size_t zstd_seg_scratch_bytes(uint64_t items, uint32_t seg_bytes)
{
    return al256(items * zstd_seg_stride(seg_bytes)) + 2u * al256(items * 4u);
}
uint64_t zstd_seg_slot_stride(uint32_t seg_bytes) { return zstd_seg_stride(seg_bytes); }

hipError_t launch_zstd_seg_concat(hipStream_t s, uint64_t n_blocks, uint32_t nseg, uint32_t seg_bytes, const uint8_t *d_seg,
                                  const uint32_t *d_seg_size, uint32_t *d_seg_off, const uint8_t *head, uint32_t head_len,
                                  uint32_t bound, uint32_t trailer, uint8_t *d_dst, uint64_t dst_stride, uint32_t *d_out_size,
                                  int32_t *d_status)
{
    ZHead h = {};
    for (uint32_t i = 0; i < head_len && i < 16u; i++) h.b[i] = head[i];
    h.len = head_len;
    hipLaunchKernelGGL(k_zstd_seg_plan, dim3((uint32_t)n_blocks), dim3(64), 0, s, n_blocks, nseg, d_seg_size, d_seg_off, h, bound,
                       trailer, d_dst, dst_stride, d_out_size, d_status);
    hipLaunchKernelGGL(k_zstd_seg_copy, dim3((uint32_t)(n_blocks * nseg)), dim3(64), 0, s, n_blocks, nseg, d_seg,
                       zstd_seg_stride(seg_bytes), d_seg_size, d_seg_off, d_dst, dst_stride);
    return hipGetLastError();
}

} // namespace cryo
