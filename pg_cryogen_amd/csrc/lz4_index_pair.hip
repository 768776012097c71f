/*
 * lz4_index_pair.hip -- the sequence index of a batch with ONE walker per block, built by pairs of waves.
 *
 * k_lz4_index (lz4_index.hip) walks 64 blocks per wave, one lane per block, and the same wave feeds the walkers' LDS
 * rings: with 39 KB of rings per wave a SIMD holds one wave, and a wave alone on its SIMD issues one vector instruction
 * every four cycles.  About a third of a turn's instructions are not the serial hop (position -> ring read -> token ->
 * next position) but the ring feed: the counted wait for the loads, the commits to the rings, the request exchange, the
 * address selects and the loads.  Here the two jobs are two waves of one workgroup on the SAME rings:
 *
 *   walker wave   lane = block, only the hop: the token state machine of k_lz4_index (second token per turn, the
 *                 255-run look-ahead, the rare states), the positions' line buffer and the 32-byte row lines.  Each turn
 *                 it reads its mailbox `filled` BEFORE the ring dwords (DS operations of one wave execute in issue
 *                 order) and publishes `pos` (bit 31: done) at the end of the hop.
 *   feeder wave   lane = block as well, for the bookkeeping (`requested`, `filled`, the chunks on their way: all owned
 *                 by the feeder); per turn it reads the published positions, decides which of the turn's 16 walkers
 *                 get a chunk by k_lz4_index's rule (a stale position is only conservative: positions only grow),
 *                 issues the turn's two loads, commits the chunks requested kIdxDist rounds earlier and then publishes
 *                 `filled` -- chunk first, `filled` second, from the same wave, a compiler fence between them.
 *
 * LDS per pair is what k_lz4_index uses per wave plus 512 bytes of mailboxes, so a SIMD holds two waves where it held one,
 * with about the same wave-instructions in total.  Nothing in the loop is a barrier: one behind the set-up, one in front of
 * the exit.  Rows, descriptors and workspace are exactly k_lz4_index's for logS == 0 (Lz4IndexLayout, seg[blk] = (0, count)).
 *
 * A walker that jumps past everything requested (a long literal run) is seen by the feeder as pos >= requested: it
 * restarts the window at the chunk of pos.  Chunks of the old window still on their way are committed where they were
 * headed and not counted: commits happen in the order of the requests, so every ring slot the walker may read after the
 * restart ([pos, filled) of the new window) has been rewritten by a chunk of the new window behind them.
 *
 * Every wait across the waves is bounded (kPairStarve, kPairIdle below); what a walker has not walked when it gives up
 * is a short row, which is legal: the decoder validates every entry and its general path decodes the rest.
 */
#include "lz_common.h"

namespace cryo {
namespace {

/* the geometry of k_lz4_index (lz4_index.hip has the reasoning): 512-byte rings fed 128 bytes at a time, two loads per
 * turn that serve eight walkers each, four turns per round, chunks committed kIdxDist rounds behind their request */
constexpr uint32_t kIdxDist = 2;
constexpr uint32_t kIdxLanes = 64, kIdxRing = 512;
constexpr uint32_t kIdxLpw = 8u;
constexpr uint32_t kIdxChunk = kIdxLpw * 16u;
constexpr uint32_t kIdxWpl = kIdxLanes / kIdxLpw;
constexpr uint32_t kIdxGroups = kIdxLanes / (2u * kIdxWpl);
constexpr uint32_t kIdxLine = 16u;
constexpr uint32_t kIdxStride = kIdxRing + 16u; /* bank skew between rings */

/* LDS of a pair: rings + a trash slot per lane, the position lines (two lines + a trash slot per lane), the mailboxes */
constexpr uint32_t kPairTrash = kIdxLanes * kIdxStride;
constexpr uint32_t kPairPos = kPairTrash + kIdxLanes * 16u;
constexpr uint32_t kPairPosStride = (2u * kIdxLine + 8u) * 2u; /* bytes per lane */
constexpr uint32_t kPairMbPos = kPairPos + kIdxLanes * kPairPosStride;
constexpr uint32_t kPairMbFilled = kPairMbPos + kIdxLanes * 4u;
constexpr uint32_t kPairLds = kPairMbFilled + kIdxLanes * 4u; /* 40 448 bytes: four pairs in a CU's 160 KiB */
static_assert(4u * kPairLds <= 163840u, "four pairs per compute unit");

/* The bounds of the two waits.
 * Walker: the longest legitimate wait for bytes is a restart of its window -- the feeder notices the jump within one of
 * its rounds (every walker is visited once per round), requests the chunk and commits it kIdxDist rounds later: at most
 * kIdxDist + 2 feeder rounds of four turns, each turn at most one wait for a load (a few microseconds under a full
 * batch's traffic): some tens of microseconds.  A starved walker's turn is at least ~300 cycles (60 instructions, one
 * issue per four cycles at best), so 65 536 consecutive turns without a byte are more than 8 ms: two orders of magnitude
 * above the legitimate case, and still far inside a test's time limit.
 * Feeder: it leaves when every walker has published `done`, or after kPairIdle consecutive rounds in which no walker's
 * published position moved and no chunk was requested; a walker's slowest legitimate turn (the rare states, a line
 * store that waits for memory) is microseconds, 65 536 feeder rounds are tens of milliseconds.  The walkers a feeder
 * leaves behind starve and end their rows by the first bound. */
constexpr uint32_t kPairStarve = 65536u;
constexpr uint32_t kPairIdle = 65536u;

__device__ inline uint32_t pair_bperm(uint32_t v, uint32_t src_lane)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane << 2), (int)v);
}
__device__ inline uint32_t mb_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void mb_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

#ifndef CRYO_IDX_PAIR_WG
#define CRYO_IDX_PAIR_WG 1 /* pairs per workgroup: 4 = 512 threads, waves w and w + 4 share a SIMD; 1 = 128 threads, four workgroups per CU */
#endif
#ifndef CRYO_IDX_PAIR_PRIO
#define CRYO_IDX_PAIR_PRIO 1 /* the walker wave runs at s_setprio 1 over its feeder */
#endif

} // namespace

template <uint32_t PAIRS, bool PRIO>
__global__ void __launch_bounds__(128 * PAIRS)
k_lz4_idx_pair(const uint8_t *__restrict__ src_base, const uint64_t *__restrict__ src_off,
               const uint32_t *__restrict__ src_size, const uint64_t n_blocks, uint16_t *__restrict__ tbl,
               const uint32_t cap, uint2 *__restrict__ seg, uint16_t *__restrict__ dummy_base)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_mem[PAIRS * kPairLds];
    const uint32_t wave = uni(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const bool feeder = wave >= PAIRS;
    const uint32_t pair = feeder ? wave - PAIRS : wave;
    uint8_t *const s_ring = s_mem + pair * kPairLds;
    uint32_t *const mb_pos = reinterpret_cast<uint32_t *>(s_ring + kPairMbPos);
    uint32_t *const mb_filled = reinterpret_cast<uint32_t *>(s_ring + kPairMbFilled);

    const uint64_t blk = ((uint64_t)blockIdx.x * PAIRS + pair) * kIdxLanes + lane;
    const bool owner = blk < n_blocks;
    /* stream of this lane's block in "virtual" positions, vp = delta + offset in the block: chunk addresses are whole
     * 128-byte lines */
    uint64_t aoff = src_off[0] & ~(uint64_t)127; /* a lane past the end of the batch re-reads block 0 */
    uint32_t delta = 0, vend = 0;
    if (owner) {
        const uint64_t o = src_off[blk];
        aoff = o & ~(uint64_t)127;
        delta = (uint32_t)(o & 127u);
        vend = delta + src_size[blk];
    }
    const bool start_done = !owner || vend == delta;
    if (!feeder) { /* the mailboxes' first values, in front of the barrier */
        mb_pos[lane] = delta | (start_done ? 0x80000000u : 0u);
        mb_filled[lane] = 0u;
    }
    __syncthreads();

    if (feeder) {
        /* ================= the feeder ================= */
        uint32_t requested = 0, filled = 0;      /* delta < 128: the window starts at the stream's first line */
        uint32_t outA = 0, outB = 0;             /* a chunk's size while a chunk of this lane's walker is on its way, per slot set */
        uint32_t lastp = delta;
        const uint32_t piece16 = (lane & (kIdxLpw - 1u)) * 16u;
        const uint32_t wil = lane / kIdxLpw;
#define PAIR_SRC(q) const uint64_t saoff##q = ((uint64_t)pair_bperm((uint32_t)(aoff >> 32), kIdxWpl * q + wil) << 32) | pair_bperm((uint32_t)aoff, kIdxWpl * q + wil); \
                    const uint32_t svend##q = pair_bperm(vend, kIdxWpl * q + wil);
        PAIR_SRC(0) PAIR_SRC(1) PAIR_SRC(2) PAIR_SRC(3)
        PAIR_SRC(4) PAIR_SRC(5) PAIR_SRC(6) PAIR_SRC(7)
#undef PAIR_SRC
        /* the chunks on their way: inline-assembly loads with hand-counted waits, as in k_lz4_index -- read-write slot
         * operands, a do-while loop, a fixed number of vector-memory operations per turn (two loads; the feeder stores
         * nothing to memory), a drain that names every slot.  A round issues 4 x 2 loads, so when a turn commits what
         * it requested kIdxDist rounds ago, 8 * kIdxDist - 2 younger loads may still be in flight. */
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        const uint32_t mytrash = kPairTrash + lane * 16u;
#define PAIR_SLOT(n) u32x4 fd##n = {0, 0, 0, 0}, fe##n = fd##n; uint32_t fa##n = mytrash, fb##n = fa##n;
        PAIR_SLOT(0) PAIR_SLOT(1) PAIR_SLOT(2) PAIR_SLOT(3)
        PAIR_SLOT(4) PAIR_SLOT(5) PAIR_SLOT(6) PAIR_SLOT(7)
#undef PAIR_SLOT
        uint32_t moved = 0; /* per round: a walker's position moved, or a chunk was requested */
        bool alldone = false;
        auto turn = [&](const uint32_t j, u32x4 &fd, u32x4 &fe, uint32_t &fa, uint32_t &fb, uint32_t &out128,
                        const uint64_t soff, const uint32_t sve, const uint64_t soff2, const uint32_t sve2) __attribute__((always_inline)) {
            const uint32_t grp = j % kIdxGroups;
            const bool myturn = lane / (2u * kIdxWpl) == grp;
            /* ---- commit, then publish: the bytes under `filled` are in the ring when a walker sees it ---- */
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(8 * kIdxDist - 2) : "memory");
            *reinterpret_cast<u32x4 *>(s_ring + fa) = fd;
            *reinterpret_cast<u32x4 *>(s_ring + fb) = fe;
            asm volatile("" ::: "memory");
            {
                const uint32_t got = myturn ? out128 : 0u;
                filled += got;
                out128 -= got;
            }
            /* ---- where the walkers stand ---- */
            const uint32_t pm = mb_load(mb_pos + lane);
            const uint32_t p = pm & 0x7fffffffu;
            const bool pdone = (pm >> 31) != 0u;
            moved |= p ^ lastp;
            lastp = p;
            /* a walker that jumped past everything requested: its window restarts at the chunk of its position (what is
             * on its way is not counted; see the head of the file) */
            const bool jump = !pdone & (p >= requested) & (p < vend);
            requested = jump ? p & ~(kIdxChunk - 1u) : requested;
            filled = jump ? requested : filled;
            outA = jump ? 0u : outA;
            outB = jump ? 0u : outB;
            mb_store(mb_filled + lane, filled);
            /* ---- request the next chunk of the turn's 16 walkers ---- */
            const bool want = myturn & !pdone & (requested < vend) & (p + (kIdxRing - kIdxChunk) >= requested);
            const uint32_t wi = want ? 1u : 0u;
            const uint32_t msg = requested | wi;
            requested += wi * kIdxChunk;
            out128 |= wi * kIdxChunk;
            moved |= wi;
            const uint32_t s1 = 2u * kIdxWpl * grp + wil, s2 = s1 + kIdxWpl;
            const uint32_t m1 = pair_bperm(msg, s1), m2 = pair_bperm(msg, s2);
            const uint32_t o1 = (m1 & ~1u) + piece16, o2 = (m2 & ~1u) + piece16;
            const bool p1 = (m1 & 1u) != 0u, p2 = (m2 & 1u) != 0u;
            fa = p1 ? s1 * kIdxStride + (o1 & (kIdxRing - 1u)) : mytrash;
            fb = p2 ? s2 * kIdxStride + (o2 & (kIdxRing - 1u)) : mytrash;
            /* always two loads per turn: a lane with nothing to fetch re-reads its stream's first 16 bytes */
            const uint8_t *g1 = src_base + (soff + ((p1 & (o1 < sve)) ? o1 : 0u));
            const uint8_t *g2 = src_base + (soff2 + ((p2 & (o2 < sve2)) ? o2 : 0u));
            asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(fd) : "v"(g1));
            asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(fe) : "v"(g2));
            if (j == kIdxGroups - 1u) alldone = wave_all(pdone);
        };
#define PAIR_TURN(j, n, o, sa, sb) turn(j, fd##n, fe##n, fa##n, fb##n, o, saoff##sa, svend##sa, saoff##sb, svend##sb);
#define PAIR_ROUND(a, b, c, d, o) PAIR_TURN(0, a, o, 0, 1) PAIR_TURN(1, b, o, 2, 3) PAIR_TURN(2, c, o, 4, 5) PAIR_TURN(3, d, o, 6, 7)
        uint32_t idle = 0;
#ifdef CRYO_IDX_PROF
        const unsigned long long t_f0 = __builtin_amdgcn_s_memtime();
        uint32_t prof_rounds = 0;
#endif
        if (!wave_all(start_done)) {
            do {
                PAIR_ROUND(0, 1, 2, 3, outA)
                PAIR_ROUND(4, 5, 6, 7, outB)
#ifdef CRYO_IDX_PROF
                prof_rounds += 2u;
#endif
                idle = wave_any(moved != 0u) ? 0u : idle + 2u;
                moved = 0;
            } while (!alldone && idle < kPairIdle);
        }
#undef PAIR_ROUND
#undef PAIR_TURN
#ifdef CRYO_IDX_PROF
        if ((blockIdx.x & 255u) == 0u && lane == 0u)
            printf("[pair] feeder %u.%u: %u rounds, %llu ticks\n", blockIdx.x, pair, prof_rounds, __builtin_amdgcn_s_memtime() - t_f0);
#endif
        /* (nothing the compiler generates behind the loop may meet a load still in flight, and the slots' registers are
         * not its to hand out before that) */
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(fd0), "+v"(fe0), "+v"(fd1), "+v"(fe1), "+v"(fd2), "+v"(fe2), "+v"(fd3), "+v"(fe3),
                                            "+v"(fd4), "+v"(fe4), "+v"(fd5), "+v"(fe5), "+v"(fd6), "+v"(fe6), "+v"(fd7), "+v"(fe7) : : "memory");
    } else {
        /* ================= the walker ================= */
        if (PRIO) __builtin_amdgcn_s_setprio(1);
        uint16_t *const row = tbl + blk * cap;
        uint16_t *const dummy = dummy_base + lane * 16u; /* 32 bytes per lane behind the rows: where a lane with nothing to store stores */
        const uint32_t kcap = cap;
        const uint32_t rb = lane * kIdxStride;
        uint32_t pos = delta, state = 0, acc = 0, tm = 0; /* 0 token, 1 literal-length extension, 2 match-length extension */
        uint32_t k = 0, ls = 0;                           /* positions recorded; 16-entry lines of them stored */
        uint32_t starved = 0;
        uint16_t *const pbuf = reinterpret_cast<uint16_t *>(s_ring + kPairPos + lane * kPairPosStride);
        uint16_t *const ptrash = pbuf + 2u * kIdxLine;
        bool done = start_done;
#ifdef CRYO_IDX_PROF
        uint32_t prof_dry = 0, prof_live = 0, prof_turns = 0;
        const unsigned long long t_w0 = __builtin_amdgcn_s_memtime();
#endif
        auto turn = [&]() __attribute__((always_inline)) {
            /* `filled` first, the ring behind it: what lies under the value read is in the ring */
            const uint32_t filled = mb_load(mb_filled + lane);
            asm volatile("" ::: "memory");
            const uint32_t w0 = *reinterpret_cast<const uint32_t *>(s_ring + rb + (pos & (kIdxRing - 4u)));
            const uint32_t w1 = *reinterpret_cast<const uint32_t *>(s_ring + rb + ((pos + 4u) & (kIdxRing - 4u)));
            const uint32_t w2 = *reinterpret_cast<const uint32_t *>(s_ring + rb + ((pos + 8u) & (kIdxRing - 4u)));
            /* ---- one hop, branch-free for the two common states: k_lz4_index's, evaluated eagerly as there ---- */
            const bool live = !done & (pos < vend);
            const bool canread = (pos + 8u <= filled) | (filled >= vend);
            const uint32_t x = __builtin_amdgcn_alignbyte(w1, w0, pos & 3u);
            const bool go = live & canread;
            starved = (live & !canread) ? starved + 1u : 0u;
#ifdef CRYO_IDX_PROF
            prof_dry += (live & !canread) ? 1u : 0u;
            prof_live += live ? 1u : 0u;
#endif
            const uint32_t ll = (x >> 4) & 15u, e1 = (x >> 8) & 255u, tmn = x & 15u;
            const bool l15 = ll == 15u;
            const uint32_t q2 = pos + 3u + ll + (l15 ? e1 + 1u : 0u); /* behind the literals and the offset */
            const bool tok = go & (state == 0u);
            const bool rare = tok & ((l15 & (e1 == 255u)) | (q2 > vend));
            const bool plain = tok & !rare;
            const uint32_t nx = ~x;
            const uint32_t n = nx ? (uint32_t)__builtin_ctz(nx) >> 3 : 4u; /* leading 0xFF bytes */
            const bool extb = go & (state == 2u);
            *(tok ? pbuf + (k & (2u * kIdxLine - 1u)) : ptrash) = (uint16_t)(pos - delta);
            k += tok ? 1u : 0u;
            tm = tok ? tmn : tm;
            const uint32_t st_tok = tmn == 15u ? 2u : 0u;
            uint32_t npos = plain ? q2 : pos, nstate = plain ? st_tok : state;
            { /* a second token in the same turn when the first one leaves it inside the eight bytes just read */
                const bool dbl = plain & !l15 & (tmn != 15u) & (ll <= 2u) & (q2 < vend) & (k < kcap);
                const uint32_t x1 = __builtin_amdgcn_alignbyte(w2, w1, pos & 3u);
                const unsigned long long xx = ((unsigned long long)x1 << 32) | x;
                const uint32_t y = (uint32_t)(xx >> (8u * (3u + ll)));
                const uint32_t llb = (y >> 4) & 15u, e1b = (y >> 8) & 255u, tmb = y & 15u;
                const bool l15b = llb == 15u;
                const uint32_t q2b = q2 + 3u + llb + (l15b ? e1b + 1u : 0u);
                const bool rec2 = dbl & !(l15b & (e1b == 255u));
                *(rec2 ? pbuf + (k & (2u * kIdxLine - 1u)) : ptrash) = (uint16_t)(q2 - delta);
                k += rec2 ? 1u : 0u;
                tm = rec2 ? tmb : tm;
                const bool last2 = rec2 & (q2b > vend); /* the second token is the stream's last sequence */
                const bool adv2 = rec2 & !last2;
                npos = adv2 ? q2b : npos;
                nstate = adv2 ? (tmb == 15u ? 2u : 0u) : nstate;
                done = done | last2;
            }
            npos = extb ? pos + (n == 4u ? 4u : n + 1u) : npos;
            nstate = extb ? (n == 4u ? 2u : 0u) : nstate;
            done = done | !live | (k >= kcap) | (starved >= kPairStarve);
            pos = npos;
            state = nstate;
            { /* a long match-length run: up to seven more dwords of the ring while they are all 255 */
                const bool longm = extb & (n == 4u) & !done;
                if (__builtin_expect(wave_any(longm), 0)) {
                    const uint32_t a0 = pos & ~3u;
                    uint32_t m = 0;
                    bool run = longm;
#pragma unroll
                    for (uint32_t kq = 0; kq < 7u; kq++) {
                        const uint32_t dq = *reinterpret_cast<const uint32_t *>(s_ring + rb + ((a0 + 4u * kq) & (kIdxRing - 4u)));
                        run = run & (dq == 0xffffffffu) & (a0 + 4u * kq + 4u <= filled);
                        m += run ? 1u : 0u;
                    }
                    const uint32_t far = a0 + 4u * m;
                    pos = (longm & (far > pos)) ? far : pos;
                }
            }
            /* rare: a literal length that goes on behind its first extension byte, the stream's last sequence */
            const bool slow = rare | (!done & (state == 1u));
            if (__builtin_expect(wave_any(slow), 0)) {
                if (rare) {
                    if (l15 && e1 == 255u) { state = 1u; acc = 15u + 255u; pos += 2u; }
                    else done = true; /* q2 > vend: last sequence */
                } else if (slow && pos < vend && live && canread) {
                    if (n == 4u) { acc += 1020u; pos += 4u; if (acc >= vend) done = true; }
                    else {
                        acc += 255u * n + ((x >> (8u * n)) & 255u);
                        const uint32_t q = pos + n + 1u + acc;
                        if (acc >= vend || q + 2u > vend) done = true;
                        else { pos = q + 2u; state = tm == 15u ? 2u : 0u; }
                    }
                }
            }
            mb_store(mb_pos + lane, pos | (done ? 0x80000000u : 0u));
        };
        /* positions go out in whole 32-byte lines of 16, each line stored once, when it is complete; one unconditional
         * pair of stores per four turns (a lane gains at most eight positions in four turns) */
#define PAIR_LINE_COPY(ps_, pd_)                                                                 \
        {                                                                                        \
            const uint4 v0_ = *reinterpret_cast<const uint4 *>(ps_);                             \
            const uint4 v1_ = *reinterpret_cast<const uint4 *>((ps_) + 8);                       \
            store16_out<false>(reinterpret_cast<uint8_t *>(pd_), v0_);                           \
            store16_out<false>(reinterpret_cast<uint8_t *>((pd_) + 8), v1_);                     \
        }
#define PAIR_PUT()                                                                               \
        {                                                                                        \
            const bool st_ = ls < k / kIdxLine;                                                  \
            const uint16_t *ps_ = pbuf + (ls & 1u) * kIdxLine;                                   \
            uint16_t *pd_ = st_ ? row + ls * kIdxLine : dummy;                                   \
            PAIR_LINE_COPY(ps_, pd_)                                                             \
            if (st_) ls++;                                                                       \
        }
        if (wave_any(!done)) {
            do {
                PAIR_PUT()
                turn(); turn(); turn(); turn();
#ifdef CRYO_IDX_PROF
                prof_turns += 4u;
#endif
            } while (wave_any(!done));
        }
#ifdef CRYO_IDX_PROF
        if ((blockIdx.x & 255u) == 0u && lane < 2u)
            printf("[pair] walker %u.%u lane %u: %u turns, live %u, dry %u, %llu ticks, k %u\n", blockIdx.x, pair, lane, prof_turns, prof_live, prof_dry,
                   __builtin_amdgcn_s_memtime() - t_w0, k);
#endif
        if (owner) { /* what is left: at most one complete line and the one being filled (stored whole) */
            PAIR_PUT()
            PAIR_PUT()
            if ((k & (kIdxLine - 1u)) != 0u && ls == k / kIdxLine) {
                const uint16_t *ps_ = pbuf + (ls & 1u) * kIdxLine;
                uint16_t *pd_ = row + ls * kIdxLine;
                PAIR_LINE_COPY(ps_, pd_)
            }
            seg[blk] = make_uint2(0u, k);
        }
#undef PAIR_PUT
#undef PAIR_LINE_COPY
        if (PRIO) __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
}

hipError_t launch_lz4_index_pair(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                                 uint64_t n_blocks, uint32_t block_size, void *d_workspace, const Lz4IndexLayout &L)
{
    (void)block_size;
    if (n_blocks == 0) return hipSuccess;
    if (L.logS != 0u) return hipErrorInvalidValue; /* one walker per block only */
    constexpr uint32_t kWg = CRYO_IDX_PAIR_WG;
    const uint64_t grid = (n_blocks + kIdxLanes * kWg - 1) / (kIdxLanes * kWg);
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    uint8_t *ws = static_cast<uint8_t *>(d_workspace);
    hipLaunchKernelGGL((k_lz4_idx_pair<kWg, CRYO_IDX_PAIR_PRIO != 0>), dim3((uint32_t)grid), dim3(128u * kWg), 0, s, d_src, d_src_off,
                       d_src_size, n_blocks, reinterpret_cast<uint16_t *>(ws), L.cap, reinterpret_cast<uint2 *>(ws + L.seg_off),
                       reinterpret_cast<uint16_t *>(ws + L.dummy_off));
    return hipGetLastError();
}

hipError_t launch_lz4_index_form(hipStream_t s, const uint8_t *d_src, const uint64_t *d_src_off, const uint32_t *d_src_size,
                                 uint64_t n_blocks, uint32_t block_size, void *d_workspace, const Lz4IndexLayout &L, int form, int cus)
{
    if (lz4_index_use_pair(L, form, n_blocks, cus)) return launch_lz4_index_pair(s, d_src, d_src_off, d_src_size, n_blocks, block_size, d_workspace, L);
    return launch_lz4_index(s, d_src, d_src_off, d_src_size, n_blocks, block_size, d_workspace, L);
}

__global__ void __launch_bounds__(256)
k_lz4_idx_counts(const uint2 *__restrict__ seg, const uint64_t n_blocks, uint32_t *__restrict__ counts)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n_blocks) counts[i] = seg[i].y;
}
hipError_t launch_lz4_index_counts(hipStream_t s, const void *d_workspace, const Lz4IndexLayout &L, uint64_t n_blocks, uint32_t *d_counts)
{
    if (n_blocks == 0) return hipSuccess;
    if (L.logS != 0u || (n_blocks + 255u) / 256u > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lz4_idx_counts, dim3((uint32_t)((n_blocks + 255u) / 256u)), dim3(256), 0, s,
                       reinterpret_cast<const uint2 *>(static_cast<const uint8_t *>(d_workspace) + L.seg_off), n_blocks, d_counts);
    return hipGetLastError();
}

} // namespace cryo
