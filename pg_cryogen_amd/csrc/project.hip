/*
 * project.hip -- the device side of the projecting scan (cryo_codec_project_batch / _blocks, include/cryo_codec.h: the rules).
 *
 * The host (cryo_codec.cpp, project_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); these kernels look into every heap tuple of the decoded chunk as the scan aggregate does, and of every tuple that
 * passes the keys only the named fixed-width columns leave the device, as one row of 8 .. 64 bytes, with an 8-byte record:
 *   k_project_block    one wave per block, four blocks per workgroup: the sweep of scan_sweep.h, whose walk runs over the columns
 *                      1 .. max(highest key column, highest projected column) with eight capture slots.  The
 *                      wave ballots the matches and the bad items of the turn; a lane's rank among both is its record's place, its
 *                      rank among the matches its row's.  A matching lane assembles its row in registers -- the column table
 *                      (width and offset per column, the host's) is wave-uniform, so the word a column lands
 *                      in is a scalar compare, and NULL columns and pads are the zeros the words start with -- and writes it as
 *                      whole 8-byte words, with its record, to the block's share of a side area in handle workspace.  There is
 *                      no OVERLAP verdict: a block places at most 290 rows whatever it holds, so nothing about the block has to
 *                      be known before its first row is written and ONE sweep suffices (the filter needs two).  A descriptor with
 *                      a byte-string key runs k_project_block<true>, whose walk compares those
 *                      too and gives an undecided tuple a record and no row; every other descriptor runs k_project_block<false>.
 *                      A descriptor with a float key (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8) runs k_projectf_block, the same body
 *                      with the walk's FLOATS parameter set.
 *   k_project_offsets  one workgroup per chunk: the tiled scan of heap_block.h (offsets_tile<2>) over rows and records at once,
 *                      from the two running totals the chunk before left in device memory; it writes rec_first and row_first.
 *   k_project_copy     a grid stride over the blocks: block k's rows and records from the side area to row_first / rec_first of
 *                      the call's output, 8 bytes per access (row_bytes is a multiple of 8), cut off at row_cap and rec_cap.
 * Every device write is a vector store in plain C++.  No LDS beyond the scan's eight words, no scratch, no global atomics.
 */
#include "kernels.h"
#include "scan_sweep.h"

namespace cryo {

constexpr uint32_t kProjectMaxCols = 8u; /* CRYO_PROJECT_MAX_COLS */

/* The staged column table: entry j is an AggCol to the walk (which reads att alone) and carries in `type` the column's width
 * w_j (1, 2, 4, 8) and in `rsv` its offset o_j within the row (0 .. 56, a multiple of w_j): ProjectLaunch's rule (kernels.h) */

/* the body of k_project_block, of k_projectf_block, the kernel of descriptors with a float key, and of k_projectl_block, the
 * kernel of descriptors with a pattern key */
template <bool BYTES, bool FLOATS, bool LIKE = false>
__device__ inline void project_block_body(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt,
                                          const int32_t *__restrict__ dec_status, const FilterAtt *__restrict__ atts,
                                          const FilterKey *__restrict__ keys, uint32_t nkeys, const AggCol *__restrict__ cols,
                                          uint32_t ncols, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
                                          uint4 *__restrict__ blocks, uint2 *__restrict__ side_rec, uint2 *__restrict__ side_rows)
{
    uint32_t k, lane;
    sweep_wave(4u, k, lane);
    if (k >= cnt) return;
    const unsigned long long below = (1ull << lane) - 1ull;
    const uint32_t col_mask = (1u << ncols) - 1u; /* ncols <= 8 */
    uint32_t n_match = 0, n_bad = 0;
    const uint8_t *__restrict__ p;
    uint32_t n, upper; /* lower <= B: n <= side_stride */
    const uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    uint2 *out_rec = side_rec + (uint64_t)k * side_stride;
    uint2 *out_rows = side_rows + (uint64_t)k * side_stride * row_words;
    for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
        const uint32_t i = t0 + lane;
        WalkCaptureN<kProjectMaxCols> cap;
        const SweepItem it = sweep_turn<true, kProjectMaxCols, BYTES, true, FLOATS, false, LIKE>(p, B, n, upper, i, atts, keys, nkeys,
                                                                                                  max_att, cols, ncols, &cap);
        const unsigned long long mm = __ballot(it.match), mb = __ballot(it.bad);
        if (it.match || it.bad) { /* records in position order: the rank among the matches and the bad items */
            const uint32_t r = n_match + n_bad + (uint32_t)__popcll((mm | mb) & below); /* below n <= side_stride */
            out_rec[r] = make_uint2((i + 1u) | (it.match ? 0u : it.verdict << 16), it.match ? ~cap.has & col_mask : 0u);
        }
        if (it.match) {
            /* the row in registers: a captured value is sign-extended and 0 when NULL, so its low w_j bytes are the
             * column's and shifting them to o_j touches no other column (o_j is a multiple of w_j: no word is crossed) */
            uint64_t word[kProjectMaxCols];
#pragma unroll
            for (uint32_t q = 0; q < kProjectMaxCols; q++) word[q] = 0;
#pragma unroll
            for (uint32_t j = 0; j < kProjectMaxCols; j++) {
                if (j >= ncols) continue; /* uniform */
                const AggCol c = cols[j];  /* uniform */
                const uint32_t w = c.type, o = c.rsv;
                const uint64_t bits = w >= 8u ? (uint64_t)cap.v[j] : (uint64_t)cap.v[j] & ((1ull << (8u * w)) - 1ull);
                const uint64_t placed = bits << (8u * (o & 7u));
#pragma unroll
                for (uint32_t q = 0; q < kProjectMaxCols; q++)
                    if ((o >> 3) == q) word[q] |= placed; /* uniform: the register is picked by a scalar compare */
            }
            const uint32_t r = n_match + (uint32_t)__popcll(mm & below); /* below n <= side_stride */
            uint2 *row = out_rows + (uint64_t)r * row_words;
            if (BYTES) {
                /* with BYTES the walk leaves no scalar registers for eight loop-invariant compares q < row_words kept
                 * as lane masks across the item loop (the compiler spilled eleven of them to vector lanes): one scalar
                 * branch on the row's length, 1 .. 8 words, and the stores from the last word down */
#define CRYO_ROW_WORD(q) row[q] = make_uint2((uint32_t)word[q], (uint32_t)(word[q] >> 32))
                switch (row_words) {
                case 0: break;
                default: CRYO_ROW_WORD(7); [[fallthrough]];
                case 7: CRYO_ROW_WORD(6); [[fallthrough]];
                case 6: CRYO_ROW_WORD(5); [[fallthrough]];
                case 5: CRYO_ROW_WORD(4); [[fallthrough]];
                case 4: CRYO_ROW_WORD(3); [[fallthrough]];
                case 3: CRYO_ROW_WORD(2); [[fallthrough]];
                case 2: CRYO_ROW_WORD(1); [[fallthrough]];
                case 1: CRYO_ROW_WORD(0);
                }
#undef CRYO_ROW_WORD
            } else {
#pragma unroll
                for (uint32_t q = 0; q < kProjectMaxCols; q++)
                    if (q < row_words) row[q] = make_uint2((uint32_t)word[q], (uint32_t)(word[q] >> 32));
            }
        }
        n_match += (uint32_t)__popcll(mm);
        n_bad += (uint32_t)__popcll(mb);
    }
    if (lane == 0) {
        blocks[2u * k] = make_uint4(status, n, n_match, n_bad);
        blocks[2u * k + 1u] = make_uint4(0u, 0u, 0u, 0u); /* rec_first, row_first: k_project_offsets */
    }
}

#ifndef CRYO_LIKE_UNIT
template <bool BYTES>
__global__ void __launch_bounds__(256)
k_project_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
                const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
                uint4 *__restrict__ blocks, uint2 *__restrict__ side_rec, uint2 *__restrict__ side_rows)
{
    project_block_body<BYTES, false>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, cols, ncols, max_att, row_words, side_stride,
                                     blocks, side_rec, side_rows);
}

/* k_project_block<true> whose walk also maps the columns of float keys; a projected float column comes back bit for bit */
__global__ void __launch_bounds__(256)
k_projectf_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
                 const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                 const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
                 uint4 *__restrict__ blocks, uint2 *__restrict__ side_rec, uint2 *__restrict__ side_rows)
{
    project_block_body<true, true>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, cols, ncols, max_att, row_words, side_stride,
                                   blocks, side_rec, side_rows);
}

/* rec_first and row_first of every row of the chunk: the records and the rows before block k, counted from the call's start;
 * running[0], running[1]: the rows and the records before the chunk in, after it out */
__global__ void __launch_bounds__(256)
k_project_offsets(uint32_t cnt, uint64_t *__restrict__ running, uint4 *__restrict__ blocks)
{
    __shared__ uint64_t wave_sum[8];
    uint64_t run_rows = running[0], run_recs = running[1]; /* the same in every thread; written again only after the tiles' barriers */
    for (uint32_t t = 0; t < cnt; t += 256u) {
        const uint32_t k = t + threadIdx.x;
        uint4 b = make_uint4(0u, 0u, 0u, 0u);
        if (k < cnt) b = blocks[2u * k];
        const uint64_t a[2] = {b.z, (uint64_t)b.z + b.w}; /* rows, records */
        uint64_t before[2], tile[2];
        offsets_tile(a, wave_sum, before, tile);
        if (k < cnt) {
            const uint64_t row_first = run_rows + before[0], rec_first = run_recs + before[1];
            blocks[2u * k + 1u] = make_uint4((uint32_t)rec_first, (uint32_t)(rec_first >> 32), (uint32_t)row_first, (uint32_t)(row_first >> 32));
        }
        run_rows += tile[0];
        run_recs += tile[1];
    }
    if (threadIdx.x == 0) {
        running[0] = run_rows;
        running[1] = run_recs;
    }
}

/* rows (row_words words each) and records (one word each) of the chunk's blocks from the side area to their places within the
 * call */
__global__ void __launch_bounds__(256)
k_project_copy(uint32_t cnt, uint32_t side_stride, uint32_t row_words, const uint4 *__restrict__ blocks,
               const uint2 *__restrict__ side_rec, const uint2 *__restrict__ side_rows, uint2 *__restrict__ rec, uint64_t rec_cap,
               uint2 *__restrict__ rows, uint64_t row_cap)
{
    for (uint32_t k = blockIdx.x; k < cnt; k += gridDim.x) {
        const uint4 head = blocks[2u * k], place = blocks[2u * k + 1u];
        const uint64_t rec_first = (uint64_t)place.x | (uint64_t)place.y << 32, row_first = (uint64_t)place.z | (uint64_t)place.w << 32;
        uint32_t nrow = head.z < side_stride ? head.z : side_stride;
        uint32_t nrec = head.z + head.w < side_stride ? head.z + head.w : side_stride; /* n_match + n_bad <= n_items <= side_stride */
        /* nothing at or beyond the caps */
        if (rec_first >= rec_cap) nrec = 0;
        else if (rec_cap - rec_first < nrec) nrec = (uint32_t)(rec_cap - rec_first);
        if (row_first >= row_cap) nrow = 0;
        else if (row_cap - row_first < nrow) nrow = (uint32_t)(row_cap - row_first);
        const uint2 *sr = side_rec + (uint64_t)k * side_stride;
        for (uint32_t w = threadIdx.x; w < nrec; w += 256u) rec[rec_first + w] = sr[w];
        const uint2 *sw = side_rows + (uint64_t)k * side_stride * row_words;
        for (uint32_t w = threadIdx.x; w < nrow * row_words; w += 256u) rows[row_first * row_words + w] = sw[w];
    }
}

static_assert(kProjectMaxCols == CRYO_PROJECT_MAX_COLS, "project_launch_ok's limit (kernels.h) is the kernels'");

hipError_t launch_project(const ScanChunk &c, const ScanDesc &d, const ProjectLaunch &p)
{
    if (c.cnt == 0) return hipSuccess;
    if (!project_launch_ok(c, d, p)) return hipErrorInvalidValue;
    hipError_t e = hipErrorInvalidValue;
    switch (scan_route(d.truth, d.floats, d.like)) {
    case kRouteLike: e = launch_projectl_block(c, d, p); break; /* a pattern key: the kernel of this source's second unit */
    case kRouteFloat: e = project_launch(k_projectf_block, true, c, d, p); break;
    case kRouteTable: e = project_launch(k_project_block<true>, true, c, d, p); break;
    case kRoutePlain: e = project_launch(k_project_block<false>, false, c, d, p); break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_project_offsets, dim3(1), dim3(256), 0, c.stream, c.cnt, p.d_running, p.d_blocks);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_project_copy, dim3(scan_copy_grid(c.cus, c.cnt)), dim3(256), 0, c.stream, c.cnt, filter_side_stride(c.block_size),
                       p.row_bytes / 8u, (const uint4 *)p.d_blocks, (const uint2 *)p.d_side_rec, (const uint2 *)p.d_side_rows, (uint2 *)p.d_rec,
                       p.rec_cap, (uint2 *)p.d_rows, p.row_cap);
    return hipGetLastError();
}

#else /* CRYO_LIKE_UNIT */
/* k_projectf_block whose walk also matches the patterns of CRYO_OP_LIKE / CRYO_OP_NOT_LIKE keys (walk_like): a kernel of its own
 * name, as k_filterl_match is -- inlined into k_project_block<true> and k_projectf_block the matcher would take them from eight
 * waves per SIMD to seven --, built from this source compiled a second time with CRYO_LIKE_UNIT (project_like.o) */
__global__ void __launch_bounds__(256)
k_projectl_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
                 const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
                 const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint32_t row_words, uint32_t side_stride,
                 uint4 *__restrict__ blocks, uint2 *__restrict__ side_rec, uint2 *__restrict__ side_rows)
{
    project_block_body<true, true, true>(dec, dec_stride, B, cnt, dec_status, atts, keys, nkeys, cols, ncols, max_att, row_words,
                                         side_stride, blocks, side_rec, side_rows);
}

hipError_t launch_projectl_block(const ScanChunk &c, const ScanDesc &d, const ProjectLaunch &p)
{
    return project_launch(k_projectl_block, true, c, d, p);
}
#endif

} // namespace cryo
