/*
 * agg.hip -- the device side of the scan aggregate (cryo_codec_agg_batch / _blocks, include/cryo_codec.h: the rules).
 *
 * The host (cryo_codec.cpp, agg_pass) decodes a chunk of stored streams into handle workspace with the shared decode loop
 * (decode_pass); this kernel looks into every heap tuple of the decoded chunk as the scan filter does, and instead of packing the
 * tuples that pass the keys it reduces up to four of their integer columns, so that a row and a few cells per block leave the
 * device:
 *   k_agg_block   one wave per block, four blocks per workgroup: the sweep of scan_sweep.h, whose walk runs over the columns
 *                 1 .. max(highest key column, highest aggregate column) and notes the aggregate columns' values as it passes
 *                 them.  A descriptor with a byte-string key runs k_agg_block<true>, whose walk compares those too and counts an
 *                 undecided tuple in n_bad; every other descriptor runs k_agg_block<false>.  There is no OVERLAP verdict and
 *                 nothing to place, so one sweep suffices.  A lane keeps, per aggregate column, the running state of agg_cell.h.
 *                 After the sweep a butterfly (__shfl_xor) reduces the five words per column across the wave; lane 0 writes the
 *                 block's row and its cells straight to the call's output.
 * A descriptor with a float key or a float aggregate column runs agg_float.hip's k_aggf_block instead (ScanDesc::floats).
 * Every device write is a vector store in plain C++.  No LDS, no scratch, no atomics; no running totals, no second kernel.
 */
#include "kernels.h"
#include "agg_cell.h"
#include "scan_sweep.h"

namespace cryo {

template <bool BYTES>
__global__ void __launch_bounds__(256)
k_agg_block(const uint8_t *__restrict__ dec, uint64_t dec_stride, uint32_t B, uint32_t cnt, const int32_t *__restrict__ dec_status,
            const FilterAtt *__restrict__ atts, const FilterKey *__restrict__ keys, uint32_t nkeys,
            const AggCol *__restrict__ cols, uint32_t ncols, uint32_t max_att, uint4 *__restrict__ blocks,
            AggCell *__restrict__ cells)
{
    uint32_t k, lane;
    sweep_wave(4u, k, lane);
    if (k >= cnt) return;
    uint32_t n_match = 0, n_bad = 0;
    uint32_t cn[kAggMaxCols];
    int64_t cmin[kAggMaxCols], cmax[kAggMaxCols];
    uint64_t clo[kAggMaxCols], chi[kAggMaxCols];
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) { cn[j] = 0; cmin[j] = INT64_MAX; cmax[j] = INT64_MIN; clo[j] = 0; chi[j] = 0; }
    const uint8_t *__restrict__ p;
    uint32_t n, upper;
    uint32_t status = sweep_open(dec, dec_stride, B, dec_status, k, p, n, upper);
    if (status == 0u) {
        for (uint32_t t0 = 0; t0 < n; t0 += 64u) {
            WalkCapture cap;
            const SweepItem it = sweep_turn<true, kAggMaxCols, BYTES, false, false>(p, B, n, upper, t0 + lane, atts, keys, nkeys, max_att,
                                                                                   cols, ncols, &cap);
            n_match += (uint32_t)__popcll(__ballot(it.match));
            n_bad += (uint32_t)__popcll(__ballot(it.bad));
#pragma unroll
            for (uint32_t j = 0; j < kAggMaxCols; j++) /* a NULL adds nothing */
                if (it.match && ((cap.has >> j) & 1u) != 0) cell_add(cap.v[j], cn[j], cmin[j], cmax[j], clo[j], chi[j]);
        }
        /* said again for the compiler: a status that is a constant on every path here is not kept in a scalar register through
         * the sweep.  Without this line both instantiations need 79 scalar registers, with it 77 (the parent's 77 and 76) */
        status = 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < kAggMaxCols; j++) {
        if (j >= ncols) continue; /* uniform */
#pragma unroll
        for (uint32_t d = 32; d >= 1u; d >>= 1) cell_meet(d, cn[j], cmin[j], cmax[j], clo[j], chi[j]);
    }
    if (lane == 0) {
        blocks[k] = make_uint4(status, n, n_match, n_bad);
#pragma unroll
        for (uint32_t j = 0; j < kAggMaxCols; j++)
            if (j < ncols) cells[(uint64_t)k * ncols + j] = cell_int(cn[j], cmin[j], cmax[j], clo[j], chi[j]);
    }
}

hipError_t launch_agg(const ScanChunk &c, const ScanDesc &d, const AggLaunch &a)
{
    if (c.cnt == 0) return hipSuccess;
    if (!agg_launch_ok(c, d, a)) return hipErrorInvalidValue;
    switch (scan_route(d.truth, d.floats, d.like)) {
    case kRouteLike: return launch_aggl(c, d, a);  /* a pattern key: agg_float.hip's second unit */
    case kRouteFloat: return launch_aggf(c, d, a); /* a float key or a float aggregate column: agg_float.hip's kernel */
    case kRouteTable: return agg_launch(k_agg_block<true>, true, c, d, a);
    case kRoutePlain: return agg_launch(k_agg_block<false>, false, c, d, a);
    }
    return hipErrorInvalidValue;
}

} // namespace cryo
