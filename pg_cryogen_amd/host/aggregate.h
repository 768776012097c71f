/*
 * aggregate.h -- a sequential scan whose keys are tested and whose integer and float columns are reduced on the GPU, one partial aggregate
 * per block (include/cryo_codec.h, cryo_codec_agg_batch: the rules of a block, of a tuple, of a key and of a cell, and what is not
 * supported).
 *
 * SELECT sum(x), min(ts), max(ts), count(x) FROM t WHERE ts >= a AND ts < b through filter.h brings every matching tuple back
 * and leaves the adding up to the host.  The walk below reads the relation as cryo_filter_scan does -- sequential-scan order
 * (scan_iterator.h), chains reassembled with cryo_stage_read_chain, the readable ones batched by method in the filter's windows --
 * hands them to the codec's agg_blocks and gets back 16 bytes per block and 40 bytes per block and aggregate column.  It touches
 * neither the decompressed-block cache nor the device pool.
 *
 * Visibility stays with the caller, and the block is the unit that makes that exact: a cryo block is written by one transaction,
 * so every block's partial comes with its chain's created_xid (FrozenTransactionId for a frozen block) and the caller adds up the
 * blocks its snapshot sees.  The totals' combined cells are the answer for a relation whose blocks are all visible.
 *
 * Where it does not pay: one block per call (a device round trip per block), and aggregates this codec does not reduce (numeric
 * columns, expressions, stddev and variance) -- those go through filter.h.  GROUP BY on one or two integer columns is group.h's.
 *
 * Float columns (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8).  A float column's cell is a cryo_agg_cell_f in the cell's 40 bytes: n, min and
 * max in float8_cmp_internal's order, and the sum as a double-double pair (sum, err) whose reduction order the header fixes, so
 * that the bytes are reproducible.  Blocks and groups combine with cryo_agg_cell_f_combine below, in block order; the totals do
 * so for float columns.  The binder's part: sum(float8) is sum, or sum + err rounded once, which is sum; err is NaN exactly
 * when the finite values left the double range -- PostgreSQL raises "value out of range: overflow" there, and so should the
 * binder.  The result can differ in the last bits from PostgreSQL's own left-to-right float8pl, whose result already depends on
 * the plan under parallel aggregation; this one errs by at most 2^-90 of the sum of magnitudes.
 */
#ifndef CRYO_AGGREGATE_H
#define CRYO_AGGREGATE_H

#include <string.h>

#include "walk.h"
#include "cryo_codec.h"

/* one block's partial aggregate; cells: ncols cells in the order of the aggregate descriptor, valid during the callback only.
 * n_bad > 0: the block holds damaged items or -- under a byte-string key -- undecided ones, which are in no cell --
 * cryo_filter_scan lists them */
typedef struct {
    BlockNumber block;
    TransactionId created_xid;
    uint32 n_items, n_match, n_bad;
    const cryo_agg_cell *cells;
} CryoAggBlock;

/* reason: a block's status (CRYO_FETCH_STREAM, CRYO_FETCH_HEADER: detail 0) or one of check.h's host-side reasons
 * (CRYO_CHECK_CHAIN: detail = the CryoError of cryo_stage_read_chain; CRYO_CHECK_METHOD: detail = the method the first page
 * names) */
typedef CryoWalkReport CryoAggReport;

typedef struct {
    uint64 blocks;       /* chains examined (every page the walk took for a block start, bad ones included) */
    uint64 empty_pages;  /* new pages skipped, as a scan skips them */
    uint64 items;        /* items of the blocks the codec looked into */
    uint64 matches;      /* tuples that passed every key */
    uint64 bad;          /* bad items (CRYO_FETCH_ITEM, CRYO_FILTER_TUPLE) and undecided ones (CRYO_FILTER_UNDECIDED) */
    uint64 reports;      /* reports made */
    uint64 codec_calls;  /* agg_blocks calls */
    uint64 bytes_back;   /* what the calls brought back: rows and cells */
    /* the cells of all blocks with status 0 combined, whatever their xid: n and the 128-bit sums added (with carry), min and max
     * over the cells with n > 0 (0 when there is none); entries ncols .. 3 are zero.  A float column's entry is a
     * cryo_agg_cell_f, combined in block order by cryo_agg_cell_f_combine */
    cryo_agg_cell cells[CRYO_AGG_MAX_COLS];
} CryoAggTotals;

/* The float order's signed integer of a double (include/cryo_codec.h, "Float keys"): a NaN INT64_MAX, a zero 0 */
static inline int64_t cryo_float_order(double x)
{
    uint64_t b;
    memcpy(&b, &x, sizeof b);
    if ((b & UINT64_C(0x7FFFFFFFFFFFFFFF)) > UINT64_C(0x7FF0000000000000)) return INT64_MAX;
    if ((b & UINT64_C(0x7FFFFFFFFFFFFFFF)) == 0) return 0;
    return (int64_t)(b ^ ((b >> 63) ? UINT64_C(0x7FFFFFFFFFFFFFFF) : 0));
}

/* the canonical double of an order value: the NaN 0x7FF8000000000000, the zero +0 */
static inline double cryo_float_of_order(int64_t m)
{
    uint64_t b = m == INT64_MAX ? UINT64_C(0x7FF8000000000000) : (uint64_t)m ^ (m < 0 ? UINT64_C(0x7FFFFFFFFFFFFFFF) : 0);
    double x;
    memcpy(&x, &b, sizeof x);
    return x;
}

/* t = t combined with c, t the blocks (or groups) before c: the header's rule ("The reduction").  n adds; min and max in the
 * float order, canonical; "some value is +Inf / -Inf / NaN" is read off the cells' (sum, err) and folded first -- NaN, or both
 * infinities: (NaN, +0); one infinity: (that, +0) --, then a pair that left the double range, in either cell or in this step:
 * (NaN, NaN); otherwise (sum, err) = t (+) c.  Adds and subtracts in IEEE binary64 alone, every intermediate named (volatile:
 * the compiler keeps each rounding). */
static inline void cryo_agg_cell_f_combine(cryo_agg_cell_f *t, const cryo_agg_cell_f *c)
{
    const double inf = cryo_float_of_order(INT64_C(0x7FF0000000000000)), nan = cryo_float_of_order(INT64_MAX);
    int64_t lo, hi, a;
    int P, M, Q, V;
    if (c->n == 0) return;
    if (t->n == 0) { *t = *c; return; }
    lo = cryo_float_order(t->min);
    a = cryo_float_order(c->min);
    if (a < lo) lo = a;
    hi = cryo_float_order(t->max);
    a = cryo_float_order(c->max);
    if (a > hi) hi = a;
    t->n += c->n;
    t->min = cryo_float_of_order(lo);
    t->max = cryo_float_of_order(hi);
    V = t->err != t->err || c->err != c->err;
    Q = (t->err == t->err && t->sum != t->sum) || (c->err == c->err && c->sum != c->sum);
    P = t->sum == inf || c->sum == inf;
    M = t->sum == -inf || c->sum == -inf;
    if (Q || (P && M)) { t->sum = nan; t->err = 0.0; }
    else if (P || M) { t->sum = P ? inf : -inf; t->err = 0.0; }
    else if (V) { t->sum = nan; t->err = nan; }
    else {
        volatile double s = t->sum + c->sum;
        volatile double bb = s - t->sum;
        volatile double d1 = s - bb;
        volatile double e1 = t->sum - d1;
        volatile double e2 = c->sum - bb;
        volatile double e = e1 + e2;
        volatile double lows = t->err + c->err;
        volatile double u = e + lows;
        volatile double h = s + u;
        volatile double d2 = h - s;
        volatile double l = u - d2;
        if (h != h || l != l || h == inf || h == -inf || l == inf || l == -inf) { t->sum = nan; t->err = nan; }
        else { t->sum = h; t->err = l; }
    }
}

/* a window of the walk -- one codec call per method present -- is the filter's: at most this many chains, or this many
 * compressed bytes, whichever comes first */
#define CRYO_AGG_WINDOW_BLOCKS 4096
#define CRYO_AGG_WINDOW_BYTES ((Size)256 << 20)
#ifdef CRYO_HOST_TEST_HOOKS
void cryo_aggregate_set_window(int blocks, Size bytes); /* test builds only: lower the window; 0, 0 restores the constants */
#endif

/* Scans the relation (nblocks read once) with the descriptors *f and *agg (host arrays; include/cryo_codec.h).  Every block the
 * codec could look into (status 0) is handed to block_cb(arg, b) in block order.  Every block it could not (STREAM, HEADER) and
 * every chain that cannot be read is reported through report(arg, r) -- in the same order, between the blocks -- and the walk
 * goes on.  *totals (may be NULL) is filled on every return.  Returns CRYO_OK (0), CRYO_E_UNSUPPORTED when the bound codec has no
 * agg_blocks, CRYO_E_NODEV when no codec can be bound, CRYO_E_ARG (a null relation or descriptor; descriptors the codec refuses),
 * CRYO_E_NOMEM, or the codec's error (the walk stops there; what was delivered stands). */
int cryo_aggregate_scan(CryoRel *rel, const cryo_filter *f, const cryo_agg *agg,
                        void (*block_cb)(void *arg, const CryoAggBlock *b),
                        void (*report)(void *arg, const CryoAggReport *r), void *arg, CryoAggTotals *totals);

#endif
