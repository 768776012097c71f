"""Reference of the grouped scan's rules (include/cryo_codec.h, "grouping a scan"), in numpy and plain Python: what
cryo_codec_group_batch must report for decoded blocks, the filter's descriptor, one or two group columns and up to four aggregate
columns.  Written from the header's comment, not from the kernel.  Test infrastructure only.

The walk over a tuple is agg_ref's (every read goes through filter_ref.Tuple, which refuses any index outside [0, len)): the
group columns are walked and read exactly as aggregate columns are.  Sums are Python integers, split at the very end."""
import struct

import numpy as np

import agg_ref as ar
import filter_ref as fr
from filter_ref import HEADER, KEY_SIZE, OK, STREAM, TUPLE, maxalign

MAX_BY = 2
ROW = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"), ("n_groups", "<u4"), ("rsv", "<u4"),
                ("first_group", "<u8")])
REC = np.dtype([("key", "<i8", (2,)), ("n_rows", "<u4"), ("nulls", "<u4")])
CELL = ar.CELL


def _col_ok(atts, att, typ):
    if not 1 <= att <= len(atts) or typ not in KEY_SIZE:
        return False
    attlen, attalign = atts[att - 1]
    return attlen == KEY_SIZE[typ] and attalign >= attlen


def desc_ok(atts, keys, by, cols, flags=0, rsv=0, grp_rsv=0, by_rsv=None, agg_rsv=0, col_rsv=None, **kw):
    """the grouping's argument rules: atts [(attlen, attalign)], keys [(att, type, op, value)], by and cols [(att, type)];
    cols None: a null aggregate descriptor"""
    if not fr.desc_ok(atts, keys, flags, rsv, **kw) or flags != 0 or grp_rsv or any(by_rsv or ()):
        return False
    if not 1 <= len(by) <= MAX_BY or not all(_col_ok(atts, a, t) for a, t in by):
        return False
    if cols is None:
        return True
    if agg_rsv or len(cols) > ar.MAX_COLS or any(col_rsv or ()):
        return False
    return all(_col_ok(atts, a, t) for a, t in cols)


def order_key(key):
    """what a block's groups are sorted by: key a tuple of values, None for NULL; NULL after every value"""
    return tuple((1, 0) if v is None else (0, v) for v in key)


def group_block(block, atts, keys, by, cols):
    """((status, n_items, n_match, n_bad), [(key tuple with None for NULL, n_rows, [cell per aggregate column])] in the
    contract's order) of one decoded block, or of None (a rejected stream)"""
    if block is None:
        return (STREAM, 0, 0, 0), []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    B = b.size
    assert B % 8 == 0 and B >= 16
    lower, upper = (int(v) for v in b[:8].view("<u4"))
    n = (lower - 8) // 8
    if lower < 8 or (lower - 8) % 8 or n > fr.MAX_ITEMS or not lower <= upper <= B or (n == 0 and upper != B):
        return (HEADER, 0, 0, 0), []
    n_match = n_bad = 0
    groups = {}
    for pos in range(1, n + 1):
        off, ln = struct.unpack_from("<II", b, 8 + 8 * (pos - 1))
        if ln == 0 or off % 8 or off < upper or off + maxalign(ln) > B:
            n_bad += 1
            continue
        # the walk goes over the columns 1 .. max(key, group, aggregate column): the group columns ride as aggregate columns
        verdict, vals = ar.agg_tuple(b[off:off + ln].tobytes(), atts, keys, list(by) + list(cols))
        if verdict == TUPLE:
            n_bad += 1
        elif verdict == OK:
            n_match += 1
            g = groups.setdefault(tuple(vals[:len(by)]), [0, [[] for _ in cols]])
            g[0] += 1
            for j, v in enumerate(vals[len(by):]):
                if v is not None:
                    g[1][j].append(v)
    out = [(key, groups[key][0], [ar.cell_of(v) for v in groups[key][1]]) for key in sorted(groups, key=order_key)]
    return (OK, n, n_match, n_bad), out


def group_call(blocks, atts, keys, by, cols):
    """(rows, records, cells of shape (groups, ncols), total) of a call: blocks[i] a decoded block or None"""
    rows, recs, cells = np.zeros(len(blocks), ROW), [], []
    for i, block in enumerate(blocks):
        row, groups = group_block(block, atts, keys, by, cols)
        rows[i] = row + (len(groups), 0, len(recs))
        for key, n_rows, cs in groups:
            k = [0 if v is None else v for v in key] + [0] * (2 - len(key))
            recs.append((k, n_rows, sum(1 << j for j, v in enumerate(key) if v is None)))
            cells.append(cs)
    r = np.zeros(len(recs), REC)
    c = np.zeros((len(recs), len(cols)), CELL)
    for g, rec in enumerate(recs):
        r[g] = rec
        for j, cell in enumerate(cells[g]):
            c[g, j] = cell
    return rows, r, c, len(recs)


def combine_block(groups, j):
    """a block's cells of aggregate column j combined by agg_ref.combine's rule: (n, min, max, sum)"""
    cs = [g[2][j] for g in groups if g[2][j][0] > 0]
    return (sum(c[0] for c in cs), min((c[1] for c in cs), default=0), max((c[2] for c in cs), default=0),
            sum((c[4] << 64) + c[3] for c in cs))
