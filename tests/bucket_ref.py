"""Reference of the bucketed group columns (include/cryo_codec.h, "Bucketed group columns"), in Python integers: the key of a
group value under a bucket, the descriptor rules of the bucket array, and the grouped call with the bucket step between the walk and the
grouping.  Written from the header's comment, not from the kernel.  Test infrastructure only.

A bucket is (kind, flags, origin, value): value a WIDTH bucket's width, a BOUNDS bucket's sequence of boundaries (any order,
duplicates allowed).  Python's // floors and its integers do not overflow, so the contract's arithmetic is stated as it reads."""
import bisect

import numpy as np

import float_ref as flr
import group_ref as gr
from filter_ref import INT2, INT4, INT8

NONE, WIDTH, BOUNDS = 0, 1, 2
INFINITE = 1
BOUNDS_MAX = 1024
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TYPE_BITS = {INT2: 16, INT4: 32, INT8: 64}
UNDECIDED = "undecided"
RAW = (NONE, 0, 0, 0)


def width(origin, w, flags=0):
    return (WIDTH, flags, origin, w)


def bounds(members, flags=0):
    return (BOUNDS, flags, 0, list(members))


def extremes(typ):
    bits = TYPE_BITS[typ]
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


def bucket_key(bucket, typ, v):
    """the key of the non-NULL value v of a group column of type typ, or UNDECIDED"""
    kind, flags, origin, value = bucket
    if kind == NONE:
        return v
    lo, hi = extremes(typ)
    if flags & INFINITE and v in (lo, hi):
        return v                                                          # -infinity and +infinity are their own buckets
    if kind == WIDTH:
        key = origin + value * ((v - origin) // value)
        if key < I64_MIN:
            return UNDECIDED
    else:
        members = sorted(set(value))
        at = bisect.bisect_right(members, v)
        if at == 0:
            return UNDECIDED
        key = members[at - 1]
    if flags & INFINITE and key in (lo, hi):
        return UNDECIDED
    return key


def buckets_ok(buckets, nby, rsv=None):
    """the rules of a bucket array: one entry per group column; rsv: the entries' reserved fields"""
    if buckets is None or len(buckets) != nby or any(rsv or ()):
        return False
    for kind, flags, origin, value in buckets:
        if flags & ~INFINITE:
            return False
        if kind == NONE:
            if flags or origin or value:
                return False
        elif kind == WIDTH:
            if not isinstance(value, int) or value < 1:
                return False
        elif kind == BOUNDS:
            if origin or value is None or not 1 <= len(value) <= BOUNDS_MAX:
                return False
        else:
            return False
    return True


def group_call(blocks, atts, keys, by, cols, buckets, truth=None):
    """(rows, records, cells of shape (groups, ncols), total) of a call, a multi-handle call included: blocks[i] a decoded block
    or None (a rejected stream).  The walk, the keys of every kind, the truth table and the cells are float_ref's (which is
    group_ref's on integer columns and plain keys); buckets[j] is applied to group column j of every match, and a match with an
    undecided key counts in n_bad instead of n_match and is in no group"""
    rows, recs, cells = np.zeros(len(blocks), gr.ROW), [], []
    for i, block in enumerate(blocks):
        (status, n, n_match, n_bad), matches = flr._reduce(block, atts, keys, list(by) + list(cols), truth)
        groups = {}
        for pos, m in matches:
            key = tuple(v if v is None else bucket_key(buckets[j], by[j][1], v) for j, v in enumerate(m[:len(by)]))
            if UNDECIDED in key:
                n_match, n_bad = n_match - 1, n_bad + 1
                continue
            g = groups.setdefault(key, [0, [[] for _ in cols]])
            g[0] += 1
            for j, v in enumerate(m[len(by):]):
                if v is not None:
                    g[1][j].append((pos, v))
        rows[i] = (status, n, n_match, n_bad, len(groups), 0, len(recs))
        for key in sorted(groups, key=gr.order_key):
            k = [0 if v is None else v for v in key] + [0] * (2 - len(key))
            recs.append((k, groups[key][0], sum(1 << j for j, v in enumerate(key) if v is None)))
            cells.append([flr.cell_of(v, cols[j][1], True) for j, v in enumerate(groups[key][1])])
    r = np.zeros(len(recs), gr.REC)
    c = np.zeros((len(recs), len(cols)), gr.CELL)
    for g, rec in enumerate(recs):
        r[g] = rec
        for j, cell in enumerate(cells[g]):
            c[g, j] = cell
    return rows, r, c, len(recs)
