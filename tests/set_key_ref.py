"""Reference of the set scan keys (include/cryo_codec.h, "filtering a scan": "Set keys"), in numpy and plain Python: what the
filter, the aggregate, the grouped scan and the projection must report when a key's op is CRYO_OP_IN or CRYO_OP_NOT_IN.  Written
from the header's comment, not from the kernel.  Test infrastructure only.

A key is (att, type, op, value) as in filter_ref and bytes_key_ref; the value of a set key is a list of Python integers, in any
order, with repeats, of any size -- a member outside the range of the key's type equals no value.  The walk, the loads and the
byte-string keys are bytes_key_ref's; the block, call and multi-handle layers restate bytes_key_ref's and project_ref's over
this module's verdict."""
import numpy as np

import agg_ref as ar
import bytes_key_ref as br
import filter_ref as fr
import group_ref as gr
import multi_ref
import project_ref as pr
from bytes_key_ref import (BYTES, BYTES_MAX, COUNT_ONLY, EQ, GE, GT, HEADER, INT2, INT4, INT8, ISNULL, ITEM, KEY_SIZE, LE, LT,  # noqa: F401
                           MAX_ITEMS, NE, NOMATCH, NOTNULL, OK, OVERLAP, STREAM, TUPLE, UNDECIDED, decode, maxalign)

IN, NOT_IN = 9, 10
SET_MAX = 1024


def is_set_key(key):
    return key[2] in (IN, NOT_IN)


def desc_ok(atts, keys, flags=0, rsv=0, key_rsv=None):
    """the descriptor's argument rules with set keys.  key_rsv: the rsv field of each key as the caller set it (None: for a set
    key whose value is a list its length, else what bytes_key_ref takes); a set key whose value is None stands for a null
    address, and one whose value is an integer for a key made as a comparison is (rsv 0)"""
    if len(keys) > fr.MAX_KEYS:
        return False
    others, other_rsv = [], []
    for i, key in enumerate(keys):
        att, typ, op, value = key
        if not is_set_key(key):
            others.append(key)
            other_rsv.append(key_rsv[i] if key_rsv else 0)
            continue
        n = key_rsv[i] if key_rsv else len(value) if hasattr(value, "__len__") else 0
        if not 1 <= att <= len(atts):
            return False
        if n == 0 or n > SET_MAX or value is None:
            return False
        if typ not in KEY_SIZE:                                      # CRYO_KEY_BYTES included
            return False
        attlen, attalign = atts[att - 1]
        if attlen != KEY_SIZE[typ] or attalign < KEY_SIZE[typ]:
            return False                                             # the members themselves are never looked at
        others.append((att, 0, NOTNULL, 0))                          # the key's place among the four; well-formed as it stands
        other_rsv.append(0)
    return br.desc_ok(atts, others, flags, rsv, other_rsv if key_rsv else None)


def tuple_verdict(data, atts, keys, cols=()):
    """(TUPLE | NOMATCH | UNDECIDED | OK, [value or None per column of cols] when OK) for the tuple `data`, the first rule that
    applies: the walk fails up to the highest column it visits; some key is decidedly false; a byte-string key met an undecided
    value; a match.  A set key is never undecided and false on a NULL column"""
    last = max([k[0] for k in keys] + [c[0] for c in cols], default=0)
    w = br.walk(data, atts, last)
    if w is None:
        return TUPLE, None
    undecided = False
    for key in keys:
        att, typ, op, value = key
        isnull, at, _ = w[att - 1]
        if op == ISNULL:
            hit = isnull
        elif op == NOTNULL:
            hit = not isnull
        elif isnull:
            hit = False
        elif is_set_key(key):
            v = ar._value(data, at, typ)                             # signed, so sign-extended
            among = v in value                                       # equal to some member
            hit = among if op == IN else not among
        elif typ == BYTES:
            payload = br.stored_value(data, at)
            if payload is None:
                undecided = True
                continue
            hit = fr._compare(op, br.compare_bytes(payload, value), 0)
        else:
            hit = fr._compare(op, ar._value(data, at, typ), value)
        if not hit:
            return NOMATCH, None
    if undecided:
        return UNDECIDED, None
    return OK, [None if w[att - 1][0] else ar._value(data, w[att - 1][1], typ) for att, typ in cols]


# ---- the filter ----
def filter_block(block, atts, keys, count_only=False):
    """(status, n_items, [(pos, status, len, source offset)] of the block's records in position order)"""
    status, n, items = br._items(block)
    if status != OK:
        return status, 0, []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    upper = int(b[4:8].view("<u4")[0])
    recs = []
    for pos, bad, off, ln in items:
        if bad:
            recs.append((pos, ITEM, 0, 0))
            continue
        v, _ = tuple_verdict(b[off:off + ln].tobytes(), atts, keys)
        if v == OK:
            recs.append((pos, OK, ln, off))
        elif v in (TUPLE, UNDECIDED):
            recs.append((pos, v, 0, 0))
    if not count_only and sum(maxalign(r[2]) for r in recs if r[1] == OK) > b.size - upper:
        return OVERLAP, n, [r for r in recs if r[1] != OK]
    return OK, n, recs


def filter_call(blocks, atts, keys, flags=0, b_base=0, r_base=0):
    """(table, records, packed, (total bytes, total records)) of a call: blocks[i] a decoded block or None"""
    count_only = bool(flags & COUNT_ONLY)
    table = np.zeros(len(blocks), fr.BLOCK)
    recs, parts, at = [], [], 0
    for i, block in enumerate(blocks):
        status, n, rs = filter_block(block, atts, keys, count_only)
        n_match = sum(1 for r in rs if r[1] == OK)
        table[i] = (status, n, n_match, len(rs) - n_match, 0 if count_only else r_base + len(recs), 0 if count_only else b_base + at)
        if count_only:
            continue
        for pos, st, ln, src in rs:
            recs.append((pos, st, ln))
            if st == OK:
                t = np.zeros(maxalign(ln), np.uint8)
                t[:ln] = block[src:src + ln]
                parts.append(t)
                at += t.size
    records = np.array(recs, fr.REC) if recs else np.zeros(0, fr.REC)
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return table, records, packed, (at, len(recs))


def multi_filter_call(blocks, atts, keys, G, B, flags=0):
    """what cryo_multi_filter_blocks with G handles gives (filter_ref.multi_call's layout)"""
    return multi_ref.filter_multi(filter_call, fr.BLOCK, blocks, atts, keys, G, B, flags)


# ---- the aggregate and the grouped scan ----
def _reduce(block, atts, keys, cols):
    """((status, n_items, n_match, n_bad), [[value or None per column] per match in position order])"""
    status, n, items = br._items(block)
    if status != OK:
        return (status, 0, 0, 0), []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    n_bad, rows = 0, []
    for pos, bad, off, ln in items:
        if bad:
            n_bad += 1
            continue
        v, vals = tuple_verdict(b[off:off + ln].tobytes(), atts, keys, cols)
        if v in (TUPLE, UNDECIDED):
            n_bad += 1
        elif v == OK:
            rows.append(vals)
    return (OK, n, len(rows), n_bad), rows


def agg_call(blocks, atts, keys, cols):
    """(rows, cells of shape (n, ncols)) of a call, a multi-handle call included"""
    rows, cells = np.zeros(len(blocks), ar.ROW), np.zeros((len(blocks), len(cols)), ar.CELL)
    for i, block in enumerate(blocks):
        rows[i], matches = _reduce(block, atts, keys, cols)
        for j in range(len(cols)):
            cells[i, j] = ar.cell_of([m[j] for m in matches if m[j] is not None])
    return rows, cells


def group_call(blocks, atts, keys, by, cols):
    """(rows, records, cells of shape (groups, ncols), total) of a call, a multi-handle call included"""
    rows, recs, cells = np.zeros(len(blocks), gr.ROW), [], []
    for i, block in enumerate(blocks):
        row, matches = _reduce(block, atts, keys, list(by) + list(cols))
        groups = {}
        for m in matches:
            g = groups.setdefault(tuple(m[:len(by)]), [0, [[] for _ in cols]])
            g[0] += 1
            for j, v in enumerate(m[len(by):]):
                if v is not None:
                    g[1][j].append(v)
        rows[i] = row + (len(groups), 0, len(recs))
        for key in sorted(groups, key=gr.order_key):
            k = [0 if v is None else v for v in key] + [0] * (2 - len(key))
            recs.append((k, groups[key][0], sum(1 << j for j, v in enumerate(key) if v is None)))
            cells.append([ar.cell_of(v) for v in groups[key][1]])
    r = np.zeros(len(recs), gr.REC)
    c = np.zeros((len(recs), len(cols)), ar.CELL)
    for g, rec in enumerate(recs):
        r[g] = rec
        for j, cell in enumerate(cells[g]):
            c[g, j] = cell
    return rows, r, c, len(recs)


# ---- the projection ----
def project_tuple(data, atts, keys, cols):
    """(TUPLE | NOMATCH | UNDECIDED, None, None) or (OK, nulls, row bytes) for the tuple `data` (its len bytes)"""
    last = max([k[0] for k in keys] + list(cols))
    w = br.walk(data, atts, last)                                    # that far for every tuple, whatever the keys say
    if w is None:
        return TUPLE, None, None
    verdict, _ = tuple_verdict(data, atts, keys)
    assert verdict != TUPLE
    if verdict != OK:
        return verdict, None, None
    offsets, row_bytes = pr.row_layout(atts, cols)
    row, nulls = bytearray(row_bytes), 0
    t = fr.Tuple(data)
    for j, att in enumerate(cols):
        isnull, at, size = w[att - 1]
        if isnull:
            nulls |= 1 << j
            continue
        row[offsets[j]:offsets[j] + size] = t.bytes(at, size)
    return OK, nulls, bytes(row)


def project_call(blocks, atts, keys, cols, w_base=0, r_base=0):
    """(table, records, rows of shape (total rows, row_bytes), (total rows, total records)) of a call"""
    _, row_bytes = pr.row_layout(atts, cols)
    table = np.zeros(len(blocks), pr.BLOCK)
    recs, rows = [], []
    for i, block in enumerate(blocks):
        status, n, items = br._items(block)
        rs = []
        if status == OK:
            b = np.ascontiguousarray(block, dtype=np.uint8)
            for pos, bad, off, ln in items:
                if bad:
                    rs.append((pos, ITEM, 0, None))
                    continue
                v, nulls, row = project_tuple(b[off:off + ln].tobytes(), atts, keys, cols)
                if v == OK:
                    rs.append((pos, OK, nulls, row))
                elif v in (TUPLE, UNDECIDED):
                    rs.append((pos, v, 0, None))
        n_match = sum(1 for r in rs if r[1] == OK)
        table[i] = (status, n if status == OK else 0, n_match, len(rs) - n_match, r_base + len(recs), w_base + len(rows))
        for pos, st, nulls, row in rs:
            recs.append((pos, st, nulls))
            if st == OK:
                rows.append(np.frombuffer(row, np.uint8))
    records = np.array(recs, pr.REC) if recs else np.zeros(0, pr.REC)
    out = np.stack(rows) if rows else np.zeros((0, row_bytes), np.uint8)
    return table, records, out, (len(rows), len(recs))


def multi_project_call(blocks, atts, keys, cols, G):
    """what cryo_multi_project_blocks with G handles gives (project_ref.multi_call's layout)"""
    return multi_ref.project_multi(project_call, pr.BLOCK, blocks, atts, keys, cols, G)
