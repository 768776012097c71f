"""Reference of the ordered scan's rules (include/cryo_codec.h, "ordering a scan"), in numpy and plain Python: what
cryo_codec_topn_batch must report for decoded blocks, the filter's descriptor, one or two order columns with a limit and up to
eight projected columns; the multi-GPU regions and the merge of blocks.  Written from the header's comment, not from the kernel.
Test infrastructure only.

Every read of a tuple goes through filter_ref.Tuple, which refuses any index outside [0, len).  The walk is bytes_key_ref's, taken
over the columns 1 .. max(highest key column, highest projected column, highest order column); the keys' verdict is float_ref's,
which knows every kind of key and the truth table; the row is laid out by project_ref's rule.  A block's matches are sorted with
Python's sort on tuples ((class, value) per order column, position): DESC negates the value (Python integers do not overflow), so
nothing here shares a trick with the kernel."""
import struct

import numpy as np

import bytes_key_ref as br
import filter_ref as fr
import float_ref as fl
import multi_ref
import project_ref as pr
from bytes_key_ref import HEADER, ITEM, MAX_ITEMS, NOMATCH, OK, STREAM, TUPLE, UNDECIDED  # noqa: F401

DESC, NULLS_FIRST = 1, 2
MAX_BY = 2
INT2, INT4, INT8, FLOAT4, FLOAT8 = fr.INT2, fr.INT4, fr.INT8, fl.FLOAT4, fl.FLOAT8
SIZE = {INT2: 2, INT4: 4, INT8: 8, FLOAT4: 4, FLOAT8: 8}
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)
ORDER_COL = np.dtype([("att", "<u2"), ("type", "u1"), ("flags", "u1"), ("rsv", "<u4")])
BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"), ("n_rows", "<u4"), ("rsv", "<u4"),
                  ("row_first", "<u8")])
REC = np.dtype([("key", "<i8", (2,)), ("pos", "<u2"), ("key_nulls", "<u2"), ("nulls", "<u4")])


def desc_ok(atts, keys, by, limit, cols, flags=0, rsv=0, prj_rsv=0, col_rsv=None, col_rsv2=None, att_rsv=None, key_rsv=None,
            by_rsv=None):
    """the ordered scan's argument rules: atts [(attlen, attalign)], keys [(att, type, op, value)], by [(att, type, flags)],
    cols [att]"""
    if any(att_rsv or ()) or flags != 0:
        return False
    if not fl.desc_ok(atts, keys, flags, rsv, key_rsv):
        return False
    if prj_rsv or any(col_rsv or ()) or any(col_rsv2 or ()) or not 1 <= len(cols) <= pr.MAX_COLS:
        return False
    for att in cols:
        if not 1 <= att <= len(atts) or atts[att - 1][0] not in pr.WIDTHS or atts[att - 1][1] < atts[att - 1][0]:
            return False
    if not 1 <= len(by) <= MAX_BY or limit < 1 or any(by_rsv or ()):
        return False
    for att, typ, oflags in by:
        if typ not in SIZE or oflags & ~(DESC | NULLS_FIRST) or not 1 <= att <= len(atts):
            return False
        if atts[att - 1][0] != SIZE[typ] or atts[att - 1][1] < SIZE[typ]:
            return False
    return True


def image(raw, typ):
    """the signed 64-bit integer the order compares of the column's stored integer `raw`: the value itself, or for a float column
    the image of the header's rule"""
    if typ == FLOAT4:
        x = struct.unpack("<f", struct.pack("<i", raw))[0]               # Python's float is the exactly widened double
    elif typ == FLOAT8:
        x = struct.unpack("<d", struct.pack("<q", raw))[0]
    else:
        return raw
    if x != x:
        return INT64_MAX
    if x == 0:
        return 0
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b if b >> 63 == 0 else (b ^ 0x7FFFFFFFFFFFFFFF) - (1 << 64)


def sort_key(by, key, key_nulls):
    """((class, value under the direction) per order column) of a record's key and key_nulls"""
    out = []
    for j, (_, _, oflags) in enumerate(by):
        if (key_nulls >> j) & 1:
            out.append((0 if oflags & NULLS_FIRST else 2, 0))
        else:
            out.append((1, -key[j] if oflags & DESC else key[j]))
    return tuple(out)


def topn_tuple(data, atts, keys, by, cols, truth=None):
    """(TUPLE | NOMATCH | UNDECIDED, ...) or (OK, key [2], key_nulls, nulls, row bytes) for the tuple `data` (its len bytes)"""
    last = max([k[0] for k in keys] + list(cols) + [b[0] for b in by])
    w = br.walk(data, atts, last)                                        # that far for every tuple, whatever the keys say
    if w is None:
        return TUPLE, None, None, None, None
    verdict, _ = fl.tuple_verdict(data, atts, keys, (), truth)           # its own, shorter walk cannot fail where the longer passed
    assert verdict != TUPLE
    if verdict != OK:
        return verdict, None, None, None, None
    t = fr.Tuple(data)
    offsets, row_bytes = pr.row_layout(atts, cols)
    row, nulls = bytearray(row_bytes), 0
    for j, att in enumerate(cols):
        isnull, at, size = w[att - 1]
        if isnull:
            nulls |= 1 << j
            continue
        assert size == atts[att - 1][0] and at % size == 0
        row[offsets[j]:offsets[j] + size] = t.bytes(at, size)
    key, key_nulls = [0, 0], 0
    for j, (att, typ, _) in enumerate(by):
        isnull, at, size = w[att - 1]
        if isnull:
            key_nulls |= 1 << j
            continue
        assert size == SIZE[typ] and at % size == 0
        key[j] = image(int.from_bytes(t.bytes(at, size), "little", signed=True), typ)
    return OK, key, key_nulls, nulls, bytes(row)


def topn_block(block, atts, keys, by, limit, cols, truth=None):
    """(status, n_items, n_match, n_bad, [(key, key_nulls, pos, nulls, row bytes)] of the kept rows in rank order)"""
    status, n, items = br._items(block)
    if status != OK:
        return status, 0, 0, 0, []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    matches, n_bad = [], 0
    for pos, bad, off, ln in items:
        if bad:
            n_bad += 1
            continue
        v, key, key_nulls, nulls, row = topn_tuple(b[off:off + ln].tobytes(), atts, keys, by, cols, truth)
        if v == OK:
            matches.append((key, key_nulls, pos, nulls, row))
        elif v in (TUPLE, UNDECIDED):
            n_bad += 1
    matches.sort(key=lambda m: (sort_key(by, m[0], m[1]), m[2]))
    return OK, n, len(matches), n_bad, matches[:limit]


def topn_call(blocks, atts, keys, by, limit, cols, truth=None, w_base=0):
    """(table, records, rows of shape (total, row_bytes), total) of a call: blocks[i] a decoded block or None"""
    _, row_bytes = pr.row_layout(atts, cols)
    table = np.zeros(len(blocks), BLOCK)
    recs, rows = [], []
    for i, block in enumerate(blocks):
        status, n, n_match, n_bad, kept = topn_block(block, atts, keys, by, limit, cols, truth)
        table[i] = (status, n, n_match, n_bad, len(kept), 0, w_base + len(rows))
        for key, key_nulls, pos, nulls, row in kept:
            recs.append((key, pos, key_nulls, nulls))
            rows.append(np.frombuffer(row, np.uint8))
    records = np.zeros(len(recs), REC)
    for i, r in enumerate(recs):
        records[i] = r
    out = np.stack(rows) if rows else np.zeros((0, row_bytes), np.uint8)
    return table, records, out, len(rows)


def multi_call(blocks, atts, keys, by, limit, cols, G, truth=None):
    """what cryo_multi_topn_blocks with G handles gives: block i -> handle i mod G; handle g has one region of min(limit, 290) x
    (its blocks) entries of rows and records alike, in handle order.  Returns (table in call order, [(first entry of the region,
    rows, records)] per handle with a share, the end of the last entry used)"""
    table = np.zeros(len(blocks), BLOCK)

    def one(idx, bases):
        t, recs, rows, total = topn_call([blocks[i] for i in idx], atts, keys, by, limit, cols, truth, bases[0])
        table[idx] = t
        return (recs, rows), [total]
    out, ends = multi_ref.share_regions(len(blocks), G, (min(limit, MAX_ITEMS),), one)
    return table, [(bases[0], rows, recs) for _, bases, (recs, rows) in out], ends[0]


def merge(by, limit, blocks):
    """the first `limit` rows of the blocks added, in this order: blocks a sequence of (records, rows).  Ordered by the descriptor
    over key / key_nulls; ties go to the block added earlier, then to the block's own order.  Returns (records, rows)"""
    entries = []
    for b, (recs, rows) in enumerate(blocks):
        for r in range(len(recs)):
            entries.append((sort_key(by, [int(k) for k in recs[r]["key"]], int(recs[r]["key_nulls"])), b, r))
    entries.sort()
    entries = entries[:limit]
    row_bytes = next((np.asarray(rows).shape[1] for _, rows in blocks if len(rows)), 0)
    out_rec, out_rows = np.zeros(len(entries), REC), np.zeros((len(entries), row_bytes), np.uint8)
    for i, (_, b, r) in enumerate(entries):
        out_rec[i] = blocks[b][0][r]
        out_rows[i] = blocks[b][1][r]
    return out_rec, out_rows


def kept_of(table, records, rows, i):
    """[(key 1, key 2, key_nulls, pos, nulls, row bytes)] of block i's kept rows in rank order, found through the table alone"""
    at, k = int(table[i]["row_first"]), int(table[i]["n_rows"])
    return [(int(r["key"][0]), int(r["key"][1]), int(r["key_nulls"]), int(r["pos"]), int(r["nulls"]), bytes(w))
            for r, w in zip(records[at:at + k], rows[at:at + k])]
