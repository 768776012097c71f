"""Reference of the projecting scan's rules (include/cryo_codec.h, "projecting a scan"), in numpy and plain Python: what
cryo_codec_project_batch must report for decoded blocks, the filter's descriptor and up to eight projected columns.  Written from
the header's comment, not from the kernel.  Test infrastructure only.

Every read of a tuple goes through filter_ref.Tuple, which refuses any index outside [0, len); the verdicts on a tuple, byte-string
keys included, are bytes_key_ref's (walk, stored_value, compare_bytes), and the walk is taken over the columns 1 .. max(highest key
column, highest projected column)."""
import numpy as np

import bytes_key_ref as br
import filter_ref as fr
import multi_ref
from bytes_key_ref import HEADER, ITEM, MAX_ITEMS, NOMATCH, OK, STREAM, TUPLE, UNDECIDED, decode, maxalign  # noqa: F401

MAX_COLS = 8
WIDTHS = (1, 2, 4, 8)
COL = np.dtype([("att", "<u2"), ("rsv", "<u2"), ("rsv2", "<u4")])
BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"), ("rec_first", "<u8"),
                  ("row_first", "<u8")])
REC = np.dtype([("pos", "<u2"), ("status", "<u2"), ("nulls", "<u4")])


def desc_ok(atts, keys, cols, flags=0, rsv=0, prj_rsv=0, col_rsv=None, col_rsv2=None, att_rsv=None, key_rsv=None):
    """the projection's argument rules: atts [(attlen, attalign)], keys [(att, type, op, value)], cols [att]"""
    if any(att_rsv or ()):
        return False
    if not br.desc_ok(atts, keys, flags, rsv, key_rsv):
        return False
    if flags != 0 or prj_rsv or any(col_rsv or ()) or any(col_rsv2 or ()):
        return False
    if not 1 <= len(cols) <= MAX_COLS:
        return False
    for att in cols:
        if not 1 <= att <= len(atts):
            return False
        attlen, attalign = atts[att - 1]
        if attlen not in WIDTHS or attalign < attlen:
            return False
    return True


def row_layout(atts, cols):
    """(offsets, row_bytes): o_0 = 0, o_j = align(o_(j-1) + w_(j-1), w_j), row_bytes = MAXALIGN(o_last + w_last)"""
    offsets, end = [], 0
    for att in cols:
        w = atts[att - 1][0]
        o = -(-end // w) * w
        offsets.append(o)
        end = o + w
    return offsets, maxalign(end)


def project_tuple(data, atts, keys, cols):
    """(TUPLE | NOMATCH | UNDECIDED, None, None) or (OK, nulls, row bytes) for the tuple `data` (its len bytes)"""
    last = max([k[0] for k in keys] + list(cols))
    w = br.walk(data, atts, last)                   # that far for every tuple, whatever the keys say
    if w is None:
        return TUPLE, None, None
    verdict, _ = br.tuple_verdict(data, atts, keys)  # the keys' verdict; its own, shorter walk cannot fail where the longer passed
    assert verdict != TUPLE
    if verdict != OK:
        return verdict, None, None
    offsets, row_bytes = row_layout(atts, cols)
    row, nulls = bytearray(row_bytes), 0
    t = fr.Tuple(data)
    for j, att in enumerate(cols):
        isnull, at, size = w[att - 1]
        if isnull:
            nulls |= 1 << j
            continue
        assert size == atts[att - 1][0] and at % size == 0           # the argument rule makes every load aligned
        row[offsets[j]:offsets[j] + size] = t.bytes(at, size)
    return OK, nulls, bytes(row)


def project_block(block, atts, keys, cols):
    """(status, n_items, [(pos, status, nulls, row bytes or None)] of the block's records in position order)"""
    status, n, items = br._items(block)
    if status != OK:
        return status, 0, []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    recs = []
    for pos, bad, off, ln in items:
        if bad:
            recs.append((pos, ITEM, 0, None))
            continue
        v, nulls, row = project_tuple(b[off:off + ln].tobytes(), atts, keys, cols)
        if v == OK:
            recs.append((pos, OK, nulls, row))
        elif v in (TUPLE, UNDECIDED):
            recs.append((pos, v, 0, None))
    return OK, n, recs


def project_call(blocks, atts, keys, cols, w_base=0, r_base=0):
    """(table, records, rows of shape (total rows, row_bytes), (total rows, total records)) of a call: blocks[i] a decoded block
    or None"""
    _, row_bytes = row_layout(atts, cols)
    table = np.zeros(len(blocks), BLOCK)
    recs, rows = [], []
    for i, block in enumerate(blocks):
        status, n, rs = project_block(block, atts, keys, cols)
        n_match = sum(1 for r in rs if r[1] == OK)
        table[i] = (status, n, n_match, len(rs) - n_match, r_base + len(recs), w_base + len(rows))
        for pos, st, nulls, row in rs:
            recs.append((pos, st, nulls))
            if st == OK:
                rows.append(np.frombuffer(row, np.uint8))
    records = np.array(recs, REC) if recs else np.zeros(0, REC)
    out = np.stack(rows) if rows else np.zeros((0, row_bytes), np.uint8)
    return table, records, out, (len(rows), len(recs))


def multi_call(blocks, atts, keys, cols, G):
    """what cryo_multi_project_blocks with G handles gives: block i -> handle i mod G; handle g has a row region and a record
    region of 290 x (its blocks) entries each, in handle order.  Returns (table in call order, [(first entry of both regions,
    rows, records)] per handle with a share, (end of the last row, of the last record used))"""
    return multi_ref.project_multi(project_call, BLOCK, blocks, atts, keys, cols, G)


def rows_of(table, records, rows, i):
    """[(pos, nulls, row bytes)] of block i's matches, found through the block table alone"""
    row = table[i]
    at, out = int(row["row_first"]), []
    for r in records[int(row["rec_first"]):int(row["rec_first"]) + int(row["n_match"]) + int(row["n_bad"])]:
        if r["status"] == OK:
            out.append((int(r["pos"]), int(r["nulls"]), bytes(rows[at])))
            at += 1
    return out
