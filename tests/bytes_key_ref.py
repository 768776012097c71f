"""Reference of the byte-string scan keys (include/cryo_codec.h, "filtering a scan": "Byte-string keys"), in numpy and plain
Python: what the filter, the aggregate and the grouped scan must report when a key of type CRYO_KEY_BYTES is among the keys.
Written from the header's comment, not from the kernel.  Test infrastructure only.

A key is (att, type, op, value) as in filter_ref; the value of a BYTES comparison is a bytes object.  Every read of a tuple goes
through filter_ref.Tuple, which refuses any index outside [0, len): in particular the payload of a varlena is read as its plen
bytes and nothing behind them.  The block, call and multi-handle layers restate filter_ref's, agg_ref's and group_ref's with the
fourth verdict, UNDECIDED, which is a bad item everywhere."""
import struct

import numpy as np

import agg_ref as ar
import filter_ref as fr
import group_ref as gr
import multi_ref
from filter_ref import (COUNT_ONLY, EQ, GE, GT, HEADER, INT2, INT4, INT8, ISNULL, ITEM, KEY_SIZE, LE, LT, MAX_ITEMS, NE, NOMATCH,  # noqa: F401
                        NOTNULL, OK, OVERLAP, STREAM, TUPLE, decode, maxalign)

BYTES = 16
BYTES_MAX = 256
UNDECIDED = 9


def is_bytes_key(key):
    return key[1] == BYTES and LT <= key[2] <= NE


def desc_ok(atts, keys, flags=0, rsv=0, key_rsv=None):
    """the descriptor's argument rules with byte-string keys.  key_rsv: the rsv field of each key as the caller set it (None: 0
    for every key but a BYTES comparison, whose rsv is its constant's length); a BYTES comparison whose value is None stands for
    a null address"""
    if not 1 <= len(atts) <= fr.MAX_ATTS or len(keys) > fr.MAX_KEYS or rsv or flags & ~COUNT_ONLY:
        return False
    for attlen, attalign in atts:
        if attlen == 0 or attlen < -1 or attlen > 32767 or attalign not in (1, 2, 4, 8):
            return False
        if attlen == -1 and attalign < 4:
            return False
    for i, key in enumerate(keys):
        att, typ, op, value = key
        if is_bytes_key(key):
            n = key_rsv[i] if key_rsv else (0 if value is None else len(value))
        else:
            n = key_rsv[i] if key_rsv else 0
            if n:
                return False                                       # rsv != 0 is refused for every other type and the null tests
        if not 1 <= att <= len(atts) or not LT <= op <= NOTNULL:
            return False
        if op in (ISNULL, NOTNULL):
            continue
        if typ == BYTES:
            if atts[att - 1][0] != -1 or n > BYTES_MAX or (n > 0 and value is None):
                return False
            continue
        if typ not in KEY_SIZE:
            return False
        size = KEY_SIZE[typ]
        attlen, attalign = atts[att - 1]
        if attlen != size or attalign < size:
            return False
        if not -(1 << (8 * size - 1)) <= value < (1 << (8 * size - 1)):
            return False
    return True


def walk(data, atts, last):
    """the walk over columns 1 .. last of the tuple `data`: None when the tuple breaks the TUPLE rule or the walk leaves it,
    else [(isnull, offset of the column within the tuple or None, its size)] per column.  Stepping is the filter's, unchanged"""
    t = fr.Tuple(data)
    if t.len < 23:
        return None
    tnatts = struct.unpack("<H", t.bytes(18, 2))[0] & 0x07FF
    hasnull = struct.unpack("<H", t.bytes(20, 2))[0] & 1
    hoff = t.byte(22)
    if hoff % 8 or hoff < maxalign(23 + ((tnatts + 7) // 8 if hasnull else 0)) or hoff > t.len:
        return None
    o, out = 0, []
    for i in range(1, last + 1):
        attlen, attalign = atts[i - 1]
        if i > tnatts or (hasnull and not (t.byte(23 + (i - 1) // 8) >> ((i - 1) % 8)) & 1):
            out.append((True, None, 0))
            continue
        if attlen > 0:
            o = (o + attalign - 1) & ~(attalign - 1)
            size = attlen
        else:
            if hoff + o >= t.len:
                return None
            if t.byte(hoff + o) == 0:
                o = (o + attalign - 1) & ~(attalign - 1)
                if hoff + o >= t.len:
                    return None
            b = t.byte(hoff + o)
            if b == 0x01:
                if hoff + o + 1 >= t.len or t.byte(hoff + o + 1) != 18:
                    return None
                size = 18
            elif b & 1:
                size = b >> 1
            else:
                if hoff + o + 4 > t.len:
                    return None
                size = struct.unpack("<I", t.bytes(hoff + o, 4))[0] >> 2
                if size < 4:
                    return None
        if hoff + o + size > t.len:
            return None
        out.append((False, hoff + o, size))
        o += size
    return out


def stored_value(data, at):
    """the payload of the non-NULL varlena at `at` (the walk has passed it), or None when its bytes are not in the tuple"""
    t = fr.Tuple(data)
    b = t.byte(at)
    if b == 0x01:
        return None                                                # an external pointer
    if b & 1:
        return t.bytes(at + 1, (b >> 1) - 1)                       # a 1-byte header
    w = struct.unpack("<I", t.bytes(at, 4))[0]
    if w & 3 == 2:
        return None                                                # compressed in line
    assert w & 3 == 0
    return t.bytes(at + 4, (w >> 2) - 4)


def compare_bytes(payload, constant):
    """c: memcmp over the shorter length on unsigned bytes, then the sign of the lengths' difference"""
    m = min(len(payload), len(constant))
    for i in range(m):
        if payload[i] != constant[i]:                              # bytes index as unsigned integers
            return -1 if payload[i] < constant[i] else 1
    return (len(payload) > len(constant)) - (len(payload) < len(constant))


def tuple_verdict(data, atts, keys, cols=()):
    """(TUPLE | NOMATCH | UNDECIDED | OK, [value or None per column of cols] when OK) for the tuple `data`, the first rule that
    applies: the walk fails up to the highest column it visits; some key is decidedly false; a byte-string key met an undecided
    value; a match"""
    last = max([k[0] for k in keys] + [c[0] for c in cols], default=0)
    w = walk(data, atts, last)
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
        elif typ == BYTES:
            payload = stored_value(data, at)
            if payload is None:
                undecided = True
                continue
            hit = fr._compare(op, compare_bytes(payload, value), 0)
        else:
            hit = fr._compare(op, ar._value(data, at, typ), value)
        if not hit:
            return NOMATCH, None
    if undecided:
        return UNDECIDED, None
    return OK, [None if w[att - 1][0] else ar._value(data, w[att - 1][1], typ) for att, typ in cols]


def _items(block):
    """(status, n, [(pos, ITEM or None, off, len)]) of a decoded block: the fetch's header and ITEM rules"""
    if block is None:
        return STREAM, 0, []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    B = b.size
    assert B % 8 == 0 and B >= 16
    lower, upper = (int(v) for v in b[:8].view("<u4"))
    n = (lower - 8) // 8
    if lower < 8 or (lower - 8) % 8 or n > MAX_ITEMS or not lower <= upper <= B or (n == 0 and upper != B):
        return HEADER, 0, []
    out = []
    for pos in range(1, n + 1):
        off, ln = struct.unpack_from("<II", b, 8 + 8 * (pos - 1))
        bad = ln == 0 or off % 8 or off < upper or off + maxalign(ln) > B
        out.append((pos, ITEM if bad else None, off, ln))
    return OK, n, out


# ---- the filter ----
def filter_block(block, atts, keys, count_only=False):
    """(status, n_items, [(pos, status, len, source offset)] of the block's records in position order)"""
    status, n, items = _items(block)
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
    """what cryo_multi_filter_blocks with G handles gives (filter_ref.multi_call's layout): (table in call order, [(byte start,
    packed bytes, record start, records)] per handle with a share, (end of the last byte, of the last record used))"""
    return multi_ref.filter_multi(filter_call, fr.BLOCK, blocks, atts, keys, G, B, flags)


# ---- the aggregate ----
def _reduce(block, atts, keys, cols):
    """((status, n_items, n_match, n_bad), [[value or None per column] per match in position order])"""
    status, n, items = _items(block)
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
    """(rows, cells of shape (n, ncols)) of a call, a multi-handle call included: blocks[i] a decoded block or None"""
    rows, cells = np.zeros(len(blocks), ar.ROW), np.zeros((len(blocks), len(cols)), ar.CELL)
    for i, block in enumerate(blocks):
        rows[i], matches = _reduce(block, atts, keys, cols)
        for j in range(len(cols)):
            cells[i, j] = ar.cell_of([m[j] for m in matches if m[j] is not None])
    return rows, cells


# ---- the grouped scan ----
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
