"""Reference of the scan aggregate's rules (include/cryo_codec.h, "aggregating a scan"), in numpy and plain Python: what
cryo_codec_agg_batch must report for decoded blocks, the filter's descriptor and up to four aggregate columns.  Written from the
header's comment, not from the kernel.  Test infrastructure only.

Every read of a tuple goes through filter_ref.Tuple, which refuses any index outside [0, len).  Sums are Python integers, split
into the cell's two words at the very end."""
import struct

import numpy as np

import filter_ref as fr
from filter_ref import HEADER, KEY_SIZE, OK, STREAM, TUPLE, decode, maxalign  # noqa: F401  (decode: for the callers)

MAX_COLS = 4
ROW = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4")])
CELL = np.dtype([("n", "<u8"), ("min", "<i8"), ("max", "<i8"), ("sum_lo", "<u8"), ("sum_hi", "<i8")])


def desc_ok(atts, keys, cols, flags=0, rsv=0, agg_rsv=0, col_rsv=None, **kw):
    """the aggregate's argument rules: atts [(attlen, attalign)], keys [(att, type, op, value)], cols [(att, type)]"""
    if not fr.desc_ok(atts, keys, flags, rsv, **kw) or flags != 0 or agg_rsv or any(col_rsv or ()):
        return False
    if not 1 <= len(cols) <= MAX_COLS:
        return False
    for att, typ in cols:
        if not 1 <= att <= len(atts) or typ not in KEY_SIZE:
            return False
        attlen, attalign = atts[att - 1]
        if attlen != KEY_SIZE[typ] or attalign < attlen:
            return False
    return True


def walk(data, atts, last):
    """the walk over columns 1 .. last of the tuple `data` (its len bytes): None when the tuple breaks the TUPLE rule or the
    walk leaves it, else [(isnull, offset of the column within the tuple or None)] per column"""
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
            out.append((True, None))
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
        out.append((False, hoff + o))
        o += size
    return out


def _value(data, at, typ):
    size = KEY_SIZE[typ]
    assert at % size == 0                                     # the argument rule makes every load aligned
    return int.from_bytes(fr.Tuple(data).bytes(at, size), "little", signed=True)


def agg_tuple(data, atts, keys, cols):
    """(TUPLE, None), (NOMATCH, None) or (OK, [value or None per aggregate column]) for the tuple `data`"""
    last = max([k[0] for k in keys] + [c[0] for c in cols])
    w = walk(data, atts, last)
    if w is None:
        return TUPLE, None
    for att, typ, op, value in keys:
        isnull, at = w[att - 1]
        if op == fr.ISNULL:
            hit = isnull
        elif op == fr.NOTNULL:
            hit = not isnull
        else:
            hit = not isnull and fr._compare(op, _value(data, at, typ), value)
        if not hit:
            return fr.NOMATCH, None
    return OK, [None if w[att - 1][0] else _value(data, w[att - 1][1], typ) for att, typ in cols]


def split(total):
    """(sum_lo, sum_hi) of a Python integer as a 128-bit two's-complement number"""
    u = total & ((1 << 128) - 1)
    lo, hi = u & ((1 << 64) - 1), u >> 64
    return lo, hi - (1 << 64) if hi >> 63 else hi


def cell_of(values):
    """the cell of a list of non-NULL values"""
    if not values:
        return (0, 0, 0, 0, 0)
    return (len(values), min(values), max(values)) + split(sum(values))


def agg_block(block, atts, keys, cols):
    """((status, n_items, n_match, n_bad), [cell per aggregate column]) of one decoded block, or of None (a rejected stream)"""
    zero = [cell_of([])] * len(cols)
    if block is None:
        return (STREAM, 0, 0, 0), zero
    b = np.ascontiguousarray(block, dtype=np.uint8)
    B = b.size
    assert B % 8 == 0 and B >= 16
    lower, upper = (int(v) for v in b[:8].view("<u4"))
    n = (lower - 8) // 8
    if lower < 8 or (lower - 8) % 8 or n > fr.MAX_ITEMS or not lower <= upper <= B or (n == 0 and upper != B):
        return (HEADER, 0, 0, 0), zero
    n_match = n_bad = 0
    values = [[] for _ in cols]
    for pos in range(1, n + 1):
        off, ln = struct.unpack_from("<II", b, 8 + 8 * (pos - 1))
        if ln == 0 or off % 8 or off < upper or off + maxalign(ln) > B:
            n_bad += 1
            continue
        verdict, vals = agg_tuple(b[off:off + ln].tobytes(), atts, keys, cols)
        if verdict == TUPLE:
            n_bad += 1
        elif verdict == OK:
            n_match += 1
            for j, v in enumerate(vals):
                if v is not None:
                    values[j].append(v)
    return (OK, n, n_match, n_bad), [cell_of(v) for v in values]


def agg_call(blocks, atts, keys, cols):
    """(rows, cells of shape (n, ncols)) of a call: blocks[i] a decoded block or None"""
    rows, cells = np.zeros(len(blocks), ROW), np.zeros((len(blocks), len(cols)), CELL)
    for i, block in enumerate(blocks):
        row, cs = agg_block(block, atts, keys, cols)
        rows[i] = row
        for j, c in enumerate(cs):
            cells[i, j] = c
    return rows, cells


def total_of(cell):
    return (int(cell["sum_hi"]) << 64) + int(cell["sum_lo"])


def combine(rows, cells):
    """the cells combined over the blocks with status OK: per column (n, min, max, sum as a Python integer)"""
    out = []
    for j in range(cells.shape[1]):
        ok = [cells[i, j] for i in range(len(rows)) if rows[i]["status"] == OK and cells[i, j]["n"] > 0]
        out.append((sum(int(c["n"]) for c in ok), min((int(c["min"]) for c in ok), default=0),
                    max((int(c["max"]) for c in ok), default=0), sum(total_of(c) for c in ok)))
    return out
