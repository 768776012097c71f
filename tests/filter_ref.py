"""Reference of the scan filter's rules (include/cryo_codec.h, "filtering a scan"), in numpy and plain Python: what
cryo_codec_filter_batch must report and pack for decoded blocks, a column descriptor and up to four scan keys.  Written from the
header's comment, not from the kernel.  Test infrastructure only.

Every read of a tuple goes through Tuple, which refuses any index outside [0, len): the reference cannot look outside a tuple
without failing an assertion."""
import struct

import numpy as np

import multi_ref
from layout_ref import decode, maxalign  # noqa: F401  (decode: the oracle's decode of a stream, or None)

OK, STREAM, HEADER, ITEM, OVERLAP, TUPLE = 0, 1, 2, 3, 7, 8
NOMATCH = -1
MAX_ITEMS, MAX_ATTS, MAX_KEYS = 290, 1600, 4
COUNT_ONLY = 1
INT2, INT4, INT8 = 1, 2, 3
LT, LE, EQ, GE, GT, NE, ISNULL, NOTNULL = range(1, 9)
KEY_SIZE = {INT2: 2, INT4: 4, INT8: 8}
BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"), ("rec_first", "<u8"), ("off", "<u8")])
REC = np.dtype([("pos", "<u2"), ("status", "<u2"), ("len", "<u4")])


def desc_ok(atts, keys, flags=0, rsv=0, att_rsv=None, key_rsv=None):
    """the descriptor's argument rules: atts [(attlen, attalign)], keys [(att, type, op, value)]"""
    if not 1 <= len(atts) <= MAX_ATTS or len(keys) > MAX_KEYS or rsv or flags & ~COUNT_ONLY:
        return False
    if any(att_rsv or ()) or any(key_rsv or ()):
        return False
    for attlen, attalign in atts:
        if attlen == 0 or attlen < -1 or attlen > 32767 or attalign not in (1, 2, 4, 8):
            return False
        if attlen == -1 and attalign < 4:
            return False
    for att, typ, op, value in keys:
        if not 1 <= att <= len(atts) or not LT <= op <= NOTNULL:
            return False
        if op in (ISNULL, NOTNULL):
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


class Tuple:
    """the len bytes of one tuple with bounds-checked reads: nothing outside [0, len) is ever loaded"""

    def __init__(self, data):
        self.d = bytes(data)
        self.len = len(self.d)

    def byte(self, at):
        assert 0 <= at < self.len, ("read outside the tuple", at, self.len)
        return self.d[at]

    def bytes(self, at, n):
        assert 0 <= at and at + n <= self.len, ("read outside the tuple", at, n, self.len)
        return self.d[at:at + n]


def _compare(op, v, k):
    return {LT: v < k, LE: v <= k, EQ: v == k, GE: v >= k, GT: v > k, NE: v != k}[op]


def _align(x, a):
    return (x + a - 1) & ~(a - 1)


def filter_tuple(data, atts, keys):
    """OK (a match), NOMATCH or TUPLE for the tuple `data` (its len bytes)"""
    t = Tuple(data)
    if t.len < 23:
        return TUPLE
    tnatts = struct.unpack("<H", t.bytes(18, 2))[0] & 0x07FF
    hasnull = struct.unpack("<H", t.bytes(20, 2))[0] & 1
    hoff = t.byte(22)
    if hoff % 8 or hoff < maxalign(23 + ((tnatts + 7) // 8 if hasnull else 0)) or hoff > t.len:
        return TUPLE
    last = max((k[0] for k in keys), default=0)
    o, ok = 0, True
    for i in range(1, last + 1):
        attlen, attalign = atts[i - 1]
        isnull = i > tnatts or bool(hasnull and not (t.byte(23 + (i - 1) // 8) >> ((i - 1) % 8)) & 1)
        value_at = None
        if not isnull:
            if attlen > 0:
                o = _align(o, attalign)
                size = attlen
                if hoff + o + size > t.len:
                    return TUPLE
            else:
                if hoff + o >= t.len:
                    return TUPLE
                if t.byte(hoff + o) == 0:
                    o = _align(o, attalign)
                    if hoff + o >= t.len:
                        return TUPLE
                b = t.byte(hoff + o)
                if b == 0x01:
                    if hoff + o + 1 >= t.len or t.byte(hoff + o + 1) != 18:
                        return TUPLE
                    size = 18
                elif b & 1:
                    size = b >> 1
                else:
                    if hoff + o + 4 > t.len:
                        return TUPLE
                    size = struct.unpack("<I", t.bytes(hoff + o, 4))[0] >> 2
                    if size < 4:
                        return TUPLE
                if hoff + o + size > t.len:
                    return TUPLE
            value_at = hoff + o
            o += size
        for att, typ, op, value in keys:
            if att != i:
                continue
            if op == ISNULL:
                ok = ok and isnull
            elif op == NOTNULL:
                ok = ok and not isnull
            elif isnull:
                ok = False
            else:
                size = KEY_SIZE[typ]
                assert value_at % size == 0                       # the argument rule makes every key load aligned
                v = int.from_bytes(t.bytes(value_at, size), "little", signed=True)
                ok = ok and _compare(op, v, value)
    return OK if ok else NOMATCH


def filter_block(block, atts, keys, count_only=False):
    """(status, n_items, [(pos, status, len, source offset)] of the block's records in position order)"""
    if block is None:
        return STREAM, 0, []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    B = b.size
    assert B % 8 == 0 and B >= 16
    lower, upper = (int(v) for v in b[:8].view("<u4"))
    n = (lower - 8) // 8
    if lower < 8 or (lower - 8) % 8 or n > MAX_ITEMS or not lower <= upper <= B or (n == 0 and upper != B):
        return HEADER, 0, []
    recs = []
    for pos in range(1, n + 1):
        off, ln = struct.unpack_from("<II", b, 8 + 8 * (pos - 1))
        if ln == 0 or off % 8 or off < upper or off + maxalign(ln) > B:
            recs.append((pos, ITEM, 0, 0))
            continue
        v = filter_tuple(b[off:off + ln].tobytes(), atts, keys)
        if v == OK:
            recs.append((pos, OK, ln, off))
        elif v == TUPLE:
            recs.append((pos, TUPLE, 0, 0))
    status = OK
    if not count_only and sum(maxalign(r[2]) for r in recs if r[1] == OK) > B - upper:
        status = OVERLAP
        recs = [r for r in recs if r[1] != OK]
    return status, n, recs


def filter_call(blocks, atts, keys, flags=0, b_base=0, r_base=0):
    """(table, records, packed, (total bytes, total records)) of a call: blocks[i] a decoded block or None"""
    count_only = bool(flags & COUNT_ONLY)
    table = np.zeros(len(blocks), BLOCK)
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
    records = np.array(recs, REC) if recs else np.zeros(0, REC)
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return table, records, packed, (at, len(recs))


def multi_call(blocks, atts, keys, G, B, flags=0):
    """what cryo_multi_filter_blocks with G handles gives: block i -> handle i mod G; handle g has a tuple region of B x (its
    blocks) bytes and a record region of 290 x (its blocks) records, in handle order.  Returns (table in call order, [(byte
    start, packed bytes, record start, records)] per handle with a share, (end of the last byte, of the last record used))"""
    return multi_ref.filter_multi(filter_call, BLOCK, blocks, atts, keys, G, B, flags)


def tuples_of(table, records, dst, i):
    """[(pos, tuple bytes)] of block i's matches, found through the block table alone"""
    row = table[i]
    at, out = int(row["off"]), []
    for r in records[int(row["rec_first"]):int(row["rec_first"]) + int(row["n_match"]) + int(row["n_bad"])]:
        if r["status"] == OK:
            out.append((int(r["pos"]), bytes(dst[at:at + int(r["len"])])))
            at += maxalign(int(r["len"]))
    return out
