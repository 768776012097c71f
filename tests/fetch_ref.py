"""Reference of the tuple fetch's rules (include/cryo_codec.h, "fetching tuples by position"), in numpy: what
cryo_codec_fetch_batch must report and pack for decoded blocks and lists of item positions.  Test infrastructure only.

A block of B bytes (B a multiple of 8, at least 16; fields LE u32): lower at 0, upper at 4, n = (lower - 8) / 8, item i =
(off_i at 8 + 8i, len_i at 12 + 8i), MAXALIGN(x) = (x + 7) & ~7.  Per block, the first failing class wins:
  STREAM   every request   the stream does not decode to B bytes (the block is None here)
  HEADER   every request   lower >= 8, (lower - 8) % 8 == 0, n <= 290, lower <= upper <= B, upper == B when n == 0 -- fails
  BADREQ   every request   a position is 0, or the block's positions are not strictly ascending
  NOITEM   the request     pos > n
  ITEM     the request     item pos - 1 has len == 0, off % 8 != 0, off < upper or off + MAXALIGN(len) > B
  OVERLAP  every request still OK   the MAXALIGNed lengths of the block's OK requests sum to more than B - upper
  OK       the request     len = len_i
Placement: requests in call order; off = the sum of MAXALIGN(len) over the OK requests before (a failed request has len 0);
the destination holds the tuple's len bytes, then zeros up to MAXALIGN(len) whatever the block's pad holds."""
import struct

import numpy as np

import multi_ref
from layout_ref import decode, maxalign  # noqa: F401  (decode: the oracle's decode of a stream, or None)

OK, STREAM, HEADER, ITEM, NOITEM, BADREQ, OVERLAP = 0, 1, 2, 3, 5, 6, 7
MAX_ITEMS = 290
RESULT = np.dtype([("status", "<u4"), ("len", "<u4"), ("off", "<u8")])


def fetch_block(block, positions):
    """[(status, len, source offset)] of one block's requests; block: uint8 array of B bytes, or None (STREAM)"""
    positions = [int(p) for p in positions]
    if block is None:
        return [(STREAM, 0, 0)] * len(positions)
    b = np.ascontiguousarray(block, dtype=np.uint8)
    B = b.size
    assert B % 8 == 0 and B >= 16
    lower, upper = (int(v) for v in b[:8].view("<u4"))
    n = (lower - 8) // 8
    if lower < 8 or (lower - 8) % 8 or n > MAX_ITEMS or not lower <= upper <= B or (n == 0 and upper != B):
        return [(HEADER, 0, 0)] * len(positions)
    if any(p == 0 for p in positions) or any(q <= p for p, q in zip(positions, positions[1:])):
        return [(BADREQ, 0, 0)] * len(positions)
    out = []
    for p in positions:
        if p > n:
            out.append((NOITEM, 0, 0))
            continue
        off, ln = struct.unpack_from("<II", b, 8 + 8 * (p - 1))
        if ln == 0 or off % 8 or off < upper or off + maxalign(ln) > B:
            out.append((ITEM, 0, 0))
        else:
            out.append((OK, ln, off))
    if sum(maxalign(ln) for st, ln, _ in out if st == OK) > B - upper:
        out = [(OVERLAP, 0, 0) if st == OK else (st, 0, 0) for st, _, _ in out]
    return out


def fetch_call(blocks, requests, base=0):
    """(records, packed, total) of a call: records a RESULT array in call order with `off` counting from `base` on, packed the
    `total` bytes the call writes; blocks[i] a decoded block or None, requests[i] its positions"""
    recs, parts, at = [], [], 0
    for block, positions in zip(blocks, requests):
        for st, ln, src in fetch_block(block, positions):
            recs.append((st, ln, base + at))
            if st == OK:
                t = np.zeros(maxalign(ln), np.uint8)
                t[:ln] = block[src:src + ln]
                parts.append(t)
                at += t.size
    records = np.array(recs, RESULT) if recs else np.zeros(0, RESULT)
    packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return records, packed, at


def multi_call(blocks, requests, G, B):
    """what cryo_multi_fetch_blocks with G handles gives: block i -> handle i mod G, handle g packs its share into a region of
    B * (its blocks) bytes, the regions in handle order.  Returns (records in call order, [(region start, packed bytes)] per
    handle with a share, total: the end of the last byte used)"""
    return multi_ref.fetch_multi(fetch_call, RESULT, blocks, requests, G, B)


def build_block(B, lens, pad=0xEE, fill=None):
    """a well-formed block of tuples of the given lengths, the bytes of tuple i set to fill(i) (default: a pattern that differs
    from tuple to tuple and byte to byte) and every PAD byte set to `pad` -- what a fetch must never let through"""
    b = np.zeros(B, np.uint8)
    off = B
    for i, ln in enumerate(lens):
        off -= maxalign(ln)
        assert off >= 8 + 8 * len(lens), "the tuples do not fit"
        b[off:off + ln] = fill(i) if fill else ((np.arange(ln) * 7 + i * 13 + 1) % 251 + 1).astype(np.uint8)
        b[off + ln:off + maxalign(ln)] = pad
        b[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", off, ln), np.uint8)
    b[:8] = np.frombuffer(struct.pack("<II", 8 + 8 * len(lens), off), np.uint8)
    return b


def slice_by_items(block):
    """[(tuple bytes)] of a well-formed block, by its item ids: what cryo_storage_fetch hands out"""
    b = np.ascontiguousarray(block, dtype=np.uint8)
    lower = int(b[:4].view("<u4")[0])
    out = []
    for i in range((lower - 8) // 8):
        off, ln = struct.unpack_from("<II", b, 8 + 8 * i)
        out.append(b[off:off + ln].copy())
    return out
