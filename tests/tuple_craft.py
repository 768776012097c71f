"""Heap tuples made by hand: a numpy/struct restatement of PostgreSQL's heap_form_tuple / heap_fill_tuple
(common/heaptuple.c) for the column kinds the scan filter knows -- fixed-width integers and varlenas -- on a little-endian
machine.  Test infrastructure only.

A tuple is the 23-byte HeapTupleHeaderData (t_infomask2 at 18: the number of attributes; t_infomask at 20: HEAP_HASNULL 0x0001,
HEAP_HASVARWIDTH 0x0002, HEAP_XMAX_INVALID 0x0800; t_hoff at 22), the null bitmap when a column is null (bit SET: not null),
zeros up to t_hoff = MAXALIGN(23 + bitmap), then the columns: a fixed-width one after zero pad bytes up to its attalign; a
varlena of up to 126 payload bytes with a 1-byte header ((payload + 1) << 1 | 1) and NO alignment; a longer one after zero pad
bytes up to its attalign with a 4-byte header ((payload + 4) << 2); an on-disk TOAST pointer as its 18 bytes (0x01, tag 18, 16
bytes), not aligned."""
import struct

import numpy as np

import fetch_ref

HASNULL, HASVARWIDTH, XMAX_INVALID = 0x0001, 0x0002, 0x0800


class Long:
    """a varlena that keeps its 4-byte header whatever its length (heap_fill_tuple would shorten it up to 126 bytes)"""

    def __init__(self, payload):
        self.payload = bytes(payload)


class Toast:
    """an external pointer: 0x01, the tag, 16 bytes"""

    def __init__(self, tag=18):
        self.tag = tag


def maxalign(x):
    return (x + 7) & ~7


def form_tuple(atts, values, xmin=1000, infomask2_flags=0, infomask_flags=0, extra_hoff=0, force_bitmap=False):
    """the bytes of a tuple with len(values) attributes (may be fewer than the relation has: columns added later).  atts:
    [(attlen, attalign)]; values[i]: None (NULL), an int (fixed width), bytes / Long / Toast (varlena).

    The header is the minimal one unless a knob says otherwise: infomask2_flags is OR-ed into bits 11 .. 15 of t_infomask2
    (HEAP_KEYS_UPDATED 0x2000, HEAP_HOT_UPDATED 0x4000, HEAP_ONLY_TUPLE 0x8000); infomask_flags into t_infomask, whose bits 0 and 1
    (HASNULL, HASVARWIDTH) stay this function's; extra_hoff, a multiple of 8, is added to t_hoff and the gap holds zeros;
    force_bitmap writes HASNULL and a bitmap (every bit set) although no value is NULL"""
    natts = len(values)
    assert infomask2_flags & ~0xF800 == 0 and infomask_flags & ~0xFFFC == 0 and extra_hoff % 8 == 0 and extra_hoff >= 0
    hasnull = force_bitmap or any(v is None for v in values)
    bitmap = bytearray((natts + 7) // 8 if hasnull else 0)
    hoff = maxalign(23 + len(bitmap)) + extra_hoff
    assert hoff <= 255
    data = bytearray()
    infomask = XMAX_INVALID | (HASNULL if hasnull else 0) | infomask_flags
    for i, v in enumerate(values):
        attlen, attalign = atts[i]
        if v is None:
            continue
        if hasnull:
            bitmap[i // 8] |= 1 << (i % 8)
        if attlen > 0:
            data += bytes(-len(data) % attalign)
            data += int(v).to_bytes(attlen, "little", signed=True)
            continue
        infomask |= HASVARWIDTH
        if isinstance(v, Toast):
            data += bytes([0x01, v.tag]) + bytes(range(16))
        elif isinstance(v, Long) or len(v) > 126:
            payload = v.payload if isinstance(v, Long) else bytes(v)
            data += bytes(-len(data) % attalign)
            data += struct.pack("<I", (len(payload) + 4) << 2) + payload
        else:
            data += bytes([((len(v) + 1) << 1) | 1]) + bytes(v)
    head = bytearray(23)
    struct.pack_into("<I", head, 0, xmin)
    struct.pack_into("<HH", head, 18, natts | infomask2_flags, infomask)
    head[22] = hoff
    return bytes(head) + bytes(bitmap) + bytes(hoff - 23 - len(bitmap)) + bytes(data)


def build_block(B, tuples, pad=0xEE):
    """a well-formed block of the given tuples (bytes), every pad byte set to `pad`"""
    return fetch_ref.build_block(B, [len(t) for t in tuples], pad=pad, fill=lambda i: np.frombuffer(tuples[i], np.uint8))
