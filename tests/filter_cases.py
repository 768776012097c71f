"""The hand-made vectors of the scan-filter tests, shared by the CPU test (what tests/filter_ref.py must say about them) and the
GPU test (the kernel against filter_ref on the same blocks).  B = 4096; the tuples are crafted with tests/tuple_craft.py over
the descriptor (int2, int8, text, int4, text, int8).  Test infrastructure only.

cases() yields (name, block, keys, matches, bad): matches the positions that must match, bad {position: status}."""
import struct

import numpy as np

import filter_ref as fr
import tuple_craft as tc
from tuple_craft import Long, Toast

B = 4096
ATTS = [(2, 2), (8, 8), (-1, 4), (4, 4), (-1, 4), (8, 8)]
GOOD = (5, 100, b"abc", 7, b"xy", 900)
K6 = [(6, fr.INT8, fr.EQ, 900)]
K4 = [(4, fr.INT4, fr.EQ, 7)]
WALK = [(6, fr.INT8, fr.GE, 0)]              # makes the walk pass every column


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def with_null(at):
    v = list(GOOD)
    v[at] = None
    return T(*v)


def patched(t, at, data):
    b = bytearray(t)
    b[at:at + len(data)] = data
    return bytes(b)


def tuple_cases():
    """[(name, bytes)] of tuples that must fail the TUPLE rule or the walk under WALK"""
    good = T(*GOOD)
    long3 = T(5, 100, Long(b"q" * 40), 7, b"xy", 900)
    at3 = 24 + 16                                                  # column 3 of `good` and `long3`: after int2, pad, int8
    many = bytearray(T(None, 100, b"abc", 7, b"xy", 900))         # HASNULL, hoff 24, one bitmap byte
    struct.pack_into("<H", many, 18, 40)                           # 40 attributes want five bitmap bytes: hoff 32 at least
    return [
        ("len 22", good[:22]),
        ("hoff 16", patched(good, 22, b"\x10")),
        ("hoff 28", patched(good, 22, b"\x1c")),
        ("hoff above len", patched(good, 22, b"\xf8")),
        ("bitmap beyond hoff", bytes(many)),
        ("fixed column one byte past len", good[:-1]),
        ("varlena past len", patched(good, at3, bytes([(100 << 1) | 1]))),
        ("short header at the last byte claims 2", good[:at3] + bytes([(2 << 1) | 1])),
        ("4-byte size of 3", patched(long3, at3, struct.pack("<I", 3 << 2))),
        ("external tag other than 18", T(5, 100, Toast(tag=1), 7, b"xy", 900)),
    ]


def int_values(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return [lo, lo + 1, -1, 0, 1, 99, 100, 101, hi - 1, hi]


def ops_block():
    """one block whose tuples carry every interesting value in the int2, int8 and int4 columns (and a NULL in each)"""
    tuples = []
    for a, b, c in zip(int_values(16), int_values(64), int_values(32)):
        tuples.append(T(a, b, b"t", c, None, 1))
    tuples += [T(None, 100, b"t", 100, None, 1), T(100, None, b"t", 100, None, 1), T(100, 100, b"t", None, None, 1)]
    return tuples


def ops_keys():
    """[(keys, column, values or None)] for all eight ops on all three types at 99 / 100 / 101 and the types' extremes"""
    out = []
    for att, typ, bits in ((1, fr.INT2, 16), (2, fr.INT8, 64), (4, fr.INT4, 32)):
        for op in range(fr.LT, fr.NOTNULL + 1):
            for value in (99, 100, 101, -(1 << (bits - 1)), (1 << (bits - 1)) - 1):
                out.append(([(att, typ, op, value)], att, op, value))
    return out


def ops_expected(att, op, value):
    """positions of ops_block() that must match a key on column att"""
    col = {1: 0, 2: 1, 4: 2}[att]
    rows = [v for v in zip(int_values(16), int_values(64), int_values(32))]
    rows += [(None, 100, 100), (100, None, 100), (100, 100, None)]
    out = []
    for pos, r in enumerate(rows, 1):
        v = r[col]
        if op == fr.ISNULL:
            hit = v is None
        elif op == fr.NOTNULL:
            hit = v is not None
        else:
            hit = v is not None and {fr.LT: v < value, fr.LE: v <= value, fr.EQ: v == value, fr.GE: v >= value, fr.GT: v > value,
                                     fr.NE: v != value}[op]
        if hit:
            out.append(pos)
    return out


def cases():
    out = []
    # a NULL in each position, before and at the key
    nulls = [with_null(i) for i in range(6)] + [T(*GOOD)]
    blk = tc.build_block(B, nulls)
    out.append(("nulls, key on 6", blk, K6, [1, 2, 3, 4, 5, 7], {}))
    out.append(("nulls, key on 4", blk, K4, [1, 2, 3, 5, 6, 7], {}))
    for col in range(1, 7):
        out.append(("ISNULL %d" % col, blk, [(col, 0, fr.ISNULL, 0)], [col], {}))
        out.append(("NOTNULL %d" % col, blk, [(col, 0, fr.NOTNULL, 0)], [p for p in range(1, 8) if p != col], {}))
    # a short text that leaves the following int4 / int8 needing 0 .. 7 pad bytes
    pads = [T(5, 100, b"a" * n, 7, b"b" * m, 900) for n in range(9) for m in range(9)]
    blk = tc.build_block(B, pads[:40])
    out.append(("pads after short texts (1)", blk, K4 + K6, list(range(1, 41)), {}))
    blk = tc.build_block(B, pads[40:])
    out.append(("pads after short texts (2)", blk, K4 + K6, list(range(1, 42)), {}))
    # 4-byte headers: one that needs a pad itself, low bytes of 0 (sizes 64 and 320), a long one in front of the keys
    longs = [T(5, 100, b"a", None, Long(b"z" * 200), 900), T(5, 100, Long(b"z" * 60), 7, b"xy", 900),
             T(5, 100, b"z" * 316, 7, b"z" * 316, 900), T(5, 100, b"abc", 7, Long(b"z" * 60), 901)]
    assert struct.unpack_from("<I", longs[1], 24 + 16)[0] & 0xFF == 0 and struct.unpack_from("<I", longs[2], 24 + 16)[0] & 0xFF == 0
    blk = tc.build_block(B, longs)
    out.append(("4-byte headers", blk, K6, [1, 2, 3], {}))
    out.append(("4-byte headers, key on 4", blk, K4, [2, 3, 4], {}))
    # a TOAST pointer in front of the key; the key column above tnatts; tnatts == 0
    odd = [T(5, 100, Toast(), 7, Toast(), 900), T(5, 100, b"abc"), tc.form_tuple(ATTS, []), T(*GOOD), T(5, 100, b"abc", 7)]
    blk = tc.build_block(B, odd)
    out.append(("toast, short tuples: key on 6", blk, K6, [1, 4], {}))
    out.append(("toast, short tuples: key on 4", blk, K4, [1, 4, 5], {}))
    out.append(("toast, short tuples: 6 is null", blk, [(6, 0, fr.ISNULL, 0)], [2, 3, 5], {}))
    out.append(("toast, short tuples: no key", blk, [], [1, 2, 3, 4, 5], {}))
    # two keys on one column (a range), keys on three columns, four keys
    rng = [T(i, 1000 + i, b"r", 10 * i, b"s", -i) for i in range(1, 31)]
    blk = tc.build_block(B, rng)
    out.append(("range on 4", blk, [(4, fr.INT4, fr.GE, 50), (4, fr.INT4, fr.LT, 120)], list(range(5, 12)), {}))
    out.append(("three columns", blk, [(1, fr.INT2, fr.GT, 3), (2, fr.INT8, fr.LE, 1020), (6, fr.INT8, fr.NE, -7)],
                [p for p in range(4, 21) if p != 7], {}))
    out.append(("four keys", blk, [(1, fr.INT2, fr.GT, 3), (6, fr.INT8, fr.LT, -5), (4, fr.INT4, fr.NE, 80), (5, 0, fr.NOTNULL, 0)],
                [p for p in range(6, 31) if p != 8], {}))
    out.append(("nothing matches", blk, [(4, fr.INT4, fr.GT, 1000)], [], {}))
    # the TUPLE cases: each hits only its own tuple, its neighbours still match
    tuples, bad = [T(*GOOD)], {}
    for name, t in tuple_cases():
        tuples.append(t)
        bad[len(tuples)] = fr.TUPLE
        tuples.append(T(*GOOD))
    blk = tc.build_block(B, tuples)
    out.append(("damaged tuples", blk, WALK, [p for p in range(1, len(tuples) + 1) if p not in bad], bad))
    # with no key the walk visits no column: only the header rule is left
    header_only = ("len 22", "hoff 16", "hoff 28", "hoff above len", "bitmap beyond hoff")
    head = {p: fr.TUPLE for p, (name, _) in zip(sorted(bad), tuple_cases()) if name in header_only}
    out.append(("damaged tuples, no key", blk, [], [p for p in range(1, len(tuples) + 1) if p not in head], head))
    # ITEM, as the fetch's: len 0, off not aligned, off below upper, beyond the block
    base = tc.build_block(B, [T(*GOOD)] * 6)
    upper = int(base[4:8].view("<u4")[0])
    for at, val in ((12, 0), (8, upper + 4), (8, upper - 8), (12, B)):
        x = base.copy()
        x[at + 8:at + 12] = np.frombuffer(struct.pack("<I", val), np.uint8)          # item 2
        out.append(("item %d = %d" % (at, val), x, K6, [1, 3, 4, 5, 6], {2: fr.ITEM}))
    return out


def overlap_block():
    """four items that claim the same large matching tuple, one item of len 0: OVERLAP, and the bad item keeps its record"""
    big = T(5, 100, b"o" * 1300, 7, b"xy", 900)
    slot = tc.maxalign(len(big))
    o = np.zeros(B, np.uint8)
    o[B - slot:B - slot + len(big)] = np.frombuffer(big, np.uint8)
    for i in range(4):
        o[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", B - slot, len(big)), np.uint8)
    o[8 + 8 * 4:16 + 8 * 4] = np.frombuffer(struct.pack("<II", B - slot, 0), np.uint8)
    o[:8] = np.frombuffer(struct.pack("<II", 8 + 8 * 5, B - slot), np.uint8)
    return o


def descriptors():
    """[(name, atts, keys, flags, patch, ok)]: every argument rule of the descriptor.  patch: None, or (which, field, index,
    value) to set a reserved field of the arrays codec.filter_desc makes ("f" the struct itself, "a" atts, "k" keys)"""
    A = ATTS
    int4 = (4, fr.INT4, fr.EQ, 1)
    return [
        ("plain", A, [int4], 0, None, True),
        ("no key", A, [], 0, None, True),
        ("count only", A, [int4], fr.COUNT_ONLY, None, True),
        ("four keys", A, [int4] * 4, 0, None, True),
        ("1600 columns", [(4, 4)] * 1600, [(1600, fr.INT4, fr.EQ, 1)], 0, None, True),
        ("char(n)-like fixed width of 32767", [(32767, 1)], [], 0, None, True),
        ("null tests on any column, type and value ignored", A, [(3, 9, fr.ISNULL, 1 << 40), (5, 0, fr.NOTNULL, -1)], 0, None, True),
        ("extremes", A, [(1, fr.INT2, fr.GE, -32768), (1, fr.INT2, fr.LE, 32767), (4, fr.INT4, fr.GE, -(1 << 31)),
                         (2, fr.INT8, fr.LE, (1 << 63) - 1)], 0, None, True),
        ("int2 key on an int2 column aligned to 4", [(2, 4)], [(1, fr.INT2, fr.EQ, 1)], 0, None, True),
        ("no column", [], [], 0, None, False),
        ("1601 columns", [(4, 4)] * 1601, [], 0, None, False),
        ("five keys", A, [int4] * 5, 0, None, False),
        ("att 0", A, [(0, fr.INT4, fr.EQ, 1)], 0, None, False),
        ("att beyond natts", A, [(7, fr.INT4, fr.EQ, 1)], 0, None, False),
        ("attlen 0", [(0, 4)], [], 0, None, False),
        ("cstring", [(-2, 1)], [], 0, None, False),
        ("attalign 0", [(4, 0)], [], 0, None, False),
        ("attalign 3", [(4, 3)], [], 0, None, False),
        ("attalign 16", [(4, 16)], [], 0, None, False),
        ("varlena aligned to 2", [(-1, 2)], [], 0, None, False),
        ("int4 key on an int8 column", A, [(2, fr.INT4, fr.EQ, 1)], 0, None, False),
        ("int8 key on a text column", A, [(3, fr.INT8, fr.EQ, 1)], 0, None, False),
        ("int8 key on an int8 column aligned to 4", [(8, 4)], [(1, fr.INT8, fr.EQ, 1)], 0, None, False),
        ("unknown type", A, [(4, 4, fr.EQ, 1)], 0, None, False),
        ("type 0", A, [(4, 0, fr.EQ, 1)], 0, None, False),
        ("op 0", A, [(4, fr.INT4, 0, 1)], 0, None, False),
        ("op 9", A, [(4, fr.INT4, 9, 1)], 0, None, False),
        ("int2 value too large", A, [(1, fr.INT2, fr.LT, 32768)], 0, None, False),
        ("int2 value too small", A, [(1, fr.INT2, fr.GT, -32769)], 0, None, False),
        ("int4 value too large", A, [(4, fr.INT4, fr.LT, 1 << 31)], 0, None, False),
        ("int4 value too small", A, [(4, fr.INT4, fr.GT, -(1 << 31) - 1)], 0, None, False),
        ("unknown flag", A, [int4], 2, None, False),
        ("reserved field of the descriptor", A, [int4], 0, ("f", "rsv", 0, 1), False),
        ("reserved field of a column", A, [int4], 0, ("a", "rsv", 5, 1), False),
        ("reserved field of a key", A, [int4], 0, ("k", "rsv", 0, 1), False),
    ]
