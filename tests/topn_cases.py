"""The hand-made vectors of the ordered-scan tests, shared by the CPU test (what tests/topn_ref.py must say about them) and the GPU
test (the kernels against topn_ref on the same blocks).  The tuples are crafted with tests/tuple_craft.py over the descriptor (int4
id, int8 k, int2 s, float8 x, float4 y, text name).  Test infrastructure only.

cases() yields (name, B, atts, block, keys, by, cols, order, keys_at): `order` is the positions of ALL the block's matches in the
contract's order, written out by hand -- a call with a limit keeps its first min(limit, len) --, and keys_at {position: (key 1, key
2, key_nulls)} names records whose keys are worth spelling."""
import struct

import bytes_key_ref as br
import filter_ref as fr
import float_ref as fl
import tuple_craft as tc
from tuple_craft import Toast

B = 4096
ATTS = [(4, 4), (8, 8), (2, 2), (8, 8), (4, 4), (-1, 4)]
ID, K, S, X, Y, NAME = 1, 2, 3, 4, 5, 6
DESC, NULLS_FIRST = 1, 2
FLAG_SETS = (0, DESC, NULLS_FIRST, DESC | NULLS_FIRST)
COLS = [ID, K]                                                         # the row: "<i4xq"
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
LIMITS = (1, 2, 63, 64, 65, 289, 290, 291, 1000)


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def f8(x):
    """the float8 x as the signed integer tuple_craft stores"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def s64(u):
    return u - (1 << 64) if u >> 63 else u


def s32(u):
    return u - (1 << 32) if u >> 31 else u


def row(i, k):
    return struct.pack("<i4xq", i, 0 if k is None else k)


def cases():
    out = []

    def add(name, tuples, keys, by, order, keys_at=None, cols=COLS):
        out.append((name, B, ATTS, tc.build_block(B, tuples), keys, by, cols, order, keys_at or {}))

    def ks(values):
        return [T(i + 1, v) for i, v in enumerate(values)]

    # every key equal: position order, whatever the flags
    for fl_ in FLAG_SETS:
        add("all equal, flags %d" % fl_, ks([7] * 5), [], [(K, fr.INT8, fl_)], [1, 2, 3, 4, 5])
    add("ascending input", ks([1, 2, 3, 4, 5]), [], [(K, fr.INT8, 0)], [1, 2, 3, 4, 5])
    add("ascending input, DESC", ks([1, 2, 3, 4, 5]), [], [(K, fr.INT8, DESC)], [5, 4, 3, 2, 1], {5: (5, 0, 0)})
    add("descending input", ks([5, 4, 3, 2, 1]), [], [(K, fr.INT8, 0)], [5, 4, 3, 2, 1])
    add("descending input, DESC", ks([5, 4, 3, 2, 1]), [], [(K, fr.INT8, DESC)], [1, 2, 3, 4, 5])
    # one column with NULLs (by bitmap) under the four flag sets
    nl = ks([3, None, 1, None, 2])
    add("nulls, ASC NULLS LAST", nl, [], [(K, fr.INT8, 0)], [3, 5, 1, 2, 4], {2: (0, 0, 1), 3: (1, 0, 0)})
    add("nulls, DESC NULLS LAST", nl, [], [(K, fr.INT8, DESC)], [1, 5, 3, 2, 4])
    add("nulls, ASC NULLS FIRST", nl, [], [(K, fr.INT8, NULLS_FIRST)], [2, 4, 3, 5, 1])
    add("nulls, DESC NULLS FIRST", nl, [], [(K, fr.INT8, DESC | NULLS_FIRST)], [2, 4, 1, 5, 3])
    # two columns (s, k): (1, 10), (0, 20), (1, 5), (0, NULL), (NULL, 1), (1, 10)
    two = [T(i + 1, k, s) for i, (s, k) in enumerate(((1, 10), (0, 20), (1, 5), (0, None), (None, 1), (1, 10)))]
    add("two columns, both plain", two, [], [(S, fr.INT2, 0), (K, fr.INT8, 0)], [2, 4, 3, 1, 6, 5],
        {4: (0, 0, 2), 5: (0, 1, 1), 6: (1, 10, 0)})
    add("two columns, DESC and DESC NULLS FIRST", two, [], [(S, fr.INT2, DESC), (K, fr.INT8, DESC | NULLS_FIRST)], [1, 6, 3, 4, 2, 5])
    add("two columns, NULLS FIRST and DESC", two, [], [(S, fr.INT2, NULLS_FIRST), (K, fr.INT8, DESC)], [5, 2, 4, 1, 6, 3])
    add("two columns, DESC NULLS FIRST and NULLS FIRST", two, [], [(S, fr.INT2, DESC | NULLS_FIRST), (K, fr.INT8, NULLS_FIRST)],
        [5, 3, 1, 6, 4, 2])
    # the same column twice
    add("the same column twice", ks([2, 1, 2]), [], [(K, fr.INT8, 0), (K, fr.INT8, DESC)], [2, 1, 3])
    # the negation trap: -INT64_MIN does not exist
    ext = ks([0, I64_MIN, I64_MAX, -1, 1])
    add("int8 extremes, ASC", ext, [], [(K, fr.INT8, 0)], [2, 4, 1, 5, 3])
    add("int8 extremes, DESC", ext, [], [(K, fr.INT8, DESC)], [3, 5, 1, 4, 2], {2: (I64_MIN, 0, 0), 3: (I64_MAX, 0, 0)})
    # sign extension of the narrower types
    add("int2 sign extension", [T(i + 1, 0, s) for i, s in enumerate((-1, 1, -32768, 32767, 0))], [], [(S, fr.INT2, 0)],
        [3, 1, 5, 2, 4], {3: (-32768, 0, 0)})
    add("int4 sign extension", [T(v, 0) for v in (-1, 1, -(1 << 31), (1 << 31) - 1, 0)], [], [(ID, fr.INT4, 0)],
        [3, 1, 5, 2, 4], {3: (-(1 << 31), 0, 0)})
    # NULL beyond the tuple's natts: the second tuple has one column
    add("null beyond natts", [T(1, 5), T(2), T(3, 1)], [], [(K, fr.INT8, 0)], [3, 1, 2], {2: (0, 0, 1)})
    add("null beyond natts, NULLS FIRST", [T(1, 5), T(2), T(3, 1)], [], [(K, fr.INT8, NULLS_FIRST)], [2, 3, 1])
    for fl_ in FLAG_SETS:
        add("all null, flags %d" % fl_, ks([None] * 4), [], [(K, fr.INT8, fl_)], [1, 2, 3, 4], {1: (0, 0, 1)})
    # floats: NaNs of two payloads (one with the sign bit) tie, -0 = +0, the infinities
    nan_a, nan_b = s64(0x7FF8000000000001), s64(0xFFF0000000000123)
    xs = [nan_a, f8(1.0), f8(-0.0), nan_b, f8(0.0), f8(float("-inf")), f8(float("inf")), f8(-1.5)]
    flo = [T(i + 1, 0, 0, x) for i, x in enumerate(xs)]
    add("float8, ASC", flo, [], [(X, fl.FLOAT8, 0)], [6, 8, 3, 5, 2, 7, 1, 4],
        {1: (I64_MAX, 0, 0), 4: (I64_MAX, 0, 0), 3: (0, 0, 0), 6: (s64(0xFFF0000000000000 ^ 0x7FFFFFFFFFFFFFFF), 0, 0),
         2: (0x3FF0000000000000, 0, 0)})
    add("float8, DESC", flo, [], [(X, fl.FLOAT8, DESC)], [1, 4, 7, 2, 3, 5, 8, 6])
    # float4 subnormals: 2^-149, -2^-149, 0, the smallest normal, -0; the float8 column holds the same values widened, and
    # ordering by it gives the same order and the same keys
    y4 = [1, s32(0x80000001), 0, 0x00800000, s32(0x80000000)]
    x8 = [f8(2.0 ** -149), f8(-(2.0 ** -149)), f8(0.0), f8(2.0 ** -126), f8(-0.0)]
    sub = [T(i + 1, 0, 0, x, y) for i, (x, y) in enumerate(zip(x8, y4))]
    sub_keys = {1: (0x36A0000000000000, 0, 0), 2: (s64(0xB6A0000000000000 ^ 0x7FFFFFFFFFFFFFFF), 0, 0), 5: (0, 0, 0),
                4: (0x3810000000000000, 0, 0)}
    add("float4 subnormals", sub, [], [(Y, fl.FLOAT4, 0)], [2, 3, 5, 1, 4], sub_keys)
    add("the same values as float8", sub, [], [(X, fl.FLOAT8, 0)], [2, 3, 5, 1, 4], sub_keys)
    add("float4 subnormals, DESC", sub, [], [(Y, fl.FLOAT4, DESC)], [4, 1, 3, 5, 2])
    # ---- filter kinds over one set of tuples: k = 50, 40, 30, 20, 10, 60 with names a .. f, ordered by k DESC ----
    named = [T(i + 1, k, i, f8(k / 4), 0, bytes([97 + i])) for i, k in enumerate((50, 40, 30, 20, 10, 60))]
    by = [(K, fr.INT8, DESC)]
    add("filter: integer range", named, [(K, fr.INT8, fr.GE, 20), (K, fr.INT8, fr.LT, 60)], by, [1, 2, 3, 4])
    add("filter: set key", named, [(ID, fr.INT4, fl.IN, [2, 5, 6, 99])], by, [6, 2, 5])
    add("filter: float key", named, [(X, fl.FLOAT8, fl.GT, 7.5)], by, [6, 1, 2])
    add("filter: byte-string key", named, [(NAME, br.BYTES, fl.GE, b"c")], by, [6, 3, 4, 5])
    return out


def truth_case():
    """(keys, truth table, order) over the `named` tuples: id <= 2 OR k = 10 -- positions 1, 2, 5 --, ordered by k DESC"""
    import pg_cryogen_amd.codec as cc
    keys = [(ID, fr.INT4, fr.LE, 2), (K, fr.INT8, fr.EQ, 10)]
    return keys, cc.truth_dnf([1, 2], 2), [1, 2, 5]


def named_block(undecided=False):
    """the tuples of the filter-kind cases; undecided: the name of position 3 is an external pointer, which a byte-string key
    cannot decide"""
    names = [bytes([97 + i]) for i in range(6)]
    if undecided:
        names[2] = Toast()
    return tc.build_block(B, [T(i + 1, k, i, f8(k / 4), 0, names[i]) for i, k in enumerate((50, 40, 30, 20, 10, 60))])


def bad_items_block():
    """six tuples ordered by k; position 2 has a bad t_hoff (TUPLE) and item 4 a length of 0 (ITEM): in n_bad, in no ranking"""
    tuples = [T(i + 1, k) for i, k in enumerate((5, 9, 3, 8, 1, 7))]
    bad = bytearray(tuples[1])
    bad[22] = 28
    tuples[1] = bytes(bad)
    block = tc.build_block(B, tuples)
    block[8 + 8 * 3 + 4:8 + 8 * 3 + 8] = 0
    return block                                                        # by k ASC: positions 5, 3, 1, 6


def header_block():
    x = tc.build_block(B, [T(i, i) for i in range(1, 4)])
    x[0:4] = list((12).to_bytes(4, "little"))                           # lower = 12: not 8 + 8 n
    return x


# ---- the turns of a wave: n tuples (id p, k (p * 37) mod 101 - 50, so keys repeat; every fifth k NULL) ----
TURN_B = 16384
TURN_SIZES = (0, 1, 63, 64, 65, 128, 129, 290)
TURN_ATTS = [(4, 4), (8, 8)]
TURN_COLS = [1, 2]


def turn_block(n):
    return tc.build_block(TURN_B, [tc.form_tuple(TURN_ATTS, [p, None if p % 5 == 0 else (p * 37) % 101 - 50]) for p in range(1, n + 1)])


def descriptors():
    """[(name, atts, keys, by, limit, cols, patch, ok)]: every argument rule the order adds, and the projection's and the filter's
    through it.  patch: None or (which, index, value) for a reserved field ("b" an order column's rsv, "c" a projected column's
    rsv, "p" the projection's)"""
    A = ATTS
    k8 = (K, fr.INT8, 0)
    return [
        ("one column", A, [], [k8], 1, COLS, None, True),
        ("two columns, every flag", A, [], [(S, fr.INT2, 3), (X, fl.FLOAT8, 1)], 10, COLS, None, True),
        ("float4", A, [], [(Y, fl.FLOAT4, 2)], 10, COLS, None, True),
        ("limit above 290", A, [], [k8], 1000, COLS, None, True),
        ("order column, projected column and key at once", A, [(K, fr.INT8, fr.GT, 0)], [k8], 5, [K], None, True),
        ("the same column twice", A, [], [k8, (K, fr.INT8, 1)], 5, COLS, None, True),
        ("int2 aligned to 4", [(2, 4)], [], [(1, fr.INT2, 0)], 5, [1], None, True),
        ("no order column", A, [], [], 5, COLS, None, False),
        ("three order columns", A, [], [k8, k8, k8], 5, COLS, None, False),
        ("limit 0", A, [], [k8], 0, COLS, None, False),
        ("att 0", A, [], [(0, fr.INT8, 0)], 5, COLS, None, False),
        ("att beyond natts", A, [], [(7, fr.INT8, 0)], 5, COLS, None, False),
        ("attlen not the type's size", A, [], [(K, fr.INT4, 0)], 5, COLS, None, False),
        ("float4 on an int8 column", A, [], [(K, fl.FLOAT4, 0)], 5, COLS, None, False),
        ("attalign below attlen", [(8, 4)], [], [(1, fr.INT8, 0)], 5, [1], None, False),
        ("type 0", A, [], [(K, 0, 0)], 5, COLS, None, False),
        ("a byte-string order column", A, [], [(NAME, br.BYTES, 0)], 5, COLS, None, False),
        ("unknown flag bit", A, [], [(K, fr.INT8, 4)], 5, COLS, None, False),
        ("reserved word of an order column", A, [], [k8], 5, COLS, ("b", 0, 1), False),
        ("a bad column behind a good one", A, [], [k8, (K, fr.INT8, 8)], 5, COLS, None, False),
        ("no projected column", A, [], [k8], 5, [], None, False),
        ("a varlena projected column", A, [], [k8], 5, [NAME], None, False),
        ("reserved word of a projected column", A, [], [k8], 5, COLS, ("c", 1, 1), False),
        ("reserved field of the projection", A, [], [k8], 5, COLS, ("p", 0, 1), False),
        ("five keys", A, [(K, fr.INT8, fr.GT, 0)] * 5, [k8], 5, COLS, None, False),
    ]


def ref_ok(tr, atts, keys, by, limit, cols, patch):
    """topn_ref.desc_ok on a descriptors() entry"""
    kw = {}
    if patch:
        which, index, value = patch
        at = [0] * index + [value]
        kw = {"b": dict(by_rsv=at), "c": dict(col_rsv2=at), "p": dict(prj_rsv=value)}[which]
    return tr.desc_ok(atts, keys, by, limit, cols, **kw)
