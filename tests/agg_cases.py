"""The hand-made vectors of the scan-aggregate tests, shared by the CPU test (what tests/agg_ref.py must say about them, with the
expected values written out there) and the GPU test (the kernel against agg_ref on the same blocks).  The tuples are crafted with
tests/tuple_craft.py, mostly over filter_cases' descriptor (int2, int8, text, int4, text, int8).  Test infrastructure only."""
import numpy as np

import filter_cases as fc
import filter_ref as fr
import tuple_craft as tc
from filter_ref import INT2, INT4, INT8

B = fc.B
ATTS = fc.ATTS
T = fc.T
COLS4 = [(2, INT8), (1, INT2), (6, INT8), (4, INT4)]
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
EXT_ATTS = [(8, 8), (4, 4), (2, 2)]                     # the extremes' descriptor: one column per type
EXT_COLS = [(1, INT8), (2, INT4), (3, INT2)]
EXT_B = 16384                                           # 290 tuples of 38 bytes and their items fit


def range_block():
    """30 tuples whose integer columns all depend on i = 1 .. 30: (i, 1000 + i, "r", 10 i, "s", -i)"""
    return tc.build_block(B, [T(i, 1000 + i, b"r", 10 * i, b"s", -i) for i in range(1, 31)])


RANGE_KEYS = [(4, INT4, fr.GE, 50), (4, INT4, fr.LT, 120)]          # i = 5 .. 11


def nulls_block():
    """a NULL in each column in turn, then a tuple without one (filter_cases' block)"""
    return tc.build_block(B, [fc.with_null(i) for i in range(6)] + [T(*fc.GOOD)])


def short_block():
    """tuples whose natts ends before the later columns: a TOAST pointer twice, three columns, none, all six, four"""
    return tc.build_block(B, [T(5, 100, tc.Toast(), 7, tc.Toast(), 900), T(5, 100, b"abc"), tc.form_tuple(ATTS, []), T(*fc.GOOD),
                              T(5, 100, b"abc", 7)])


def all_null_block():
    """every tuple matches a key on column 4 and is NULL in column 2"""
    return tc.build_block(B, [T(i, None, b"n", 7, b"m", i) for i in range(1, 9)])


def cut_block():
    """good tuples around one cut a byte short of its last column (an int8): columns 1 .. 5 still fit"""
    good = T(*fc.GOOD)
    return tc.build_block(B, [good, good[:-1], good])


def damaged_block():
    """every damaged tuple of filter_cases between good ones; returns (block, positions of the damaged ones)"""
    tuples, bad = [T(*fc.GOOD)], []
    for _, t in fc.tuple_cases():
        tuples.append(t)
        bad.append(len(tuples))
        tuples.append(T(*fc.GOOD))
    return tc.build_block(B, tuples), bad


def bad_item_block():
    """six good tuples; item 2 has len 0"""
    x = tc.build_block(B, [T(*fc.GOOD)] * 6)
    x[12 + 8:16 + 8] = 0
    return x


def header_block():
    x = tc.build_block(B, [T(*fc.GOOD)] * 3)
    x[0:4] = np.frombuffer((12).to_bytes(4, "little"), np.uint8)          # lower = 12: not 8 + 8 n
    return x


def extremes_blocks():
    """[(name, block)]: 290 tuples (int8, int4, int2) all at the types' minima, all at the maxima, and alternating"""
    lo, hi = (I64_MIN, -(1 << 31), -(1 << 15)), (I64_MAX, (1 << 31) - 1, (1 << 15) - 1)
    out = []
    for name, pick in (("min", lambda i: lo), ("max", lambda i: hi), ("mix", lambda i: hi if i % 2 == 0 else lo)):
        out.append((name, tc.build_block(EXT_B, [tc.form_tuple(EXT_ATTS, list(pick(i))) for i in range(290)])))
    return out


TURN_ATTS = [(4, 4)]
TURN_B = 16384
TURN_SIZES = (0, 1, 63, 64, 65, 128, 129, 290)


def turn_blocks():
    """[(n, block, marked positions)]: n int4 tuples; the ones in the first and the last lane of each turn of 64 items, and the
    block's last item, carry 1000 + position, the others their position"""
    out = []
    for n in TURN_SIZES:
        marked = [p for p in range(1, n + 1) if (p - 1) % 64 in (0, 63) or p == n]
        tuples = [tc.form_tuple(TURN_ATTS, [1000 + p if p in marked else p]) for p in range(1, n + 1)]
        out.append((n, tc.build_block(TURN_B, tuples), marked))
    return out


TURN_KEYS = [(1, INT4, fr.GE, 1000)]


def descriptors():
    """[(name, atts, keys, cols, flags, patch, ok)]: every argument rule of the aggregate.  patch: None, or (which, field, index,
    value) to set a reserved field ("f" the filter struct, "a" atts, "k" keys, "g" the aggregate struct, "c" its columns)"""
    A = ATTS
    int4 = (4, INT4, fr.EQ, 1)
    out = [
        ("one column", A, [int4], [(2, INT8)], 0, None, True),
        ("no key", A, [], [(4, INT4)], 0, None, True),
        ("four columns", A, [int4], COLS4, 0, None, True),
        ("the same column twice", A, [], [(2, INT8), (2, INT8)], 0, None, True),
        ("a column that carries a key", A, [int4], [(4, INT4)], 0, None, True),
        ("int2 column aligned to 4", [(2, 4)], [], [(1, INT2)], 0, None, True),
        ("column 1600", [(4, 4)] * 1600, [], [(1600, INT4)], 0, None, True),
        ("count only", A, [int4], [(2, INT8)], fr.COUNT_ONLY, None, False),
        ("unknown flag", A, [int4], [(2, INT8)], 2, None, False),
        ("no column", A, [int4], [], 0, None, False),
        ("five columns", A, [int4], COLS4 + [(2, INT8)], 0, None, False),
        ("att 0", A, [], [(0, INT4)], 0, None, False),
        ("att beyond natts", A, [], [(7, INT8)], 0, None, False),
        ("type 0", A, [], [(4, 0)], 0, None, False),
        ("type 4", A, [], [(4, 4)], 0, None, False),
        ("int4 on an int8 column", A, [], [(2, INT4)], 0, None, False),
        ("int8 on a text column", A, [], [(3, INT8)], 0, None, False),
        ("int8 on an int4 column", A, [], [(4, INT8)], 0, None, False),
        ("int8 column aligned to 4", [(8, 4)], [], [(1, INT8)], 0, None, False),
        ("a bad column behind a good one", A, [], [(2, INT8), (3, INT8)], 0, None, False),
        ("reserved field of the aggregate", A, [], [(2, INT8)], 0, ("g", "rsv", 0, 1), False),
        ("reserved byte of a column", A, [], [(2, INT8), (4, INT4)], 0, ("c", "rsv", 1, 1), False),
        ("reserved word of a column", A, [], [(2, INT8)], 0, ("c", "rsv2", 0, 1), False),
    ]
    # the filter's own rules, on a descriptor whose aggregate column is fine
    for name, atts, keys, flags, patch, ok in fc.descriptors():
        if not ok and atts is A and flags == 0:
            out.append(("filter: " + name, atts, keys, [(4, INT4)], flags, patch, False))
    return out


def ref_ok(ar, atts, keys, cols, flags, patch):
    """agg_ref.desc_ok on a descriptors() entry"""
    kw = {}
    if patch:
        which, _, index, value = patch
        kw = {"f": dict(rsv=value), "a": dict(att_rsv=[0] * index + [value]), "k": dict(key_rsv=[0] * index + [value]),
              "g": dict(agg_rsv=value), "c": dict(col_rsv=[0] * index + [value])}[which]
    return ar.desc_ok(atts, keys, cols, flags, **kw)
