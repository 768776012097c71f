"""The hand-made vectors of the grouped-scan tests, shared by the CPU test (what tests/group_ref.py must say about them, with the
expected values written out there) and the GPU test (the kernels against group_ref on the same blocks).  The tuples are crafted
with tests/tuple_craft.py; the aggregate's own blocks (agg_cases) are reused where they fit.  Test infrastructure only."""
import random

import agg_cases as ac
import filter_cases as fc
import filter_ref as fr
import tuple_craft as tc
from filter_ref import INT2, INT4, INT8

I64_MIN, I64_MAX = ac.I64_MIN, ac.I64_MAX
TURN_B = ac.TURN_B                                      # 290 tuples of 40 bytes and their items fit
TURN_SIZES = ac.TURN_SIZES
GX_ATTS = [(4, 4), (8, 8)]                              # (g int4, x int8)
GX_BY, GX_COLS = [(1, INT4)], [(2, INT8)]
GX_KEYS = [(2, INT8, fr.GE, 0)]                         # x >= 0
PATTERNS = ("one", "distinct", "alternate", "runs3")


def runs3(n):
    """group numbers of n positions in runs of three, cut so that a run lies across every multiple of 64: no run starts there"""
    g, p, gid = [], 0, 0
    while p < n:
        ln = 2 if (p + 3) % 64 == 0 else 3
        g += [gid] * min(ln, n - p)
        p += ln
        gid += 1
    return g


def pattern_keys(pattern, m):
    """the group value of each of m matches, in position order"""
    if pattern == "one":
        return [7] * m
    if pattern == "distinct":
        return [1000 - 3 * p for p in range(m)]         # descending: the contract's order is the reverse of the position order
    if pattern == "alternate":
        return [5 if p % 2 == 0 else -5 for p in range(m)]
    if pattern == "straddle":                           # ascending, so a match's place is its position: one run over places 63 .. 65
        return [63 if 63 <= p <= 65 else p for p in range(m)]
    return runs3(m)


def turn_block(pattern, m, interleave=False, atts=GX_ATTS, row=None):
    """m matches (g by the pattern, x = the match's number); interleave: behind every second match a tuple the key rejects, behind
    every seventh a damaged one (its t_hoff is 4).  atts and row: another row type, row(p, g) the values of match p"""
    assert row is None or not interleave
    tuples = []
    for p, g in enumerate(pattern_keys(pattern, m)):
        tuples.append(tc.form_tuple(atts, row(p, g) if row else [g, p]))
        if interleave and p % 2 == 1:
            tuples.append(tc.form_tuple(GX_ATTS, [g, -1]))
        if interleave and p % 7 == 6:
            tuples.append(fc.patched(tc.form_tuple(GX_ATTS, [g, p]), 22, b"\x04"))
    assert len(tuples) <= 290
    return tc.build_block(TURN_B, tuples)


INTERLEAVED_SIZES = tuple(m for m in TURN_SIZES if m + m // 2 + m // 7 <= 290)


ORDER_ATTS = [(8, 8), (4, 4), (2, 2), (8, 8)]           # (a int8, b int4, c int2, x int8)
ORDER_B = 16384
ORDER_VALUES = [I64_MIN, -1, 0, 1, I64_MAX]


def order_block():
    """30 tuples: a takes the five int8 values of ORDER_VALUES six times each in a shuffled position order; b and c take their
    types' extremes and 0 by the position; x = the position"""
    rnd = random.Random(5)
    a = ORDER_VALUES * 6
    rnd.shuffle(a)
    b = [-(1 << 31), (1 << 31) - 1, 0]
    c = [(1 << 15) - 1, -(1 << 15), 0, -1]
    return tc.build_block(ORDER_B, [tc.form_tuple(ORDER_ATTS, [a[p], b[p % 3], c[p % 4], p + 1]) for p in range(30)])


def second_differs_block():
    """12 tuples whose first group column (int8) is the same and whose second (int2) differs: c = 3, -3, 0, 32767, -32768, 3, ..."""
    c = [3, -3, 0, 32767, -32768, 3]
    return tc.build_block(ORDER_B, [tc.form_tuple(ORDER_ATTS, [I64_MAX, 1, c[p % 6], 10 * (p + 1)]) for p in range(12)])


NULL_ATTS = [(4, 4), (4, 4), (8, 8)]                    # (g1 int4, g2 int4, x int8)
NULL_BY2 = [(1, INT4), (2, INT4)]


def nulls_block():
    """all four null patterns of two group columns, NULL by bitmap and by a short natts, x NULL in every row of one group:
      pos  g1    g2    x
       1   5     NULL  10
       2   NULL  5     20
       3   NULL  NULL  NULL    (bitmap)
       4   5     5     40
       5   5     -     -       (natts 1: g2 and x are NULL)
       6   -     -     -       (natts 0: all NULL)
       7   NULL  5     70
       8   5     5     NULL
       9   4     9     90
      10   5     NULL  NULL"""
    F = lambda *v: tc.form_tuple(NULL_ATTS, list(v))    # noqa: E731
    return tc.build_block(ORDER_B, [F(5, None, 10), F(None, 5, 20), F(None, None, None), F(5, 5, 40), F(5), F(), F(None, 5, 70),
                                    F(5, 5, None), F(4, 9, 90), F(5, None, None)])


def descriptors():
    """[(name, atts, keys, by, cols, flags, patch, ok)]: every argument rule of the grouping.  cols None: a null aggregate
    descriptor.  patch: None, or (which, field, index, value) to set a reserved field ("f" the filter struct, "a" atts, "k" keys,
    "r" the group struct, "b" its columns, "g" the aggregate struct, "c" its columns)"""
    A = ac.ATTS
    int4 = (4, INT4, fr.EQ, 1)
    out = [
        ("one group column, one aggregate column", A, [int4], [(4, INT4)], [(2, INT8)], 0, None, True),
        ("two group columns, four aggregate columns", A, [int4], [(1, INT2), (6, INT8)], ac.COLS4, 0, None, True),
        ("no aggregate column", A, [], [(4, INT4)], [], 0, None, True),
        ("a null aggregate descriptor", A, [], [(4, INT4)], None, 0, None, True),
        ("the group column twice", A, [], [(2, INT8), (2, INT8)], [(2, INT8)], 0, None, True),
        ("key, group and aggregate column at once", A, [int4], [(4, INT4)], [(4, INT4)], 0, None, True),
        ("int2 group column aligned to 4", [(2, 4)], [], [(1, INT2)], [], 0, None, True),
        ("group column 1600", [(4, 4)] * 1600, [], [(1600, INT4)], [], 0, None, True),
        ("count only", A, [int4], [(4, INT4)], [(2, INT8)], fr.COUNT_ONLY, None, False),
        ("no group column", A, [int4], [], [(2, INT8)], 0, None, False),
        ("three group columns", A, [], [(4, INT4), (2, INT8), (1, INT2)], [], 0, None, False),
        ("five aggregate columns", A, [], [(4, INT4)], ac.COLS4 + [(2, INT8)], 0, None, False),
        ("group att 0", A, [], [(0, INT4)], [], 0, None, False),
        ("group att beyond natts", A, [], [(7, INT8)], [], 0, None, False),
        ("group type 0", A, [], [(4, 0)], [], 0, None, False),
        ("group type 4", A, [], [(4, 4)], [], 0, None, False),
        ("int4 group on an int8 column", A, [], [(2, INT4)], [], 0, None, False),
        ("int8 group on a text column", A, [], [(3, INT8)], [], 0, None, False),
        ("int8 group column aligned to 4", [(8, 4)], [], [(1, INT8)], [], 0, None, False),
        ("a bad group column behind a good one", A, [], [(2, INT8), (3, INT8)], [], 0, None, False),
        ("a bad aggregate column", A, [], [(4, INT4)], [(2, INT8), (3, INT8)], 0, None, False),
        ("reserved field of the group descriptor", A, [], [(2, INT8)], [], 0, ("r", "rsv", 0, 1), False),
        ("reserved byte of a group column", A, [], [(2, INT8), (4, INT4)], [], 0, ("b", "rsv", 1, 1), False),
        ("reserved word of a group column", A, [], [(2, INT8)], [], 0, ("b", "rsv2", 0, 1), False),
        ("reserved field of the aggregate", A, [], [(2, INT8)], [(2, INT8)], 0, ("g", "rsv", 0, 1), False),
        ("reserved field of an aggregate without columns", A, [], [(2, INT8)], [], 0, ("g", "rsv", 0, 1), False),
        ("reserved byte of an aggregate column", A, [], [(2, INT8)], [(2, INT8), (4, INT4)], 0, ("c", "rsv", 1, 1), False),
    ]
    # the filter's own rules, on a descriptor whose group column is fine
    for name, atts, keys, flags, patch, ok in fc.descriptors():
        if not ok and atts is A and flags == 0:
            out.append(("filter: " + name, atts, keys, [(4, INT4)], [(2, INT8)], flags, patch, False))
    return out


def ref_ok(gr, atts, keys, by, cols, flags, patch):
    """group_ref.desc_ok on a descriptors() entry"""
    kw = {}
    if patch:
        which, _, index, value = patch
        kw = {"f": dict(rsv=value), "a": dict(att_rsv=[0] * index + [value]), "k": dict(key_rsv=[0] * index + [value]),
              "r": dict(grp_rsv=value), "b": dict(by_rsv=[0] * index + [value]),
              "g": dict(agg_rsv=value), "c": dict(col_rsv=[0] * index + [value])}[which]
    return gr.desc_ok(atts, keys, by, cols, flags, **kw)
