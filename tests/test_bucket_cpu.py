"""CPU tests of tests/bucket_ref.py, the reference of the bucketed group columns, against yardsticks that share no code with it:
numpy's datetime64 for days and months, values written out by hand for the floor below the origin, the 64-bit edges and the
infinities, and group_ref on descriptors whose buckets are all NONE."""
import random

import numpy as np

import bucket_ref as bk
import group_cases as gc
import group_ref as gr
from filter_ref import INT2, INT4, INT8

US_PER_DAY = 86_400_000_000
PG_EPOCH_US = 946_684_800_000_000                       # 2000-01-01 00:00 in microseconds since 1970-01-01
I64_MIN, I64_MAX = bk.I64_MIN, bk.I64_MAX


def unix_us(text):
    return int(np.datetime64(text, "us").astype(np.int64))


def test_day_buckets_are_datetime64_days():
    """timestamps as microseconds since 1970: the day bucket from the origin 2000-01-01 is numpy's truncation to [D] -- which
    floors --, for instants after 2000, between 1970 and 2000, and before 1970"""
    rnd = random.Random(1)
    instants = [unix_us(t) for t in ("2024-02-29T23:59:59.999999", "2000-01-01T00:00:00", "1999-12-31T23:59:59.999999",
                                     "1970-01-01T00:00:00", "1969-12-31T23:59:59.999999", "1969-07-20T20:17:40", "1600-03-01T12:00:00")]
    instants += [rnd.randrange(unix_us("1700-01-01"), unix_us("2200-01-01")) for _ in range(2000)]
    for v in instants:
        want = int(np.datetime64(v, "us").astype("datetime64[D]").astype("datetime64[us]").astype(np.int64))
        assert bk.bucket_key(bk.width(PG_EPOCH_US, US_PER_DAY), INT8, v) == want, v
    # PostgreSQL's own representation counts from 2000-01-01: the same instants, origin 0
    for v in instants:
        want = int(np.datetime64(v, "us").astype("datetime64[D]").astype("datetime64[us]").astype(np.int64)) - PG_EPOCH_US
        assert bk.bucket_key(bk.width(0, US_PER_DAY), INT8, v - PG_EPOCH_US) == want, v


def test_floor_and_not_truncation_below_the_origin():
    day = bk.width(0, US_PER_DAY)
    assert bk.bucket_key(day, INT8, -1) == -US_PER_DAY                    # 1999-12-31 23:59:59.999999 is in 1999-12-31
    assert bk.bucket_key(day, INT8, -US_PER_DAY) == -US_PER_DAY and bk.bucket_key(day, INT8, -US_PER_DAY - 1) == -2 * US_PER_DAY
    assert bk.bucket_key(day, INT8, 0) == 0 and bk.bucket_key(day, INT8, US_PER_DAY - 1) == 0
    assert [bk.bucket_key(bk.width(-1, 3), INT2, v) for v in range(-8, 6)] == [-10, -7, -7, -7, -4, -4, -4, -1, -1, -1, 2, 2, 2, 5]
    week = bk.width(2, 7)                                                 # dates as int4 days from 2000-01-01; 2000-01-03 is a Monday
    for d in range(-800, 800):
        date = np.datetime64("2000-01-01") + d
        monday = date - (date.astype("datetime64[D]").view("int64") - 4) % 7   # 1970-01-01 was a Thursday
        assert bk.bucket_key(week, INT4, d) == int((monday - np.datetime64("2000-01-01")).astype(np.int64)), d


def test_month_boundaries_are_datetime64_months():
    """the binder's list for date_trunc('month', ...): the first instant of every month of a range, handed over unsorted and
    with duplicates; a value's key is its datetime64[M]; below the first boundary a value is undecided"""
    months = np.arange(np.datetime64("1968-11"), np.datetime64("1972-03"))
    members = [int(m.astype("datetime64[us]").astype(np.int64)) for m in months]
    shuffled = members + members[::5]
    random.Random(2).shuffle(shuffled)
    b = bk.bounds(shuffled)
    rnd = random.Random(3)
    values = members + [m - 1 for m in members[1:]] + [m + 1 for m in members] + [rnd.randrange(members[0], members[-1]) for _ in range(500)]
    for v in values:
        want = int(np.datetime64(v, "us").astype("datetime64[M]").astype("datetime64[us]").astype(np.int64))
        assert bk.bucket_key(b, INT8, v) == want, v
    assert bk.bucket_key(b, INT8, members[0] - 1) == bk.UNDECIDED and bk.bucket_key(b, INT8, I64_MIN) == bk.UNDECIDED
    assert bk.bucket_key(b, INT8, I64_MAX) == members[-1]                 # at or above the largest
    assert bk.bucket_key(bk.bounds([5, I64_MIN]), INT8, I64_MIN) == I64_MIN and bk.bucket_key(bk.bounds([5, I64_MIN]), INT8, 4) == I64_MIN


def test_edges_of_64_bits():
    assert bk.bucket_key(bk.width(I64_MIN, I64_MAX), INT8, I64_MAX) == I64_MAX - 1   # the difference needs 64 unsigned bits
    assert bk.bucket_key(bk.width(I64_MIN, 1 << 32), INT8, I64_MAX) == I64_MAX - (1 << 32) + 1
    assert bk.bucket_key(bk.width(I64_MAX, I64_MAX), INT8, I64_MIN) == bk.UNDECIDED  # the key would be INT64_MIN - 1
    assert bk.bucket_key(bk.width(I64_MAX, I64_MAX), INT8, I64_MIN + 1) == I64_MIN + 1      # exactly two widths below the origin
    assert bk.bucket_key(bk.width(I64_MAX, I64_MAX), INT8, -I64_MAX + I64_MAX) == 0
    assert bk.bucket_key(bk.width(0, 3), INT8, I64_MIN) == bk.UNDECIDED              # -2^63 is 1 mod 3: the key lies below it
    assert bk.bucket_key(bk.width(0, 3), INT8, I64_MIN + 1) == bk.UNDECIDED          # 2 mod 3
    assert bk.bucket_key(bk.width(0, 3), INT8, I64_MIN + 2) == I64_MIN + 2 == bk.bucket_key(bk.width(0, 3), INT8, I64_MIN + 4)
    assert bk.bucket_key(bk.width(0, 2), INT8, I64_MIN) == I64_MIN
    assert bk.bucket_key(bk.width(0, 1), INT8, I64_MIN) == I64_MIN and bk.bucket_key(bk.width(0, 1), INT8, I64_MAX) == I64_MAX
    assert bk.bucket_key(bk.width(0, 1 << 40), INT4, -5) == -(1 << 40)               # not clamped to the column's type


def test_infinities():
    for typ, bits in ((INT2, 16), (INT4, 32), (INT8, 64)):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        for b in (bk.width(0, 7, bk.INFINITE), bk.bounds([lo, 0, hi], bk.INFINITE)):
            assert bk.bucket_key(b, typ, lo) == lo and bk.bucket_key(b, typ, hi) == hi
            assert bk.bucket_key(b, typ, 15) == (14 if b[0] == bk.WIDTH else 0)
        assert bk.bucket_key(bk.bounds([lo, 0], bk.INFINITE), typ, -1) == bk.UNDECIDED    # a finite value in -infinity's bucket
        assert bk.bucket_key(bk.bounds([lo, 0]), typ, -1) == lo                            # without the flag it is a bucket
        assert bk.bucket_key(bk.bounds([0, hi], bk.INFINITE), typ, hi) == hi
        assert bk.bucket_key(bk.width(hi, 1, bk.INFINITE), typ, hi) == hi
    assert bk.bucket_key(bk.width(0, 1 << 15, bk.INFINITE), INT2, -3) == bk.UNDECIDED     # the key is -32768
    assert bk.bucket_key(bk.width(0, 1 << 15), INT2, -3) == -(1 << 15)
    assert bk.bucket_key(bk.width(0, 1 << 31, bk.INFINITE), INT4, -3) == bk.UNDECIDED     # the key is INT32_MIN
    assert bk.bucket_key(bk.width(0, 1 << 31, bk.INFINITE), INT8, -3) == -(1 << 31)       # which is no extreme of an int8
    assert bk.bucket_key(bk.width(I64_MIN, 5, bk.INFINITE), INT8, I64_MIN + 3) == bk.UNDECIDED
    assert bk.bucket_key(bk.width(I64_MIN, 5), INT8, I64_MIN + 3) == I64_MIN


def test_descriptor_rules():
    ok = [[bk.RAW], [bk.width(0, 1)], [bk.width(I64_MIN, I64_MAX, bk.INFINITE)], [bk.bounds([3, 3, 1])], [bk.bounds(range(1024), 1)]]
    for b in ok:
        assert bk.buckets_ok(b, 1), b
    assert bk.buckets_ok([bk.RAW, bk.width(5, 5)], 2) and not bk.buckets_ok([bk.RAW], 2) and not bk.buckets_ok(None, 1)
    bad = [[(3, 0, 0, 0)], [(255, 0, 0, 0)], [bk.width(0, 0)], [bk.width(0, -1)], [bk.bounds([])], [bk.bounds(range(1025))],
           [(bk.BOUNDS, 0, 1, [1])], [(bk.BOUNDS, 0, 0, None)], [(bk.NONE, 1, 0, 0)], [(bk.NONE, 0, 1, 0)], [(bk.NONE, 0, 0, 1)],
           [bk.width(0, 1, 2)], [bk.width(0, 1, 0x81)], [bk.bounds([1], 4)]]
    for b in bad:
        assert not bk.buckets_ok(b, 1), b
    assert not bk.buckets_ok([bk.width(0, 1)], 1, rsv=[1])


def test_all_none_is_group_ref():
    """with every bucket NONE the reference says what group_ref says, NULL groups and the order included"""
    for blocks, atts, keys, by, cols in (
            ([gc.turn_block(p, m, True) for p in gc.PATTERNS for m in (1, 65)], gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS),
            ([gc.nulls_block(), None], gc.NULL_ATTS, [], gc.NULL_BY2, [(3, INT8)]),
            ([gc.order_block()], gc.ORDER_ATTS, [], [(1, INT8), (3, INT2)], [(4, INT8), (2, INT4)])):
        got, want = bk.group_call(blocks, atts, keys, by, cols, [bk.RAW] * len(by)), gr.group_call(blocks, atts, keys, by, cols)
        assert got[3] == want[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3]))


def test_undecided_matches_count_as_bad():
    blocks = [gc.nulls_block()]
    rows, recs, cells, total = bk.group_call(blocks, gc.NULL_ATTS, [], gc.NULL_BY2, [(3, INT8)], [bk.bounds([5]), bk.width(0, 4)])
    # g1 = 4 (position 9) lies below the only boundary; the NULLs stay NULL groups; g2 = 5 -> 4, 9 -> 8
    assert tuple(rows[0])[:5] == (0, 10, 9, 1, 4) and int(recs["n_rows"].sum()) == 9
    assert [(tuple(r["key"]), int(r["nulls"]), int(r["n_rows"])) for r in recs] == \
        [((5, 4), 0, 2), ((5, 0), 2, 3), ((0, 4), 1, 2), ((0, 0), 3, 2)]
