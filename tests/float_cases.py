"""Hand-made blocks for the float scan keys and float aggregate columns, with their expectations written out by hand: shared by the
CPU test of the reference (test_float_cpu.py) and the GPU tests (test_gpu_float.py, test_gpu_float_host.py).  Float values are
handed to tuple_craft.form_tuple as the signed integer of their bits (float_ref.f4, float_ref.f8).  Test infrastructure only."""
import random
import struct

import float_ref as fl
import tuple_craft as tc
from float_ref import EQ, FLOAT4, FLOAT8, GE, GT, IN, INT4, INT8, ISNULL, LE, LT, NE, NOT_IN, NOTNULL, f4, f8

B = 4096
# (id int4, x float8, y float4, name text, z float4 aligned to 8, k int8, g int2)
ATTS = [(4, 4), (8, 8), (4, 4), (-1, 4), (4, 8), (8, 8), (2, 2)]
INF = float("inf")
NAN = float("nan")
NAN_SIGN = -0x0008000000000000            # 0xFFF8000000000000 as a signed integer: a NaN with the sign bit set
NAN_PAYLOAD = 0x7FF0000000000123          # a signalling NaN with a payload
NAN4_SIGN = -0x00400000                   # 0xFFC00000
NAN4_PAYLOAD = 0x7F800321
SUB8 = 0x0000000000000001                 # the smallest float8 subnormal, 2^-1074
SUB4 = 0x00000001                         # the smallest float4 subnormal, 2^-149
MAX8 = f8(1.7976931348623157e308)
MAX4 = 0x7F7FFFFF                         # 3.4028234663852886e38


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def row(i, x=None, y=None, z=None, k=0, g=0, name=b"n"):
    """a tuple whose float columns are given as Python floats, raw bits (int) or None"""
    def raw(v, four):
        if v is None or isinstance(v, int):
            return v
        return f4(v) if four else f8(v)
    return T(i, raw(x, False), raw(y, True), name, raw(z, True), k, g)


# the special values of a float8 column x at positions 1 .. 12, in a block that every key case below filters
SPECIALS = [0.0, -0.0, INF, -INF, NAN_SIGN, NAN_PAYLOAD, SUB8, f8(-5e-324),
            MAX8, f8(-1.7976931348623157e308), 1.5, None]
# the same for the float4 column y: widened they are the doubles of the same values
SPECIALS4 = [0.0, -0.0, INF, -INF, NAN4_SIGN, NAN4_PAYLOAD, SUB4, f4(-1.401298464324817e-45), MAX4, f4(-3.4028234663852886e38), 1.5, None]


def specials_block():
    return tc.build_block(B, [row(i + 1, SPECIALS[i], SPECIALS4[i], SPECIALS4[i], k=i, g=i % 3) for i in range(12)])


# positions by value, for reading the expectations below: 1 +0, 2 -0, 3 +Inf, 4 -Inf, 5 NaN (sign), 6 NaN (payload), 7 +tiny,
# 8 -tiny, 9 +max, 10 -max, 11 1.5, 12 NULL
KEY_CASES = [
    # (name, op, constant, the positions that match) -- the same for x (float8), y (float4) and z (float4 aligned to 8)
    ("< 0", LT, 0.0, [4, 8, 10]),
    ("<= -0", LE, -0.0, [1, 2, 4, 8, 10]),
    ("= 0", EQ, 0.0, [1, 2]),
    ("<> -0", NE, -0.0, [3, 4, 5, 6, 7, 8, 9, 10, 11]),
    ("> 1", GT, 1.0, [3, 5, 6, 9, 11]),
    (">= 1.5", GE, 1.5, [3, 5, 6, 9, 11]),
    ("< -1", LT, -1.0, [4, 10]),
    ("> -1", GT, -1.0, [1, 2, 3, 5, 6, 7, 8, 9, 11]),
    ("= NaN", EQ, NAN, [5, 6]),
    ("= NaN with a sign and a payload", EQ, -0x0007FFFFFFFFFFFF, [5, 6]),
    ("<> NaN", NE, NAN, [1, 2, 3, 4, 7, 8, 9, 10, 11]),
    ("< NaN", LT, NAN, [1, 2, 3, 4, 7, 8, 9, 10, 11]),
    (">= NaN", GE, NAN, [5, 6]),
    ("> NaN", GT, NAN, []),
    ("<= NaN", LE, NAN, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]),
    ("> +Inf", GT, INF, [5, 6]),
    (">= +Inf", GE, INF, [3, 5, 6]),
    ("< -Inf", LT, -INF, []),
    ("<= -Inf", LE, -INF, [4]),
    ("> 0 finds the subnormal", GT, 0.0, [3, 5, 6, 7, 9, 11]),
]
# keys whose constant lies between values that only one of the widths has
WIDTH_CASES = [
    # (name, key, positions): 2^-1074 is below the float4 subnormal 2^-149; 1e39 is above the largest float4 and below the largest float8
    ("x > 2^-1074", (2, FLOAT8, GT, 5e-324), [3, 5, 6, 9, 11]),
    ("y > 2^-1074", (3, FLOAT4, GT, 5e-324), [3, 5, 6, 7, 9, 11]),
    ("y >= 2^-149 exactly", (3, FLOAT4, GE, 1.401298464324817e-45), [3, 5, 6, 7, 9, 11]),
    ("z = 2^-149 exactly", (5, FLOAT4, EQ, 1.401298464324817e-45), [7]),
    ("y < 1e39", (3, FLOAT4, LT, 1e39), [1, 2, 4, 7, 8, 9, 10, 11]),
    ("x < 1e39", (2, FLOAT8, LT, 1e39), [1, 2, 4, 7, 8, 10, 11]),
    ("y = the largest float4, widened", (3, FLOAT4, EQ, 3.4028234663852886e38), [9]),
    ("x is null", (2, FLOAT8, ISNULL, 0), [12]),
    ("y is not null", (3, 0, NOTNULL, 0), list(range(1, 12))),
]


def cases():
    """[(name, B, atts, block, keys, truth or None, matching positions, {bad position: status})]"""
    out = []
    blk = specials_block()
    for name, op, const, want in KEY_CASES:
        for att, typ in ((2, FLOAT8), (3, FLOAT4), (5, FLOAT4)):
            out.append(("%s on column %d" % (name, att), B, ATTS, blk, [(att, typ, op, const)], None, want, {}))
    for name, key, want in WIDTH_CASES:
        out.append((name, B, ATTS, blk, [key], None, want, {}))
    # two float keys ANDed, and beside an integer key
    out.append(("a range", B, ATTS, blk, [(2, FLOAT8, GE, -1.0), (2, FLOAT8, LT, 2.0)], None, [1, 2, 7, 8, 11], {}))
    out.append(("a float and an integer key", B, ATTS, blk, [(3, FLOAT4, GT, 0.0), (6, INT8, LE, 6)], None, [3, 5, 6, 7], {}))
    # a float key beside a byte-string key and a set key under a truth table: x > 1 OR (name = 'n' AND k IN (0, 7))
    keys = [(2, FLOAT8, GT, 1.0), (4, fl.BYTES, EQ, b"n"), (6, INT8, IN, [0, 7, 99])]
    out.append(("a truth table over a float, a byte-string and a set key", B, ATTS, blk, keys, fl.tr.dnf([1, 6], 3), [1, 3, 5, 6, 8, 9, 11], {}))
    # columns beyond tnatts are NULL; a tuple that ends inside the float column is TUPLE
    short = [tc.form_tuple(ATTS, [1]), tc.form_tuple(ATTS, [2, f8(2.5)]), row(3, 2.5, 1.0, 1.0), tc.form_tuple(ATTS, [4, f8(-2.5)])[:-4]]
    sb = tc.build_block(B, short)
    out.append(("columns beyond tnatts", B, ATTS, sb, [(2, FLOAT8, GT, 0.0)], None, [2, 3], {4: fl.TUPLE}))
    out.append(("a column beyond tnatts is null", B, ATTS, sb, [(3, FLOAT4, ISNULL, 0)], None, [1, 2], {4: fl.TUPLE}))
    return out


def descriptors():
    """[(name, atts, keys, key_rsv or None, accepted)]: the descriptor table of a float key"""
    return [
        ("float4 on (4, 4)", ATTS, [(3, FLOAT4, LT, 1.0)], None, True),
        ("float4 on (4, 8)", ATTS, [(5, FLOAT4, LT, 1.0)], None, True),
        ("float8 on (8, 8)", ATTS, [(2, FLOAT8, NE, NAN)], None, True),
        ("every bit pattern is a constant", ATTS, [(2, FLOAT8, EQ, -1), (3, FLOAT4, EQ, NAN_PAYLOAD)], None, True),
        ("beside byte-string and set keys", ATTS, [(2, FLOAT8, GT, 0.0), (4, fl.BYTES, GE, b"a"), (6, INT8, NOT_IN, [1, 2])], None, True),
        ("a null test ignores the type", ATTS, [(4, FLOAT8, ISNULL, 0)], None, True),
        ("float8 on (8, 4)", [(4, 4), (8, 4)], [(2, FLOAT8, LT, 1.0)], None, False),
        ("float4 on an int8 column", ATTS, [(6, FLOAT4, LT, 1.0)], None, False),
        ("float8 on a float4 column", ATTS, [(3, FLOAT8, LT, 1.0)], None, False),
        ("float4 on a varlena", ATTS, [(4, FLOAT4, LT, 1.0)], None, False),
        ("float8 on a varlena", ATTS, [(4, FLOAT8, EQ, 1.0)], None, False),
        ("a float type with IN", ATTS, [(2, FLOAT8, IN, [1, 2])], None, False),
        ("a float type with NOT IN", ATTS, [(3, FLOAT4, NOT_IN, [1])], None, False),
        ("rsv != 0", ATTS, [(2, FLOAT8, LT, 1.0)], [1], False),
        ("types 10 and 7 stay unknown", ATTS, [(2, 10, LT, 1)], None, False),
    ]


# ---- sums ----
P900, P840, M900 = 2.0 ** 900, 2.0 ** 840, 2.0 ** -900
CANCEL = [P900, P840, 1.0, -P900, M900]    # exact: 2^840 + 1 + 2^-900; plain left-to-right summation loses 2^840
SUM_CASES = [
    # (name, [(position, x or None)], (n, min, max, sum, err) of the aggregate call -- floats, or bit patterns as ints)
    # one lane, four turns apart: the group's order too.  (2^900, 2^840) absorbs the 1; the rest is exact
    ("cancellation in one lane", [(1 + 64 * t, v) for t, v in enumerate(CANCEL)], (5, -P900, P900, P840, M900)),
    # lanes 0 .. 4 of one turn: the butterfly joins (2^900, 2^-900) with 1 -- the tail is lost there -- and 2^840 with -2^900
    ("cancellation across lanes", [(1 + t, v) for t, v in enumerate(CANCEL)], (5, -P900, P900, P840, 0.0)),
    ("only +Inf", [(1, INF), (2, INF), (70, 1.0)], (3, 1.0, INF, INF, 0.0)),
    ("only -Inf", [(3, -INF), (64, -2.0)], (2, -INF, -2.0, -INF, 0.0)),
    ("+Inf with -Inf", [(1, INF), (65, -INF), (2, 5.0)], (3, -INF, INF, fl.NAN_BITS, 0.0)),
    ("a NaN among finite values", [(1, 1.0), (2, NAN_SIGN), (3, -3.0), (130, INF)], (4, -3.0, fl.NAN_BITS, fl.NAN_BITS, 0.0)),
    ("all NaN", [(1, NAN_PAYLOAD), (2, NAN_SIGN)], (2, fl.NAN_BITS, fl.NAN_BITS, fl.NAN_BITS, 0.0)),
    ("an overflow pair", [(1, 1.5e308), (2, 1.5e308)], (2, 1.5e308, 1.5e308, fl.NAN_BITS, fl.NAN_BITS)),
    ("an overflow in one lane", [(1, 1.5e308), (65, 1.5e308), (2, -1.0)], (3, -1.0, 1.5e308, fl.NAN_BITS, fl.NAN_BITS)),
    ("all NULL", [(1, None), (2, None), (66, None)], (0, 0.0, 0.0, 0.0, 0.0)),
    ("zeros come back as +0", [(1, -0.0), (2, -0.0)], (2, 0.0, 0.0, 0.0, 0.0)),
    ("subnormals add exactly", [(1, SUB8), (2, SUB8), (65, SUB8)], (3, 5e-324, 5e-324, 1.5e-323, 0.0)),
    ("the largest values cancel", [(1, MAX8), (2, f8(-1.7976931348623157e308)), (3, 0.25)], (3, -1.7976931348623157e308, 1.7976931348623157e308, 0.25, 0.0)),
]
# the grouped call's (sum, err) where its order gives another pair than the aggregate's butterfly
GROUP_SUMS = {"cancellation across lanes": (P840, M900)}


def words(expect):
    """five unsigned words of a hand-written (n, min, max, sum, err)"""
    return (expect[0],) + tuple(v if isinstance(v, int) else fl.bits_of(v) for v in expect[1:])


def sum_block(values, n_items=None):
    """a block over ATTS whose tuple at position p has x = values[p] (a float, raw bits, or None: NULL), y and z = the float4
    nearest where it is exact, and k = 1 on the listed positions and 0 elsewhere; positions not listed hold x = 1e300"""
    at = dict(values)
    n = n_items or max(at)
    rows = []
    for p in range(1, n + 1):
        if p in at:
            rows.append(row(p, at[p], None, None, k=1, g=p % 2))
        else:
            rows.append(row(p, 1e300, 1.0, 1.0, k=0, g=p % 2))
    return tc.build_block(SUM_B, rows)


SUM_B = 32768                               # 257 tuples of 72 bytes and their item ids
SUM_KEYS = [(6, INT8, EQ, 1)]               # the listed positions alone match
SUM_COLS = [(2, FLOAT8), (1, INT4)]


# ---- blocks of 1, 63, 64, 65 and 290 items ----
def sized_block(n, seed):
    """n items over ATTS (B = SIZED_B; 290 is five turns, the last partial): x a float8 and y, z float4 values of mixed sign and
    magnitude, a NULL in every seventh x, an infinity and a NaN in the larger blocks; k = position, g = position mod 3"""
    rng = random.Random(seed)
    rows = []
    for p in range(1, n + 1):
        x = None if p % 7 == 0 else rng.choice((-1, 1)) * rng.random() * 10.0 ** rng.randint(-30, 30)
        if n > 64 and p == 40:
            x = INF
        if n > 100 and p == 200:
            x = NAN_SIGN
        y = None if p % 11 == 0 else struct.unpack("<f", struct.pack("<f", rng.uniform(-100, 100)))[0]
        rows.append(row(p, x, y, y, k=p, g=p % 3))
    return tc.build_block(SIZED_B, rows)


SIZED_B = 32768
SIZES = (1, 63, 64, 65, 290)
SIZED_KEYS = [(2, FLOAT8, GT, -1e10), (3, FLOAT4, LE, 50.0)]
SIZED_COLS = [(2, FLOAT8), (3, FLOAT4), (6, INT8), (5, FLOAT4)]
SIZED_BY = [(7, fl.INT2)]


# ---- seeded random tuples ----
def random_value(rng, four):
    kind = rng.randrange(12)
    if kind == 0:
        return None
    if kind == 1:
        return rng.choice((0.0, -0.0))
    if kind == 2:
        return rng.choice((INF, -INF)) if rng.randrange(4) == 0 else 1.0
    if kind == 3:
        return (rng.choice((NAN4_SIGN, NAN4_PAYLOAD)) if four else rng.choice((NAN_SIGN, NAN_PAYLOAD))) if rng.randrange(4) == 0 else -1.0
    if kind == 4:
        return rng.choice((1, -1)) * rng.randrange(1, 50) * (1.401298464324817e-45 if four else 5e-324)
    x = rng.choice((-1, 1)) * rng.random() * 2.0 ** rng.randint(-20, 20)
    return struct.unpack("<f", struct.pack("<f", x))[0] if four else x


def random_blocks(n=24, seed=11):
    """n blocks (B = 4 096) of 5 .. 40 random tuples over ATTS; some tuples are cut short"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        rows = []
        for p in range(1, rng.randint(5, 40) + 1):
            t = row(p, random_value(rng, False), random_value(rng, True), random_value(rng, True), k=rng.randint(-5, 5), g=rng.randint(0, 3),
                    name=b"n" * rng.randint(0, 3))
            if rng.randrange(40) == 0:
                t = t[:rng.randint(24, len(t) - 1)]
            rows.append(t)
        out.append(tc.build_block(B, rows))
    return out


def random_descriptors(seed=5, n=10):
    """[(keys, truth or None, aggregate columns)]: one to four keys, at least one of a float type, under a random monotone
    table or ANDed; one to four aggregate columns of mixed integer and float types"""
    rng = random.Random(seed)
    consts = [0.0, -0.0, 1.0, -1.0, NAN, INF, -INF, 5e-324, 0.37, -12.5, 1e-40]
    ops = [LT, LE, EQ, GE, GT, NE]
    pool = [(2, FLOAT8), (3, FLOAT4), (5, FLOAT4), (6, INT8), (1, INT4), (7, fl.INT2)]
    out = []
    for i in range(n):
        nk = rng.randint(1, 4)
        keys = []
        for k in range(nk):
            att, typ = rng.choice(pool[:3]) if k == 0 else rng.choice(pool)
            if fl.is_float(typ):
                keys.append((att, typ, rng.choice(ops), rng.choice(consts)))
            elif rng.randrange(3) == 0:
                keys.append((att, typ, rng.choice((ISNULL, NOTNULL)), 0))
            else:
                keys.append((att, typ, rng.choice(ops), rng.randint(-3, 3)))
        truth = None if i % 3 == 0 else rng.choice(fl.tr.monotone_tables(nk))
        cols = [rng.choice(pool) for _ in range(rng.randint(1, 4))]
        if i % 2 == 0 and not any(fl.is_float(t) for _, t in cols):
            cols[0] = pool[i % 3]
        out.append((keys, truth, cols))
    return out
