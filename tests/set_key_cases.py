"""The hand-made vectors of the set-key tests (CRYO_OP_IN, CRYO_OP_NOT_IN), shared by the CPU test (what tests/set_key_ref.py must
say about them) and the GPU tests (the kernels against set_key_ref on the same blocks), the descriptor table, and the seeded
generator of the property test.  The tuples are crafted with tests/tuple_craft.py over the descriptor (int4 id, text tag, int8
big, int2 small, int4 app): every keyed column but the first lies behind a varlena.  Test infrastructure only.

cases() yields (name, B, atts, block, keys, matches, bad): matches the positions that must match, bad {position: status}.  The
expectations are written out by hand or follow from how the block was made (a probe value is put at a known position because
it is, or is not, a member); none comes from the reference."""
import random

import set_key_ref as sr
import tuple_craft as tc
from tuple_craft import Toast

B = 4096
ATTS = [(4, 4), (-1, 4), (8, 8), (2, 2), (4, 4)]
LINEAR = 8                                   # sets up to this many distinct members are scanned by the kernels, larger ones searched
SIZES = (1, 2, 3, LINEAR, LINEAR + 1, 63, 64, 65, 1023, 1024)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def members(n, step=7):
    """n distinct members, ascending, `step` apart, about half of them negative"""
    return [step * (i - n // 2) for i in range(n)]


def as_given(sorted_members):
    """the list a caller would hand over: out of order, and with the first and the last member repeated where 1 024 leaves room"""
    n = len(sorted_members)
    stride = next(s for s in (389, 5, 3, 2, 1) if n % s or s == 1)       # coprime to n: a permutation
    out = [sorted_members[(i * stride + n // 3) % n] for i in range(n)]
    assert sorted(out) == sorted_members
    return (out + [sorted_members[-1], sorted_members[0]])[:sr.SET_MAX]


def probes(m):
    """[(value or None, is a member)] around the ascending members m: the first, a middle and the last member, one below the
    smallest, one above the largest, strictly between two neighbours, and a NULL"""
    out = [(m[0], True), (m[len(m) // 2], True), (m[-1], True), (m[0] - 1, False), (m[-1] + 1, False), (None, False)]
    if len(m) > 1:
        out += [(m[0] + 3, False), (m[len(m) // 2 - 1] + 3, False), (m[-2] + 3, False)]
    return out


def big_block():
    """290 items at B = 16 384 over (int4 id, int4 app), app = id % 11 - 5: hits and misses of {-5, 0, 3} in each of the five turns"""
    atts = [(4, 4), (4, 4)]
    return atts, tc.build_block(16384, [tc.form_tuple(atts, [i, i % 11 - 5]) for i in range(1, 291)])


BIG_KEYS = [(2, sr.INT4, sr.IN, [3, 0, -5, 3, 77])]
BIG_MATCHES = [i for i in range(1, 291) if i % 11 in (0, 5, 8)]


def cases():
    out = []

    def add(name, tuples, keys, matches, bad=None, atts=ATTS, size=B):
        out.append((name, size, atts, tc.build_block(size, tuples), keys, matches, bad or {}))

    # every set size: the probes on the int4 column behind the text, both ops
    for n in SIZES:
        m = members(n)
        pv = probes(m)
        tuples = [T(i, b"t" * (i % 5), 10, 1, v) for i, (v, _) in enumerate(pv, 1)]
        given = as_given(m)
        add("%d members, IN" % n, tuples, [(5, sr.INT4, sr.IN, given)], [i for i, (v, hit) in enumerate(pv, 1) if hit])
        add("%d members, NOT IN" % n, tuples, [(5, sr.INT4, sr.NOT_IN, given)],
            [i for i, (v, hit) in enumerate(pv, 1) if not hit and v is not None])
    # a list of 1 024 entries that are three values
    few = [T(1, b"", 0, 0, 5), T(2, b"", 0, 0, -5), T(3, b"", 0, 0, 6), T(4, b"", 0, 0, 0), T(5, b"", 0, 0, 4)]
    add("1 024 entries, three distinct", few, [(5, sr.INT4, sr.IN, [5, -5, 0, 0] * 256)], [1, 2, 4])
    # signed order on an int8 column, its extremes among the members
    wide = [T(1, b"ab", I64_MIN, 0, 0), T(2, b"ab", I64_MAX, 0, 0), T(3, b"ab", -1, 0, 0), T(4, b"ab", 0, 0, 0), T(5, b"ab", I64_MIN + 1, 0, 0),
            T(6, b"ab", I64_MAX - 1, 0, 0), T(7, b"ab", 1 << 32, 0, 0), T(8, b"ab", -(1 << 32), 0, 0), T(9, b"ab", None, 0, 0)]
    ext = [I64_MAX, -1, I64_MIN, 1 << 32]
    add("int8 extremes, IN", wide, [(3, sr.INT8, sr.IN, ext)], [1, 2, 3, 7])
    add("int8 extremes, NOT IN", wide, [(3, sr.INT8, sr.NOT_IN, ext)], [4, 5, 6, 8])
    add("int8, twelve members around zero", wide, [(3, sr.INT8, sr.IN, [I64_MIN + 1, -(1 << 32), -3, -2, 0, 2, 3, 4, 5, 6, 7, I64_MAX - 1])],
        [4, 5, 6, 8])
    # members outside the column type's range equal no value: int2 against 32 768 and -32 769, int4 against 2^31 and 2^32 + 5
    narrow = [T(1, b"", 0, -32768, 5), T(2, b"", 0, 32767, -(1 << 31)), T(3, b"", 0, 5, (1 << 31) - 1), T(4, b"", 0, 0, 0), T(5, b"", 0, -1, -1)]
    add("int2: members out of range match nothing", narrow, [(4, sr.INT2, sr.IN, [32768, -32769])], [])
    add("int2: members out of range, NOT IN", narrow, [(4, sr.INT2, sr.NOT_IN, [32768, -32769])], [1, 2, 3, 4, 5])
    add("int2: one member in range", narrow, [(4, sr.INT2, sr.IN, [32768, 5, -32769, 65535, -32768])], [1, 3])
    add("int4: members out of range", narrow, [(5, sr.INT4, sr.IN, [1 << 31, (1 << 32) + 5, (1 << 32) - 1, -(1 << 31)])], [2])
    # combinations
    rows = [T(i, b"p", 100 + i, i % 3, i) for i in range(1, 13)]
    add("two sets on one column: the intersection", rows, [(5, sr.INT4, sr.IN, [2, 4, 6, 8, 10]), (5, sr.INT4, sr.IN, [9, 8, 4, 3, 1])], [4, 8])
    add("IN and NOT IN of one set", rows, [(5, sr.INT4, sr.IN, [2, 4, 6]), (5, sr.INT4, sr.NOT_IN, [6, 4, 2])], [])
    add("a set beside a range on another column", rows, [(5, sr.INT4, sr.IN, [2, 3, 5, 7, 11]), (3, sr.INT8, sr.GE, 105), (3, sr.INT8, sr.LT, 111)],
        [5, 7])
    add("sets on three columns", rows, [(5, sr.INT4, sr.NOT_IN, [1, 2, 3]), (3, sr.INT8, sr.IN, [104, 105, 106, 109, 112]),
                                       (4, sr.INT2, sr.IN, [0, 2]), (1, sr.INT4, sr.NOT_IN, [6])], [5, 9, 12])
    # NULLs and columns beyond tnatts: neither op matches
    nulls = [T(1, b"p", 1, 1, None), T(2, b"p", 1, 1, 7), T(3, b"p", 1), T(4, b"p", 1, 1, 8), T(5, None, None, None, 7), tc.form_tuple(ATTS, [])]
    add("a NULL and a missing column: IN", nulls, [(5, sr.INT4, sr.IN, [7])], [2, 5])
    add("a NULL and a missing column: NOT IN", nulls, [(5, sr.INT4, sr.NOT_IN, [7])], [4])
    add("a NULL is in no set, ISNULL finds it", nulls, [(5, sr.INT4, sr.NOT_IN, [7]), (3, 0, sr.ISNULL, 0)], [])
    # beside a comparison, a null test and a byte-string key, with an undecided tuple: no match wins over undecided; the walk
    # goes to the highest key column whatever the set said (a damaged column 5 behind a false set key on column 3 is TUPLE)
    hurt = T(7, b"de", 5, 1, 9)[:-2]
    mix = [T(1, b"de", 5, 1, 9), T(2, Toast(), 5, 1, 9), T(3, Toast(), 6, 1, 9), T(4, b"fr", 5, 1, 9), T(5, b"de", 5, None, 9),
           T(6, b"de", 5, 1, 3), hurt, T(8, b"de", 7, 1, 9)]
    keys = [(3, sr.INT8, sr.IN, [7, 5, 5]), (2, sr.BYTES, sr.EQ, b"de"), (4, 0, sr.NOTNULL, 0), (5, sr.INT4, sr.GT, 4)]
    add("a set, a byte string, a null test and a comparison", mix, keys, [1, 8], {2: sr.UNDECIDED, 7: sr.TUPLE})
    keys = [(3, sr.INT8, sr.NOT_IN, [7, 5, 5]), (2, sr.BYTES, sr.EQ, b"de"), (5, sr.INT4, sr.GT, 4)]
    add("NOT IN beside an undecided value", mix, keys, [], {3: sr.UNDECIDED, 7: sr.TUPLE})
    add("NOT IN true beside an undecided value", mix, [(3, sr.INT8, sr.NOT_IN, [5]), (2, sr.BYTES, sr.NE, b"de")], [], {3: sr.UNDECIDED})
    # 290 items, five turns of the wave
    atts, blk = big_block()
    out.append(("290 items", 16384, atts, blk, BIG_KEYS, BIG_MATCHES, {}))
    return out


def descriptors():
    """[(name, atts, keys, key_rsv or None, ok)]: the argument rules of a set key, and the pinned refusals of
    tests/filter_cases.py and tests/bytes_key_cases.py beside them.  key_rsv: the rsv fields to set after codec.filter_desc made
    the arrays; a set value of None: a null address"""
    A = ATTS
    one = [1, 2, 3]
    return [
        ("IN on an int4 column", A, [(5, sr.INT4, sr.IN, one)], None, True),
        ("NOT IN on an int8 column", A, [(3, sr.INT8, sr.NOT_IN, one)], None, True),
        ("IN on an int2 column", A, [(4, sr.INT2, sr.IN, one)], None, True),
        ("one member", A, [(5, sr.INT4, sr.IN, [4])], None, True),
        ("1 024 members", A, [(5, sr.INT4, sr.IN, list(range(1024)))], None, True),
        ("four sets of 1 024 members", A, [(5, sr.INT4, sr.IN, list(range(1024)))] * 2 + [(3, sr.INT8, sr.NOT_IN, list(range(1024)))] * 2, None, True),
        ("members outside the type's range", A, [(4, sr.INT2, sr.IN, [32768, -32769, I64_MIN, I64_MAX])], None, True),
        ("beside a byte-string key, a comparison and a null test", A,
         [(5, sr.INT4, sr.IN, one), (2, sr.BYTES, sr.EQ, b"abc"), (1, sr.INT4, sr.GT, 0), (3, 0, sr.NOTNULL, 0)], None, True),
        ("no member", A, [(5, sr.INT4, sr.IN, one)], [0], False),
        ("1 025 members", A, [(5, sr.INT4, sr.IN, list(range(1025)))], None, False),
        ("a count of 2^32 - 1", A, [(5, sr.INT4, sr.IN, one)], [0xFFFFFFFF], False),
        ("a null address", A, [(5, sr.INT4, sr.NOT_IN, None)], [3], False),
        ("type BYTES", A, [(2, sr.BYTES, sr.IN, one)], None, False),
        ("type 0", A, [(5, 0, sr.IN, one)], None, False),
        ("type 4", A, [(5, 4, sr.IN, one)], None, False),
        ("an int4 set on the int8 column", A, [(3, sr.INT4, sr.IN, one)], None, False),
        ("an int8 set on the text column", A, [(2, sr.INT8, sr.IN, one)], None, False),
        ("an int4 column aligned to 2", [(4, 2)], [(1, sr.INT4, sr.IN, one)], None, False),
        ("column 0", A, [(0, sr.INT4, sr.IN, one)], None, False),
        ("column 6 of 5", A, [(6, sr.INT4, sr.IN, one)], None, False),
        ("op 11", A, [(5, sr.INT4, 11, 1)], None, False),
        ("op 11 with a count", A, [(5, sr.INT4, 11, 1)], [1], False),
        ("five keys", A, [(5, sr.INT4, sr.IN, one)] * 5, None, False),
        # pinned by tests/filter_cases.py and tests/bytes_key_cases.py: they stay refused
        ("op 9 on an integer key made as a comparison", A, [(1, sr.INT4, 9, 1)], None, False),
        ("op 9 with a byte-string constant", A, [(2, sr.BYTES, 9, b"abc")], None, False),
        ("a length on an integer comparison", A, [(1, sr.INT4, sr.EQ, 1)], [1], False),
        ("a length on a null test", A, [(5, sr.INT4, sr.IN, one), (3, 0, sr.ISNULL, 0)], [3, 3], False),
    ]


# ---- the seeded property test ----
SEED = 20261018
TURNS = len(SIZES)
DOMAIN = 48                                  # the keyed columns hold values in [-DOMAIN, DOMAIN]


def _value(rng, lo, hi, p_null=0.07):
    return None if rng.random() < p_null else rng.randint(lo, hi)


def random_tuple(rng, rowid):
    tag = rng.random()
    tag = None if tag < 0.05 else Toast() if tag < 0.09 else bytes(rng.choice(b"ab") for _ in range(rng.choice((0, 1, 2, 2, 5, 9))))
    vals = [rowid, tag, _value(rng, -DOMAIN, DOMAIN), _value(rng, -DOMAIN, DOMAIN), _value(rng, -DOMAIN, DOMAIN)]
    return tc.form_tuple(ATTS, vals[:rng.choice((5, 5, 5, 5, 5, 5, 4, 3))])


def random_blocks(seed=SEED):
    """64 blocks of up to 39 random tuples"""
    rng = random.Random(seed)
    blocks = []
    for k in range(64):
        blocks.append(tc.build_block(B, [random_tuple(rng, 100 * k + i) for i in range(rng.randrange(20, 40))]))
    return blocks


def random_set(rng, n):
    """n distinct members, about half of them (at most 60) from the columns' domain, the rest scattered on either side of it, as
    a caller's list: shuffled, with repeats where there is room"""
    inside = rng.sample(range(-DOMAIN, DOMAIN + 1), min((n + 1) // 2, 60))
    outside = set()
    while len(outside) < n - len(inside):
        v = rng.randint(DOMAIN + 1, 1 << rng.choice((8, 20, 40, 62)))
        outside.add(v if rng.random() < 0.5 else -v)
    out = inside + sorted(outside)
    out += [rng.choice(out) for _ in range(min(rng.randrange(3), sr.SET_MAX - n))]
    rng.shuffle(out)
    return out


def random_keys(rng, n):
    """one to four keys, the first a set of n distinct members; the others sets of any size class, comparisons, null tests
    and byte-string keys"""
    col = {3: sr.INT8, 4: sr.INT2, 5: sr.INT4}
    att = rng.choice((3, 4, 5))
    keys = [(att, col[att], rng.choice((sr.IN, sr.IN, sr.NOT_IN)), random_set(rng, n))]
    for _ in range(rng.choice((0, 1, 1, 2, 3))):
        kind = rng.random()
        att = rng.choice((3, 4, 5))
        if kind < 0.3:
            keys.append((att, col[att], rng.choice((sr.IN, sr.NOT_IN)), random_set(rng, rng.choice(SIZES))))
        elif kind < 0.6:
            keys.append((att, col[att], rng.choice((sr.GE, sr.LE, sr.NE)), rng.randint(-DOMAIN // 2, DOMAIN // 2) * rng.choice((-1, 1))))
        elif kind < 0.8:
            keys.append((rng.choice((2, 4, 5)), 0, rng.choice((sr.ISNULL, sr.NOTNULL, sr.NOTNULL)), 0))
        else:
            keys.append((2, sr.BYTES, rng.choice((sr.GE, sr.NE, sr.LT)), bytes(rng.choice(b"ab") for _ in range(rng.randrange(3)))))
    rng.shuffle(keys)
    return keys


def random_key_sets(seed=SEED):
    """TURNS key sets: every size class of SIZES leads one of them"""
    rng = random.Random(seed + 1)
    return [random_keys(rng, SIZES[t % len(SIZES)]) for t in range(TURNS)]


def size_class(key):
    return len(set(key[3]))


def coverage(blocks, key_sets):
    """by the reference alone: ({size class: [tuples whose non-NULL value a set key of that class found among its members, found
    not among them]}, total matches, tuples some set key rejected on a non-NULL value)"""
    seen, matches, rejected = {}, 0, 0
    for keys in key_sets:
        last = max(k[0] for k in keys)
        sets = [k for k in keys if sr.is_set_key(k)]
        for blk in blocks:
            status, n, items = sr.br._items(blk)
            for pos, bad, off, ln in items:
                data = blk[off:off + ln].tobytes()
                w = None if bad else sr.br.walk(data, ATTS, last)
                if w is None:
                    continue
                refused = False
                for att, typ, op, value in sets:
                    isnull, at, _ = w[att - 1]
                    if isnull:
                        continue
                    among = sr.ar._value(data, at, typ) in value
                    seen.setdefault(len(set(value)), [0, 0])[0 if among else 1] += 1
                    refused = refused or among != (op == sr.IN)
                rejected += refused
                matches += sr.tuple_verdict(data, ATTS, keys)[0] == sr.OK
    return seen, matches, rejected
