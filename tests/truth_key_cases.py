"""The hand-made vectors of the truth-table tests (CRYO_FILTER_TRUTH), shared by the CPU test (what tests/truth_key_ref.py must say
about them) and the GPU tests (the kernels against truth_key_ref on the same blocks), the descriptor table, the block that
realises every combination of key states, and the seeded generator of the property test.  The tuples are crafted with
tests/tuple_craft.py over set_key_cases' descriptor (int4 id, text tag, int8 big, int2 small, int4 app).  Test infrastructure only.

cases() yields (name, B, atts, block, keys, truth, matches, bad): matches the positions that must match, bad {position: status}.
The expectations are written out by hand or follow from how the block was made; none comes from the reference.  A table is
written as the OR of its terms (tr.dnf: each term the mask of the keys it ANDs, bit k keys[k])."""
import itertools
import random

import truth_key_ref as tr
import tuple_craft as tc
import walk_gen as wg
from set_key_cases import ATTS, B, T, big_block
from tuple_craft import Toast

OR2 = tr.dnf([0b01, 0b10], 2)                                   # A OR B: 0b1110


def mix():
    """(id, tag, big, small, app): the tag in line, external (undecided), NULL; the last tuple is cut within column 5"""
    hurt = T(6, b"de", 5, 1, 3)[:-2]
    return [T(1, b"de", 5, 1, 9), T(2, Toast(), 5, 1, 3), T(3, Toast(), 6, 1, 9), T(4, b"fr", 5, 1, 3), T(5, Toast(), None, 1, 3), hurt]


BIG_KEYS = [(2, tr.INT4, tr.IN, [-5, 3]), (1, tr.INT4, tr.GE, 280), (2, tr.INT4, tr.EQ, 0)]
BIG_TRUTH = tr.dnf([0b001, 0b110], 3)                           # app IN (-5, 3) OR (id >= 280 AND app = 0)
BIG_MATCHES = [i for i in range(1, 291) if i % 11 in (0, 8) or (i >= 280 and i % 11 == 5)]      # app = id % 11 - 5


def cases():
    out = []

    def add(name, tuples, keys, truth, matches, bad=None, atts=ATTS, size=B):
        out.append((name, size, atts, tc.build_block(size, tuples), keys, truth, matches, bad or {}))

    rows = [T(i, b"p", 100 + i, i % 3, i) for i in range(1, 13)]
    add("OR of two integer keys", rows, [(5, tr.INT4, tr.LE, 2), (3, tr.INT8, tr.GE, 111)], OR2, [1, 2, 11, 12])
    # A: app >= 4, B: app <= 6, C: small = 0 (rows 3, 6, 9, 12)
    add("(A AND B) OR C", rows, [(5, tr.INT4, tr.GE, 4), (5, tr.INT4, tr.LE, 6), (4, tr.INT2, tr.EQ, 0)], tr.dnf([0b011, 0b100], 3),
        [3, 4, 5, 6, 9, 12])
    # A: app >= 4, B: small = 0, C: big IN (105, 107, 112)
    add("A AND (B OR C)", rows, [(5, tr.INT4, tr.GE, 4), (4, tr.INT2, tr.EQ, 0), (3, tr.INT8, tr.IN, [112, 105, 107])],
        tr.dnf([0b011, 0b101], 3), [5, 6, 7, 9, 12])
    add("the same keys ANDed by the AND table", rows, [(5, tr.INT4, tr.GE, 4), (4, tr.INT2, tr.EQ, 0), (3, tr.INT8, tr.IN, [112, 105, 107])],
        tr.and_table(3), [12])
    # tuple 6 has three columns: small and app are missing, so NULL
    nulls = [T(1, b"p", None, 1, 7), T(2, b"p", 5, 1, None), T(3, b"p", None, 1, None), T(4, b"p", 5, 1, 7), T(5, b"p", 6, 1, 8), T(6, b"p", 5)]
    add("OR with a NULL column on either side", nulls, [(3, tr.INT8, tr.EQ, 5), (5, tr.INT4, tr.EQ, 7)], OR2, [1, 2, 4, 6])
    add("ISNULL OR a comparison", nulls, [(3, 0, tr.ISNULL, 0), (5, tr.INT4, tr.EQ, 8)], OR2, [1, 3, 5])
    # a byte-string key undecided (tuples 2, 3, 5) beside a true key: a match; beside a false key: UNDECIDED; tuple 6 is damaged in
    # column 5 and TUPLE although its tag alone makes the OR true
    by_tag = [(2, tr.BYTES, tr.EQ, b"de"), (5, tr.INT4, tr.EQ, 3)]
    add("undecided OR a key: a true key decides", mix(), by_tag, OR2, [1, 2, 4, 5], {3: tr.UNDECIDED, 6: tr.TUPLE})
    add("undecided AND a key: a false key decides", mix(), by_tag, tr.and_table(2), [], {2: tr.UNDECIDED, 5: tr.UNDECIDED, 6: tr.TUPLE})
    # (tag = 'de' AND app = 3) OR big = 5: tuple 3 has app 9 and big 6 (no match whatever the tag is), tuple 5 app 3 and a NULL big
    add("undecided under an AND inside an OR", mix(), by_tag + [(3, tr.INT8, tr.EQ, 5)], tr.dnf([0b011, 0b100], 3), [1, 2, 4],
        {5: tr.UNDECIDED, 6: tr.TUPLE})
    add("two undecided keys on one value", mix(), [(2, tr.BYTES, tr.GE, b"de"), (2, tr.BYTES, tr.LT, b"dz"), (5, tr.INT4, tr.EQ, 9)],
        tr.dnf([0b011, 0b100], 3), [1, 3], {2: tr.UNDECIDED, 5: tr.UNDECIDED, 6: tr.TUPLE})
    # app IN (2, 4, 40) OR small NOT IN (0, 1): small = 2 in rows 2, 5, 8, 11
    add("set keys under OR", rows, [(5, tr.INT4, tr.IN, [40, 2, 4]), (4, tr.INT2, tr.NOT_IN, [0, 1])], OR2, [2, 4, 5, 8, 11])
    add("constant true: keys that nothing passes", mix(), [(5, tr.INT4, tr.EQ, 1000), (2, tr.BYTES, tr.EQ, b"zz")], 0b1111, [1, 2, 3, 4, 5],
        {6: tr.TUPLE})
    add("a table that ignores its second key", mix(), [(5, tr.INT4, tr.EQ, 3), (2, tr.BYTES, tr.EQ, b"zz")], 0b1010, [2, 4, 5], {6: tr.TUPLE})
    atts, blk = big_block()
    out.append(("290 items", 16384, atts, blk, BIG_KEYS, BIG_TRUTH, BIG_MATCHES, {}))
    return out


def descriptors():
    """[(name, atts, keys, flags, rsv, ok for the filter)]: the rules of the flag and the table, the older refusals beside them"""
    A = ATTS
    a, b = (5, tr.INT4, tr.GE, 1), (3, tr.INT8, tr.LT, 9)
    return [
        ("OR of two", A, [a, b], tr.TRUTH, 0b1110, True),
        ("the AND table", A, [a, b], tr.TRUTH, 0b1000, True),
        ("constant true", A, [a, b], tr.TRUTH, 0b1111, True),
        ("the first key alone", A, [a, b], tr.TRUTH, 0b1010, True),
        ("one key", A, [a], tr.TRUTH, 0b10, True),
        ("one key, constant true", A, [a], tr.TRUTH, 0b11, True),
        ("four keys, A AND B AND (C OR D)", A, [a, b, a, b], tr.TRUTH, tr.dnf([0b0111, 0b1011], 4), True),
        ("four keys, all ones", A, [a, b, a, b], tr.TRUTH, 0xFFFF, True),
        ("with COUNT_ONLY", A, [a, b], tr.TRUTH | tr.COUNT_ONLY, 0b1110, True),
        ("no key", A, [], tr.TRUTH, 1, False),
        ("table 0", A, [a, b], tr.TRUTH, 0, False),
        ("a bit beyond 2^nkeys", A, [a, b], tr.TRUTH, 0b11110, False),
        ("bit 16 of four keys", A, [a, b, a, b], tr.TRUTH, 0x18000, False),
        ("bit 31", A, [a, b], tr.TRUTH, 0x80000000 | 0b1110, False),
        ("XOR", A, [a, b], tr.TRUTH, 0b0110, False),
        ("NOR", A, [a, b], tr.TRUTH, 0b0001, False),
        ("A AND NOT B", A, [a, b], tr.TRUTH, 0b0010, False),
        ("NOT A", A, [a], tr.TRUTH, 0b01, False),
        ("five keys", A, [a] * 5, tr.TRUTH, 1 << 31, False),
        ("flag 2 beside the flag", A, [a, b], tr.TRUTH | 2, 0b1110, False),
        ("flag 8 beside the flag", A, [a, b], tr.TRUTH | 8, 0b1110, False),
        # as before the flag existed
        ("flags 2", A, [a, b], 2, 0, False),
        ("rsv 1 without the flag", A, [a, b], 0, 1, False),
        ("a table without the flag", A, [a, b], tr.COUNT_ONLY, 0b1110, False),
        ("five keys without the flag", A, [a] * 5, 0, 0, False),
        ("no flag", A, [a, b], 0, 0, True),
    ]


# ---- every combination of key states ----
STATE_ATTS = [(4, 4), (-1, 4), (-1, 4), (4, 4), (8, 8)]           # (int4 id, text s1, text s2, int4 x, int8 y)
STATE_B = 32768
STATE_KEYS = [(2, tr.BYTES, tr.EQ, b"de"), (3, tr.BYTES, tr.GE, b"m"), (4, tr.INT4, tr.LT, 0), (5, tr.INT8, tr.IN, [7, 1 << 40, -7])]
_TEXT1 = {tr.T: b"de", tr.F: b"fr", tr.U: Toast(), None: None}
_TEXT2 = {tr.T: b"nn", tr.F: tc.Long(b"a"), tr.U: Toast(), None: None}
_X = {tr.T: -4, tr.F: 4, None: None}
_Y = {tr.T: 1 << 40, tr.F: 8, None: None}


def state_block():
    """(block, [the four keys' states per item]): 290 items over STATE_ATTS whose tuples run through the 4 x 4 x 3 x 3 = 144
    combinations of (s1, s2: T, F, U, NULL; x, y: T, F, NULL) -- a NULL is F to these keys -- twice, and two items more"""
    combos = list(itertools.product((tr.T, tr.F, tr.U, None), (tr.T, tr.F, tr.U, None), (tr.T, tr.F, None), (tr.T, tr.F, None)))
    assert len(combos) == 144
    tuples, states = [], []
    for i in range(290):
        s1, s2, x, y = combos[(i * 37) % 144]                    # 37 is coprime to 144: every turn of 64 lanes is a mixture
        tuples.append(tc.form_tuple(STATE_ATTS, [i + 1, _TEXT1[s1], _TEXT2[s2], _X[x], _Y[y]]))
        states.append([s or tr.F for s in (s1, s2, x, y)])
    return tc.build_block(STATE_B, tuples), states


def state_expect(states, W):
    """by construction: (positions that match, {position: UNDECIDED}) of the state block under W"""
    v = [tr.verdict_of(s, W) for s in states]
    return [p for p, s in enumerate(v, 1) if s == tr.OK], {p: s for p, s in enumerate(v, 1) if s == tr.UNDECIDED}


# ---- the seeded property test: random keys and random tables on the wide random tuples of tests/walk_gen.py ----
SEED = 20261019
PROPERTY_CASES = ["bitmap-edges", "varlena-8", "random-64", "random-17", "random-9"]
DESCS_PER_CASE = 6


def _present(rows, c):
    return [r[c - 1] for r in rows if len(r) >= c and r[c - 1] is not None]


def random_key(rng, atts, rows):
    """a key of any kind on a column that can carry it: a comparison, a null test, a byte-string key, a set key"""
    ints = [c for c in range(1, len(atts) + 1) if wg.is_int(atts[c - 1])]
    texts = [c for c in range(1, len(atts) + 1) if atts[c - 1][0] == -1]
    kind = rng.random()
    if kind < 0.2:
        return (rng.randint(1, len(atts)), 0, rng.choice((tr.ISNULL, tr.NOTNULL)), 0)
    if kind < 0.55 and texts:
        c = rng.choice(texts)
        inline = [v.payload if isinstance(v, tc.Long) else v for v in _present(rows, c) if isinstance(v, (bytes, tc.Long))]
        const = rng.choice(inline) if inline and rng.random() < 0.5 else rng.choice((b"", b"a", b"ab", b"b", b"\xe9"))
        return (c, tr.BYTES, rng.choice((tr.LT, tr.LE, tr.EQ, tr.GE, tr.GT, tr.NE)), const[:200])
    c = rng.choice(ints)
    typ = wg.INT_TYPE[atts[c - 1][0]]
    seen = _present(rows, c) or [0]
    if kind < 0.8:
        return (c, typ, rng.choice((tr.LT, tr.LE, tr.EQ, tr.GE, tr.GT, tr.NE)), rng.choice(seen))
    members = [rng.choice(seen) for _ in range(rng.choice((1, 3, 9, 20)))] + [wg.draw_fixed(rng, atts[c - 1][0])]
    return (c, typ, rng.choice((tr.IN, tr.NOT_IN)), members)


def property_descriptors(seed=SEED):
    """[(case name, keys, table)]: per case DESCS_PER_CASE descriptors of 1 .. 4 random keys, the first of every second one a
    byte-string key, with a random valid table of that many keys"""
    rng = random.Random(seed)
    tables = {n: tr.monotone_tables(n) for n in range(1, 5)}
    out = []
    for name in PROPERTY_CASES:
        case = wg.case(name)
        texts = [c for c in range(1, len(case.call_atts) + 1) if case.call_atts[c - 1][0] == -1]
        for d in range(DESCS_PER_CASE):
            n = 1 + (d + rng.randrange(2)) % 4
            keys = [random_key(rng, case.call_atts, case.rows) for _ in range(n)]
            if d % 2 == 0 and texts:
                keys[0] = (rng.choice(texts), tr.BYTES, rng.choice((tr.NE, tr.GE, tr.LT)), rng.choice((b"a", b"b", b"")))
            out.append((name, keys, rng.choice(tables[n])))
    return out


def property_coverage(descs):
    """by the reference alone: (descriptors with at least one UNDECIDED tuple, descriptors with a tuple that an OR decided -- a
    match with a false or undecided key, or no match with every decided key true --, all matches, number of keys seen)"""
    undecided = or_decided = matches = 0
    for name, keys, W in descs:
        case = wg.case(name)
        u = o = False
        for blk in case.blocks:
            for it in blk.items:
                states = tr.key_states(case.item_bytes(it), case.call_atts, keys)
                if states is None:
                    continue
                v = tr.verdict_of(states, W)
                u = u or v == tr.UNDECIDED
                o = o or (v == tr.OK and set(states) != {tr.T}) or (v == tr.NOMATCH and tr.F not in states)
                matches += v == tr.OK
        undecided += u
        or_decided += o
    return undecided, or_decided, matches, {len(k) for _, k, _ in descs}
