"""The hand-made vectors of the byte-string key tests, shared by the CPU test (what tests/bytes_key_ref.py must say about them)
and the GPU tests (the kernels against bytes_key_ref on the same blocks).  The tuples are crafted with tests/tuple_craft.py over
the descriptor (int4, text, text, int8, text); the byte-string keys sit on column 3 (behind a short text, so that its payload
starts anywhere) and on column 5.  Test infrastructure only.

cases() yields (name, B, atts, block, keys, matches, bad): matches the positions that must match, bad {position: status}.  The
expectations of the small cases are written out by hand; those of the length sweep come from Python's own ordering of bytes
objects, which is the contract's (unsigned bytes, then the shorter first) and shares no code with the reference."""
import struct

import bytes_key_ref as br
import tuple_craft as tc
from tuple_craft import Long, Toast

B = 4096
ATTS = [(4, 4), (-1, 4), (-1, 4), (8, 8), (-1, 4)]
LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 32, 126, 127, 255, 256)
OPS = (br.LT, br.LE, br.EQ, br.GE, br.GT, br.NE)


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def K3(op, const):
    return (3, br.BYTES, op, const)


def compressed(t, payload):
    """the tuple t with the 4-byte header of its Long(payload) column turned into a compressed one: low bits 10, size as it was"""
    head = struct.pack("<I", (len(payload) + 4) << 2)
    at = t.index(head + payload)
    assert t.count(head + payload) == 1 and at % 4 == 0
    return t[:at] + struct.pack("<I", (len(payload) + 4) << 2 | 2) + t[at + 4:]


def pattern(n):
    """n bytes that differ from place to place and use the high bit"""
    return bytes((37 * i + 11) % 256 for i in range(n))


def length_tuples(n):
    """[payload] around the constant pattern(n): one shorter, equal, one longer, and a first difference -- lower and higher -- at
    byte 0, 7, 8 and the last byte, where the constant has them"""
    c = pattern(n)
    out = [c, c + b"\x00", c + b"\xff"]
    if n:
        out.append(c[:-1])
    for at in sorted({0, 7, 8, n - 1}):
        if 0 <= at < n:
            for d in (-1, 1):
                if 0 <= c[at] + d <= 255:
                    out.append(c[:at] + bytes([c[at] + d]) + c[at + 1:])
    return out


def by_python(payloads, op, const):
    """the positions whose payload (None: NULL) stands in relation `op` to const, by Python's ordering of bytes"""
    test = {br.LT: lambda p: p < const, br.LE: lambda p: p <= const, br.EQ: lambda p: p == const, br.GE: lambda p: p >= const,
            br.GT: lambda p: p > const, br.NE: lambda p: p != const}[op]
    return [i for i, p in enumerate(payloads, 1) if p is not None and test(p)]


def big_block():
    """290 items at B = 16 384: every 17th an external pointer, the others 'k0' / 'k1' / 'k2' by position: matches and undecided
    tuples in each of the five turns"""
    atts = [(4, 4), (-1, 4)]
    tuples = [tc.form_tuple(atts, [i, Toast() if i % 17 == 0 else b"k" + bytes([48 + i % 3])]) for i in range(1, 291)]
    return atts, tc.build_block(16384, tuples)


def cases():
    out = []

    def add(name, tuples, keys, matches, bad=None, atts=ATTS, size=B):
        out.append((name, size, atts, tc.build_block(size, tuples), keys, matches, bad or {}))

    # all six ops for c < 0, c = 0, c > 0; a proper prefix either way; an empty payload; a NULL
    ops = [T(1, b"p", b"l", 10, b"t"), T(2, b"p", b"m", 10, b"t"), T(3, b"p", b"n", 10, b"t"), T(4, b"p", b"", 10, b"t"),
           T(5, b"p", b"ma", 10, b"t"), T(6, b"p", None, 10, b"t")]
    for op, want in ((br.LT, [1, 4]), (br.LE, [1, 2, 4]), (br.EQ, [2]), (br.GE, [2, 3, 5]), (br.GT, [3, 5]), (br.NE, [1, 3, 4, 5])):
        add("op %d against 'm'" % op, ops, [K3(op, b"m")], want)
    add("'ma' is longer than its prefix 'm'", ops, [K3(br.GT, b"m"), K3(br.LT, b"mb")], [5])
    add("the constant 'mab' is longer than its prefix 'ma'", ops, [K3(br.LT, b"mab"), K3(br.GT, b"m")], [5])
    # unsigned order
    uns = [T(1, b"p", b"\x7f", 10, b"t"), T(2, b"p", b"\x80", 10, b"t"), T(3, b"p", b"\x00", 10, b"t"), T(4, b"p", b"\xff", 10, b"t")]
    add("0x7F sorts before 0x80", uns, [K3(br.LT, b"\x80")], [1, 3])
    add("0x80 sorts after 0x7F", uns, [K3(br.GT, b"\x7f")], [2, 4])
    add("0x00 sorts before 0xFF", uns, [K3(br.LT, b"\xff")], [1, 2, 3])
    add("0xFF sorts after 0x00", uns, [K3(br.GT, b"\x00")], [1, 2, 4])
    # the empty constant
    emp = [T(1, b"p", b"", 10, b"t"), T(2, b"p", b"a", 10, b"t"), T(3, b"p", None, 10, b"t"), T(4, b"p", Long(b""), 10, b"t")]
    add("empty = empty", emp, [K3(br.EQ, b"")], [1, 4])
    add("nothing is below empty", emp, [K3(br.LT, b"")], [])
    add("'a' > empty", emp, [K3(br.GT, b"")], [2])
    add("every value >= empty, a NULL is not", emp, [K3(br.GE, b"")], [1, 2, 4])
    # the constant's lengths: payloads one shorter, equal, one longer, first differences at byte 0, 7, 8 and the last
    for n in LENGTHS:
        payloads = length_tuples(n)
        tuples = [T(i, b"p" * (i % 9), p, 10, b"t") for i, p in enumerate(payloads, 1)]
        for op in OPS:
            add("length %d, op %d" % (n, op), tuples, [K3(op, pattern(n))], by_python(payloads, op, pattern(n)))
    # placement: the payload starts at every offset mod 8; the same content under a 1-byte and a 4-byte header; 127 bytes and more
    place = [T(i, b"p" * i, b"needle", 10, b"t") for i in range(9)] + [T(i, b"p" * i, Long(b"needle"), 10, b"t") for i in range(9)]
    place += [T(1, b"p" * i, b"needlf", 10, b"t") for i in range(9)]
    add("every offset, both headers: =", place, [K3(br.EQ, b"needle")], list(range(1, 19)))
    add("every offset, both headers: >", place, [K3(br.GT, b"needle")], list(range(19, 28)))
    q = b"q" * 126
    longs = [T(1, b"pp", q, 10, b"t"), T(2, b"pp", q + b"q", 10, b"t"), T(3, b"p", q + b"qqqq", 10, b"t"), T(4, b"", Long(q), 10, b"t")]
    add("126 bytes keep a 1-byte header, 127 take four", longs, [K3(br.EQ, q)], [1, 4])
    add("127 bytes", longs, [K3(br.EQ, q + b"q")], [2])
    add("130 bytes", longs, [K3(br.GE, q + b"qqqq")], [3])
    # pad bytes are not the payload's: 'ab' ends at its tuple's last byte; the first tuple ends at the block's last byte, the
    # second has one pad byte of 0xEE behind it
    atts3 = ATTS[:3]
    pads = [tc.form_tuple(atts3, [1, b"p" * 8, b"ab"]), tc.form_tuple(atts3, [2, b"p" * 7, b"ab"])]
    assert len(pads[0]) == 40 and len(pads[1]) == 39
    blk = tc.build_block(B, pads, pad=0xEE)
    assert struct.unpack_from("<II", blk, 8) == (B - 40, 40) and blk[B - 80 + 39] == 0xEE
    add("the pad is not read: =", pads, [K3(br.EQ, b"ab\xee")], [], atts=atts3)
    add("the pad is not read: <", pads, [K3(br.LT, b"ab\xee")], [1, 2], atts=atts3)
    add("the pad is not read: = 'ab'", pads, [K3(br.EQ, b"ab")], [1, 2], atts=atts3)
    # special columns and key combinations
    short = [T(1, b"p"), T(2, b"p", b"abc"), T(3, b"p", None, 10, b"t"), tc.form_tuple(ATTS, [])]
    add("a column beyond natts is NULL: =", short, [K3(br.EQ, b"abc")], [2])
    add("a column beyond natts is NULL: <>", short, [K3(br.NE, b"abc")], [])
    add("a column beyond natts is NULL: ISNULL", short, [(3, br.BYTES, br.ISNULL, 0)], [1, 3, 4])
    pre = [T(i, b"p", p, 10 * i, b"t") for i, p in enumerate((b"abb", b"abc", b"abcz", b"abd", b"ab", b"abd0", b"abc\xff"), 1)]
    add("LIKE 'abc%' as a range", pre, [K3(br.GE, b"abc"), K3(br.LT, b"abd")], [2, 3, 7])
    four = [T(1, b"p", b"de", 10, b"x"), T(2, b"p", b"de", 10, b"y"), T(3, b"p", b"de", 11, b"x"), T(0, b"p", b"de", 10, b"x"),
            T(5, b"p", b"fr", 10, b"x"), T(6, b"pp", Long(b"de"), 10, Long(b"x")), T(7, b"p", b"de", None, b"x")]
    add("two byte-string and two integer keys", four,
        [K3(br.EQ, b"de"), (1, br.INT4, br.GT, 0), (5, br.BYTES, br.NE, b"y"), (4, br.INT8, br.LE, 10)], [1, 6])
    # undecided: a compressed header and an external pointer, each with every other key true, with an integer key false and
    # with a damaged column later in the walk; an external pointer under no byte-string key is stepped over
    z = b"z" * 40
    good = T(1, b"p", b"de", 10, b"tail")
    comp_ok = compressed(T(2, b"p", Long(z), 10, b"tail"), z)
    ext_ok = T(3, b"p", Toast(), 10, b"tail")
    comp_int = compressed(T(4, b"p", Long(z), 11, b"tail"), z)
    ext_int = T(5, b"p", Toast(), 11, b"tail")
    tail_at = len(good) - 5
    assert good[tail_at] == (5 << 1) | 1
    hurt = bytes([(100 << 1) | 1])
    comp_bad = compressed(T(6, b"p", Long(z), 10, b"tail"), z)
    comp_bad = comp_bad[:-5] + hurt + comp_bad[-4:]
    ext_bad = T(7, b"p", Toast(), 10, b"tail")
    ext_bad = ext_bad[:-5] + hurt + ext_bad[-4:]
    elsewhere = T(8, Toast(), b"de", 10, b"tail")
    und = [good, comp_ok, ext_ok, comp_int, ext_int, comp_bad, ext_bad, elsewhere]
    keys = [K3(br.EQ, b"de"), (4, br.INT8, br.EQ, 10), (5, 0, br.NOTNULL, 0)]
    add("undecided", und, keys, [1, 8], {2: br.UNDECIDED, 3: br.UNDECIDED, 6: br.TUPLE, 7: br.TUPLE})
    add("undecided under <>", und, [K3(br.NE, b"de"), (4, br.INT8, br.EQ, 10), (5, 0, br.NOTNULL, 0)], [],
        {2: br.UNDECIDED, 3: br.UNDECIDED, 6: br.TUPLE, 7: br.TUPLE})
    add("undecided, the walk ends at the key", und, [K3(br.EQ, b"de")], [1, 8], {p: br.UNDECIDED for p in range(2, 8)})
    add("a false byte-string key beside an undecided one", und, [K3(br.EQ, b"de"), (5, br.BYTES, br.EQ, b"other")], [],
        {6: br.TUPLE, 7: br.TUPLE})
    add("no byte-string key: every varlena is stepped over", und, [(4, br.INT8, br.EQ, 10), (5, 0, br.NOTNULL, 0)],
        [1, 2, 3, 8], {6: br.TUPLE, 7: br.TUPLE})
    # 290 items, five turns of the wave
    atts, blk = big_block()
    out.append(("290 items", 16384, atts, blk, [(2, br.BYTES, br.EQ, b"k1")], [i for i in range(1, 291) if i % 3 == 1 and i % 17],
                {i: br.UNDECIDED for i in range(17, 291, 17)}))
    return out


def descriptors():
    """[(name, atts, keys, key_rsv or None, ok)]: the argument rules of a byte-string key, and the pinned refusals of
    tests/filter_cases.py beside them.  key_rsv: the rsv fields to set after codec.filter_desc made the arrays; a BYTES value of
    None: a null address"""
    A = ATTS
    return [
        ("= on a text column", A, [K3(br.EQ, b"abc")], None, True),
        ("every op", A, [K3(op, b"abc") for op in (br.LT, br.LE, br.GE, br.GT)], None, True),
        ("an empty constant", A, [K3(br.EQ, b"")], None, True),
        ("an empty constant with a null address", A, [K3(br.NE, None)], [0], True),
        ("256 bytes", A, [K3(br.EQ, b"x" * 256)], None, True),
        ("four constants of 256 bytes", A, [K3(br.EQ, b"x" * 256)] * 2 + [(5, br.BYTES, br.GE, b"y" * 256)] * 2, None, True),
        ("beside integer keys and a null test", A, [K3(br.EQ, b"abc"), (1, br.INT4, br.GT, 0), (5, 0, br.NOTNULL, 0)], None, True),
        ("a null test of type BYTES: type and value ignored", A, [(3, br.BYTES, br.ISNULL, 0)], None, True),
        ("257 bytes", A, [K3(br.EQ, b"x" * 257)], None, False),
        ("a length of 2^32 - 1", A, [K3(br.EQ, b"abc")], [0xFFFFFFFF], False),
        ("a null address with a length", A, [K3(br.EQ, None)], [3], False),
        ("on an int4 column", A, [(1, br.BYTES, br.EQ, b"abc")], None, False),
        ("on an int8 column", A, [(4, br.BYTES, br.EQ, b"abcdefgh")], None, False),
        ("on a fixed-width column of 16 bytes", [(16, 1)], [(1, br.BYTES, br.EQ, b"x" * 16)], None, False),
        ("a null test of type BYTES with a length", A, [(3, br.BYTES, br.ISNULL, 0)], [3], False),
        ("op 9", A, [(3, br.BYTES, 9, b"abc")], None, False),
        ("op 0", A, [(3, br.BYTES, 0, b"abc")], None, False),
        ("type 17", A, [(3, 17, br.EQ, 0)], None, False),
        ("type 15", A, [(3, 15, br.EQ, 0)], None, False),
        # pinned by tests/filter_cases.py: they stay refused
        ("type 4", A, [(1, 4, br.EQ, 1)], None, False),
        ("type 0", A, [(1, 0, br.EQ, 1)], None, False),
        ("op 9 on an integer key", A, [(1, br.INT4, 9, 1)], None, False),
        ("a length on an integer key", A, [(1, br.INT4, br.EQ, 1)], [1], False),
        ("a length on an integer key beside a byte-string key", A, [K3(br.EQ, b"abc"), (1, br.INT4, br.EQ, 1)], [3, 1], False),
    ]
