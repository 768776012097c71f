"""The hand-made vectors of the pattern key tests, shared by the CPU test (what tests/like_ref.py must say about them) and the GPU
tests (the kernels against like_ref on the same blocks).  The tuples are crafted with tests/tuple_craft.py over the descriptor of
tests/bytes_key_cases.py, (int4, text, text, int8, text); the pattern keys sit on column 3 (behind a short text, so that its
payload starts anywhere) and on column 5.  Test infrastructure only.

cases() yields (name, B, atts, block, keys, truth, matches, bad): matches the positions that must match, bad {position: status},
both written out by hand.  Most cases come in pairs: the LIKE key with the positions written beside it, and the NOT LIKE key
on the same block, whose positions are the other values -- less the NULLs and the undecided ones, which a case names."""
import bytes_key_cases as bc
import like_ref as lr
import tuple_craft as tc
from bytes_key_cases import ATTS, T, compressed
from like_ref import P
from tuple_craft import Long, Toast

B = 4096
BIG = 131072
OR2 = 0b1110                                                            # keys[0] OR keys[1]


def K3(op, pattern, utf8=True):
    return (3, lr.BYTES, op, P(pattern, utf8))


def lit(n, seed=0):
    """n bytes that differ from place to place, use the high bit and are never '%', '_' or a backslash"""
    out = bytearray()
    i = seed
    while len(out) < n:
        b = (37 * i + 11) % 256
        i += 1
        if b not in (0x25, 0x5F, 0x5C):
            out.append(b)
    return bytes(out)


LETTERS = bytes(97 + i % 26 for i in range(128))                        # a .. z, five times over
SEGMENTS_128 = b"%".join(bytes([c]) for c in LETTERS)                   # 'a%b%c% .. %x': 128 one-byte segments, 255 bytes


class Z:
    """a value compressed in line: a 4-byte header with the low bits 10 over 40 bytes"""
    payload = b"z" * 40


def rows(values, ints=None):
    """one tuple per value, column 3 holding it behind a text of 0 .. 8 bytes; column 4 is 10 or ints[i]"""
    out = []
    for i, v in enumerate(values, 1):
        x = 10 if ints is None else ints[i - 1]
        if v is Z:
            out.append(compressed(T(i, b"p" * (i % 9), Long(Z.payload), x, b"t"), Z.payload))
        else:
            out.append(T(i, b"p" * (i % 9), v, x, b"t"))
    return out


def cases():
    out = []

    def add(name, tuples, keys, matches, bad=None, truth=None, atts=ATTS, size=B):
        out.append((name, size, atts, tc.build_block(size, tuples), keys, truth, matches, bad or {}))

    def pair(name, values, pattern, matches, utf8=True, nulls=(), undecided=(), size=B):
        """LIKE with the positions written out, NOT LIKE with the others; nulls and undecided: the positions that are neither"""
        tuples = rows(values)
        bad = {p: lr.UNDECIDED for p in undecided}
        add("%s: LIKE" % name, tuples, [K3(lr.LIKE, pattern, utf8)], matches, bad, size=size)
        rest = [p for p in range(1, len(values) + 1) if p not in matches and p not in nulls and p not in undecided]
        add("%s: NOT LIKE" % name, tuples, [K3(lr.NOT_LIKE, pattern, utf8)], rest, bad, size=size)

    # the smallest patterns
    pair("the empty pattern matches the empty value alone", [b"", b"a", None, Long(b""), b"%"], b"", [1, 4], nulls=[3])
    pair("'%' matches every value, the empty one too", [b"", b"a", b"abc", None, Long(b"abc")], b"%", [1, 2, 3, 5], nulls=[4])
    pair("'_' is one character", [b"", b"a", b"ab", "é".encode(), b"_"], b"_", [2, 4, 5])
    pair("'_' is one byte without the flag", [b"", b"a", b"ab", "é".encode(), b"_"], b"_", [2, 5], utf8=False)
    pair("'%%' is '%'", [b"", b"x", None], b"%%", [1, 2], nulls=[3])
    pair("'%_%' is any value that is not empty", [b"", b"x", b"xy", Long(b"")], b"%_%", [2, 3])
    # anchors
    pair("no '%': anchored at both ends", [b"abc", b"abcd", b"xabc", b"ab", b"abC", Long(b"abc"), b""], b"abc", [1, 6])
    pair("a leading '%' alone", [b"abc", b"xabc", b"abcx", b"abcabc", b"bc", b"ababc"], b"%abc", [1, 2, 4, 6])
    pair("a trailing '%' alone", [b"abc", b"abcx", b"xabc", b"ab", b"abcabc"], b"abc%", [1, 2, 5])
    pair("'%' on both sides", [b"abc", b"xabcx", b"ab", b"aabbcc", b"xxabc"], b"%abc%", [1, 2, 5])
    pair("'_' inside a segment", [b"abc", b"axc", b"ac", b"abbc", b"xaxcx"], b"%a_c%", [1, 2, 5])
    # greedy traps
    pair("a segment that occurs twice, only the second leaving room for the tail", [b"abab", b"abxab", b"ab", b"aab", b"ababx", b"abab ab"],
         b"%ab%ab", [1, 2, 6])
    pair("the overlap trap", [b"aaab", b"aab", b"aaba", b"ab", b"aabaab"], b"%aab", [1, 2, 5])
    pair("the tail must end at the end, not at its first occurrence", [b"xay", b"xayay", b"xayaz", b"xa"], b"x%ay", [1, 2])
    pair("a middle segment takes its leftmost place", [b"a1b2b3c", b"ab", b"a-b-c", b"acb", b"abbc"], b"a%b%c", [1, 3, 5])
    # escapes
    pair("escaped '%', '_' and backslash are literals", [b"%_\\", b"a_\\", b"%x\\", b"%_", b"%_\\\\"], b"\\%\\_\\\\", [1])
    pair("an escaped '%' inside a prefix", [b"a%b", b"a%bcd", b"axb", b"a%", b"a%%b"], b"a\\%b%", [1, 2])
    pair("an escaped ordinary byte is that byte", [b"ab", b"a\\b", b"a"], b"\\a\\b", [1])
    # long patterns
    p256, p254 = lit(256), lit(254, 5)
    assert p256[255] != 1
    pair("a pattern of 256 bytes", [p256, p256[:255] + b"\x01", p256 + b"q", p256[:255]], p256, [1])
    pair("a pattern of 255 bytes", [b"zz" + p254, p254, p254[1:], p254 + b"z"], b"%" + p254, [1, 2])
    gaps = b"--".join(bytes([c]) for c in LETTERS)
    pair("128 one-byte segments", [LETTERS, gaps, LETTERS[:-1], LETTERS[::-1], b"-" + LETTERS, LETTERS + LETTERS], SEGMENTS_128, [1, 2, 6])
    # the value's length and header
    ends = [b"." * (n - 6) + b"needle" for n in (7, 8, 9, 126, 127)]
    pair("values of 7, 8, 9, 126 and 127 bytes: the tail", ends + [v[:-1] + b"f" for v in ends], b"%needle", [1, 2, 3, 4, 5])
    starts = [b"needle" + b"." * (n - 6) for n in (7, 8, 9, 126, 127)]
    pair("values of 7, 8, 9, 126 and 127 bytes: the head", starts + [b"f" + v[1:] for v in starts], b"needle%", [1, 2, 3, 4, 5])
    pair("the same content under a 1-byte and a 4-byte header", [b"needle", Long(b"needle"), Long(b"needlf"), Long(b"xneedle")], b"%needle",
         [1, 2, 4])
    # the cap
    pair("2047 and 2048 bytes are matched, 2049 are not", [b"a" * (n - 3) + b"end" for n in (2047, 2048, 2049)] + [b"a" * 2048],
         b"%end", [1, 2], undecided=[3], size=BIG)
    pair("2049 bytes are undecided under '%' too", [b"a" * 2049, b"a" * 2048], b"%", [2], undecided=[1], size=BIG)
    # nothing behind the payload is the value's: 'ab' ends at its tuple's last byte; the first tuple ends at the block's last
    # byte, the second has one pad byte of 0xEE behind it, which would complete each of these patterns
    atts3 = ATTS[:3]
    pads = [tc.form_tuple(atts3, [1, b"p" * 8, b"ab"]), tc.form_tuple(atts3, [2, b"p" * 7, b"ab"])]
    assert len(pads[0]) == 40 and len(pads[1]) == 39
    for pattern, matches in ((b"ab\xee", []), (b"ab_", []), (b"%\xee", []), (b"ab%\xee", []), (b"%b_", []), (b"ab", [1, 2]), (b"ab%", [1, 2]),
                             (b"%b", [1, 2])):
        add("the pad is not read: %r" % pattern, pads, [K3(lr.LIKE, pattern, False)], matches, atts=atts3)
    add("the pad is not read: NOT LIKE 'ab_'", pads, [K3(lr.NOT_LIKE, b"ab_", False)], [1, 2], atts=atts3)
    # ... and neither is the next column: 'ab' is followed by the header byte 0x07 and the bytes 'cd' of column 4
    atts4 = ATTS[:3] + [(-1, 4)]
    nxt = [tc.form_tuple(atts4, [1, b"p", b"ab", b"cd"]), tc.form_tuple(atts4, [2, b"pp", b"ab", b"cd"])]
    assert nxt[0].endswith(b"ab\x07cd")
    for pattern, matches in ((b"ab\x07cd", []), (b"ab___", []), (b"ab%cd", []), (b"%cd", []), (b"ab_", []), (b"ab", [1, 2]), (b"%ab", [1, 2])):
        add("the next column is not read: %r" % pattern, nxt, [K3(lr.LIKE, pattern, False)], matches, atts=atts4)
    # characters
    e2, e3, e4 = "é".encode(), "€".encode(), "\U0001d11e".encode()
    assert (len(e2), len(e3), len(e4)) == (2, 3, 4)
    chars = [e2, e3, e4, b"a", e2 + e3, b"a" + e4, b""]
    pair("'_' over characters of 2, 3 and 4 bytes", chars, b"_", [1, 2, 3, 4])
    pair("the same values as bytes: '_'", chars, b"_", [4], utf8=False)
    pair("'__' over characters", chars, b"__", [5, 6])
    pair("the same values as bytes: '__'", chars, b"__", [1], utf8=False)
    pair("'___' as bytes", chars, b"___", [2], utf8=False)
    pair("a literal character between two '_'", [b"x" + e2 + b"y", e3 + e2 + e4, e2 + e2, b"x" + e2], b"_" + e2 + b"_", [1, 2])
    pair("'%' and a character", [b"caf" + e2, e2, b"cafe", e2 + b"s"], b"%" + e2, [1, 2])
    # text that is no valid UTF-8: three continuation bytes are one character (the first byte and the two that follow it); a
    # lead byte without its continuation is a character of one byte
    odd = [b"\x80\x80\x80", b"\xc3", b"\xc3a", b"\x80", b"a\x80\x80", b""]
    pair("'%_' on continuation bytes and a truncated lead", odd, b"%_", [1, 2, 3, 4, 5])
    pair("'_%' on continuation bytes and a truncated lead", odd, b"_%", [1, 2, 3, 4, 5])
    pair("'_' on continuation bytes and a truncated lead", odd, b"_", [1, 2, 4, 5])
    pair("'_' on the same bytes without the flag", odd, b"_", [2, 4], utf8=False)
    pair("'__' on continuation bytes and a truncated lead", odd, b"__", [3])
    pair("'__' on the same bytes without the flag", odd, b"__", [3], utf8=False)
    pair("'___' on the same bytes without the flag", odd, b"___", [1, 5], utf8=False)
    pair("'_a': the lead byte alone is the character", odd, b"_a", [3])
    pair("'%a_': 'a' and the two bytes behind it", odd, b"%a_", [5])
    pair("'a%' then nothing: the run takes the continuation bytes", odd, b"a%", [5])
    # NULL, an external pointer, a value compressed in line: under AND, and under LIKE .. OR x = 10 where the integer settles it
    vals = [b"abc", None, Toast(), Z, b"zzz", b"abc", None, Toast(), Z, b"zzz", b"abcd"]
    ints = [10, 10, 10, 10, 10, 11, 11, 11, 11, 11, None]
    und = rows(vals, ints)
    both = [K3(lr.LIKE, b"abc%"), (4, lr.INT8, lr.EQ, 10)]
    add("NULL, external, compressed: LIKE AND x = 10", und, both, [1], {3: lr.UNDECIDED, 4: lr.UNDECIDED})
    add("NULL, external, compressed: LIKE OR x = 10", und, both, [1, 2, 3, 4, 5, 6, 11], {8: lr.UNDECIDED, 9: lr.UNDECIDED}, truth=OR2)
    nboth = [K3(lr.NOT_LIKE, b"abc%"), (4, lr.INT8, lr.EQ, 10)]
    add("NULL, external, compressed: NOT LIKE AND x = 10", und, nboth, [5], {3: lr.UNDECIDED, 4: lr.UNDECIDED})
    add("NULL, external, compressed: NOT LIKE OR x = 10", und, nboth, [1, 2, 3, 4, 5, 10], {8: lr.UNDECIDED, 9: lr.UNDECIDED}, truth=OR2)
    add("NULL, external, compressed: the key alone", und, [K3(lr.LIKE, b"abc%")], [1, 6, 11], {p: lr.UNDECIDED for p in (3, 4, 8, 9)})
    add("a false integer key beside an undecided pattern key", und, [K3(lr.LIKE, b"abc%"), (4, lr.INT8, lr.EQ, 12)], [])
    add("IS NULL beside a pattern key on the same column", und, [K3(lr.NOT_LIKE, b"abc%"), (3, 0, lr.ISNULL, 0)], [2, 5, 7, 10],
        {p: lr.UNDECIDED for p in (3, 4, 8, 9)}, truth=OR2)
    short = [T(1, b"p"), T(2, b"p", b"abc"), tc.form_tuple(ATTS, [])]
    add("a column beyond natts is NULL: LIKE", short, [K3(lr.LIKE, b"%")], [2])
    add("a column beyond natts is NULL: NOT LIKE", short, [K3(lr.NOT_LIKE, b"x")], [2])
    # several pattern keys
    two = [T(1, b"p", b"a-z", 10, b"cat"), T(2, b"p", b"a-y", 10, b"cat"), T(3, b"p", b"b-z", 10, b"hat"), T(4, b"p", b"az", 10, b"dog"),
           T(5, b"p", b"a", 10, None), T(6, b"p", b"z", 10, b"t")]
    add("two pattern keys on one column", two, [K3(lr.LIKE, b"a%"), K3(lr.LIKE, b"%z")], [1, 4])
    add("a pattern key on each of two columns", two, [K3(lr.LIKE, b"a%"), (5, lr.BYTES, lr.LIKE, P(b"%at"))], [1, 2])
    add("LIKE and NOT LIKE on two columns, beside an integer and a byte-string key", two,
        [K3(lr.LIKE, b"%z"), (5, lr.BYTES, lr.NOT_LIKE, P(b"%at")), (1, lr.INT4, lr.GE, 4), (3, lr.BYTES, lr.NE, b"z")], [4])
    add("four pattern keys, any of them", two, [K3(lr.LIKE, b"b%"), K3(lr.LIKE, b"_"), (5, lr.BYTES, lr.LIKE, P(b"d_g")),
                                                (5, lr.BYTES, lr.LIKE, P(b"%x%"))], [3, 4, 5, 6], truth=0xFFFE)
    # 290 items, five turns of the wave: every 17th an external pointer, the others 'k0' / 'k1' / 'k2' by position
    atts, blk = bc.big_block()
    out.append(("290 items", 16384, atts, blk, [(2, lr.BYTES, lr.LIKE, P(b"%1"))], None, [i for i in range(1, 291) if i % 3 == 1 and i % 17],
                {i: lr.UNDECIDED for i in range(17, 291, 17)}))
    return out


def descriptors():
    """[(name, atts, keys, key_rsv or None, ok)]: the argument rules of a pattern key, and the refusals that stay.  key_rsv: the
    rsv fields as the call carries them, when they are not what codec.like made"""
    A = ATTS
    return [
        ("LIKE on a text column", A, [K3(lr.LIKE, b"a%")], None, True),
        ("NOT LIKE", A, [K3(lr.NOT_LIKE, b"%a_")], None, True),
        ("without the flag", A, [K3(lr.LIKE, b"a%", False)], None, True),
        ("the empty pattern", A, [K3(lr.LIKE, b"")], None, True),
        ("the empty pattern with a null address", A, [K3(lr.LIKE, None)], None, True),
        ("256 bytes", A, [K3(lr.LIKE, b"x" * 256)], None, True),
        ("four patterns of 256 bytes", A, [K3(lr.LIKE, b"%" * 256)] * 2 + [(5, lr.BYTES, lr.NOT_LIKE, P(b"y" * 256))] * 2, None, True),
        ("beside every other kind of key", A, [K3(lr.LIKE, b"a%"), (1, lr.INT4, lr.IN, [1, 2]), (5, lr.BYTES, lr.EQ, b"t"), (4, 0, lr.NOTNULL, 0)],
         None, True),
        ("an escaped backslash at the end", A, [K3(lr.LIKE, b"a\\\\")], None, True),
        ("257 bytes", A, [K3(lr.LIKE, b"x" * 257)], None, False),
        ("a null address with a length", A, [(3, lr.BYTES, lr.LIKE, P(None, rsv=3))], None, False),
        ("rsv bit 17", A, [(3, lr.BYTES, lr.LIKE, P(b"abc", rsv=3 | 1 << 17))], None, False),
        ("rsv bit 31", A, [(3, lr.BYTES, lr.NOT_LIKE, P(b"abc", rsv=3 | 1 << 31))], None, False),
        ("on an int4 column", A, [(1, lr.BYTES, lr.LIKE, P(b"abc"))], None, False),
        ("on an int8 column", A, [(4, lr.BYTES, lr.NOT_LIKE, P(b"abcdefgh"))], None, False),
        ("type INT4", A, [(3, lr.INT4, lr.LIKE, P(b"abc"))], None, False),
        ("type 0", A, [(3, 0, lr.LIKE, P(b"abc"))], None, False),
        ("a trailing escape", A, [K3(lr.LIKE, b"abc\\")], None, False),
        ("a backslash alone", A, [K3(lr.NOT_LIKE, b"\\")], None, False),
        ("an escaped backslash and a trailing escape", A, [K3(lr.LIKE, b"\\\\\\")], None, False),
        ("op 13", A, [(3, lr.BYTES, 13, P(b"abc"))], None, False),
        # pinned by the tests of the other keys: they stay refused
        ("op 11 on an integer key", A, [(1, lr.INT4, 11, 1)], None, False),
        ("op 9 on a byte-string key", A, [(3, lr.BYTES, 9, b"abc")], None, False),
    ]
