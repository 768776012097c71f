"""The hand-made vectors of the projecting-scan tests, shared by the CPU test (what tests/project_ref.py must say about them) and
the GPU test (the kernels against project_ref on the same blocks).  The tuples are crafted with tests/tuple_craft.py over the
descriptor (int4 id, bool flag, text name, float8 x, int2 s, "char" c, float4 y, timestamp ts): every width a projection knows,
a varlena in front of most of them.  Test infrastructure only.

cases() yields (name, B, atts, block, keys, cols, expected): expected the block's records in position order, (pos, status, nulls,
row) with the row's bytes written out by hand with struct formats that spell every pad byte -- they share no code with the
reference's layout rule."""
import struct

import numpy as np

import bytes_key_cases as bkc
import bytes_key_ref as br
import filter_ref as fr
import tuple_craft as tc
from tuple_craft import Long, Toast

B = 4096
ATTS = [(4, 4), (1, 1), (-1, 4), (8, 8), (2, 2), (1, 1), (4, 4), (8, 8)]
OK, ITEM, TUPLE, UNDECIDED = 0, 3, 8, 9
NAN8, NEG0_8, DENORM8, INF8 = 0x7FF8000000000001, 0x8000000000000000, 0x0000000000000001, 0x7FF0000000000000
NAN4, NEG0_4 = 0x7FC00001, 0x80000000


def sbits(u, bits):
    """the unsigned bit pattern u as the signed integer tuple_craft stores"""
    return u - (1 << bits) if u >> (bits - 1) else u


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def F8(u):
    return sbits(u, 64)


def F4(u):
    return sbits(u, 32)


def plain(i, name=None):
    """tuple i of the plain blocks: (i, i odd, "n" x i, the float8 bits 0x4000000000000000 + i, -i, 64 + i mod 60, the float4 bits
    0x40000000 + i, 10^12 + i)"""
    return T(i, i & 1, b"n" * i if name is None else name, 0x4000000000000000 + i, -i, 64 + i % 60, 0x40000000 + i, 10 ** 12 + i)


ID_RANGE = [(1, fr.INT4, fr.GE, 2), (1, fr.INT4, fr.LT, 5)]           # id = 2, 3, 4
MIX = [2, 8, 6, 5, 7, 1]                                              # widths 1, 8, 1, 2, 4, 4: pads after the first and the fourth
MIX_FMT = "<B7xqBxhII4x"                                              # offsets 0, 8, 16, 18, 20, 24; 32 bytes
EIGHT = [2, 6, 5, 1, 7, 4, 8, 2]                                      # widths 1, 1, 2, 4, 4, 8, 8, 1
EIGHT_FMT = "<BBhiI4xQqB7x"                                            # offsets 0, 1, 2, 4, 8, 16, 24, 32; 40 bytes
BYTES_KEY = [(3, br.BYTES, br.EQ, b"abc")]
INT_KEY = [(1, fr.INT4, fr.GE, 0)]


def mix_row(i):
    return struct.pack(MIX_FMT, i & 1, 10 ** 12 + i, 64 + i, -i, 0x40000000 + i, i)


def eight_row(i):
    return struct.pack(EIGHT_FMT, i & 1, 64 + i, -i, i, 0x40000000 + i, 0x4000000000000000 + i, 10 ** 12 + i, i & 1)


def cases():
    out = []

    def add(name, tuples, keys, cols, expected, atts=ATTS, size=B, patch=None):
        block = tc.build_block(size, tuples)
        if patch:
            patch(block)
        out.append((name, size, atts, block, keys, cols, expected))

    five = [plain(i) for i in range(1, 6)]
    # a width mix that forces pads inside the row; a range on the id
    add("width mix, range on id", five, ID_RANGE, MIX, [(p, OK, 0, mix_row(p)) for p in (2, 3, 4)])
    # one 1-byte column: a row of 8 bytes; no key: everything matches
    add("one char column, no key", five, [], [6], [(p, OK, 0, struct.pack("<B7x", 64 + p)) for p in range(1, 6)])
    # eight columns, one of them named twice
    add("eight columns", five, ID_RANGE, EIGHT, [(p, OK, 0, eight_row(p)) for p in (2, 3, 4)])
    # the same column twice, and it carries the key
    add("key column twice and an int8", five, [(1, fr.INT4, fr.EQ, 3)], [1, 1, 8],
        [(3, OK, 0, struct.pack("<iiq", 3, 3, 10 ** 12 + 3))])
    # nothing matches
    add("nothing matches", five, [(1, fr.INT4, fr.GT, 100)], MIX, [])
    # float bit patterns come back as they lie: NaN with a payload, -0.0, a denormal, infinity
    floats = [T(i + 1, 0, b"f", F8(u8), 0, 0, F4(u4), 0) for i, (u8, u4) in
              enumerate(((NAN8, NAN4), (NEG0_8, NEG0_4), (DENORM8, 1), (INF8, 0x7F800000)))]
    add("float bit patterns", floats, [], [4, 7],
        [(1, OK, 0, struct.pack("<QI4x", NAN8, NAN4)), (2, OK, 0, struct.pack("<QI4x", NEG0_8, NEG0_4)),
         (3, OK, 0, struct.pack("<QI4x", DENORM8, 1)), (4, OK, 0, struct.pack("<QI4x", INF8, 0x7F800000))])
    # NULLs: a clear bitmap bit on a projected column (5), columns beyond the tuple's natts (a tuple of three columns), all
    # projected columns NULL, and a NULL on a column that is not projected (3: the row is complete)
    nulls = [T(1, 1, b"a", 5, None, 70, 9, 11), T(2, 0, b"b"), T(3, None, b"c", 5, None, None, None, None), T(4, 1, None, 5, -4, 71, 9, 12)]
    add("nulls", nulls, [], [2, 5, 6, 8],                             # widths 1, 2, 1, 8: offsets 0, 2, 4, 8; 16 bytes
        [(1, OK, 0b0010, struct.pack("<BxhB3xq", 1, 0, 70, 11)), (2, OK, 0b1110, struct.pack("<BxhB3xq", 0, 0, 0, 0)),
         (3, OK, 0b1111, bytes(16)), (4, OK, 0, struct.pack("<BxhB3xq", 1, -4, 71, 12))])
    # a comparison on a NULL column is false, ISNULL picks it; the NULL key column is projected too
    add("null key column", nulls, [(5, 0, fr.ISNULL, 0)], [5, 1],
        [(1, OK, 0b01, struct.pack("<h2xi", 0, 1)), (2, OK, 0b01, struct.pack("<h2xi", 0, 2)), (3, OK, 0b01, struct.pack("<h2xi", 0, 3))])
    # varlenas in front of the projected columns: a 1-byte header, a 4-byte header that needs a pad, a TOAST pointer
    var = [plain(1, b"short"), plain(2, Long(b"z" * 61)), plain(3, Toast()), plain(4, b"q" * 300)]
    add("varlenas in front", var, [], [4, 8, 6],
        [(p, OK, 0, struct.pack("<QqB7x", 0x4000000000000000 + p, 10 ** 12 + p, 64 + p)) for p in (1, 2, 3, 4)])
    # a tuple cut a byte short of its last column (the timestamp): with the key on the id alone the filter passes it; a projection
    # that names the timestamp walks that far and calls it TUPLE; one that stops at the float4 passes it
    cut = [plain(1), plain(2)[:-1], plain(3)]
    add("cut before a projected column", cut, INT_KEY, [1, 8],
        [(1, OK, 0, struct.pack("<i4xq", 1, 10 ** 12 + 1)), (2, TUPLE, 0, None), (3, OK, 0, struct.pack("<i4xq", 3, 10 ** 12 + 3))])
    add("cut behind the projected columns", cut, INT_KEY, [1, 7],
        [(p, OK, 0, struct.pack("<iI", p, 0x40000000 + p)) for p in (1, 2, 3)])
    # a bad t_hoff, and an item of len 0
    bad_hoff = bytearray(plain(2))
    bad_hoff[22] = 28

    def item3_len0(block):
        block[8 + 8 * 2 + 4:8 + 8 * 2 + 8] = 0

    add("bad hoff and a bad item", [plain(1), bytes(bad_hoff), plain(3), plain(4)], [], [5],
        [(1, OK, 0, struct.pack("<h6x", -1)), (2, TUPLE, 0, None), (3, ITEM, 0, None), (4, OK, 0, struct.pack("<h6x", -4))],
        patch=item3_len0)
    # a byte-string key: in-line values are compared, a compressed in-line value and an external pointer are undecided -- a record
    # and no row, whatever the other columns hold; with integer keys only the same tuples all match
    z = bytes(range(200))
    comp = bkc.compressed(tc.form_tuple(ATTS, [3, 1, Long(z), 7, 8, 9, 10, 11]), z)
    bts = [plain(1, b"abc"), plain(2, b"abd"), comp, plain(4, Toast()), plain(5, b"abc")]
    add("byte-string key", bts, BYTES_KEY, [1, 5],
        [(1, OK, 0, struct.pack("<ih2x", 1, -1)), (3, UNDECIDED, 0, None), (4, UNDECIDED, 0, None), (5, OK, 0, struct.pack("<ih2x", 5, -5))])
    add("the same tuples, integer key", bts, INT_KEY, [1, 5],
        [(1, OK, 0, struct.pack("<ih2x", 1, -1)), (2, OK, 0, struct.pack("<ih2x", 2, -2)), (3, OK, 0, struct.pack("<ih2x", 3, 8)),
         (4, OK, 0, struct.pack("<ih2x", 4, -4)), (5, OK, 0, struct.pack("<ih2x", 5, -5))])
    return out


def other_block(n=7):
    """a block of other tuples, for the batches in which crafted blocks alternate with it: ids 100 .. 100 + n - 1"""
    return tc.build_block(B, [plain(100 + i) for i in range(n)])


def header_block():
    x = tc.build_block(B, [plain(i) for i in range(1, 4)])
    x[0:4] = np.frombuffer((12).to_bytes(4, "little"), np.uint8)          # lower = 12: not 8 + 8 n
    return x


TURN_ATTS = [(4, 4), (1, 1)]
TURN_B = 16384
TURN_SIZES = (0, 1, 63, 64, 65, 128, 129, 290)
TURN_COLS = [2, 1]                                                     # widths 1, 4: offsets 0, 4; 8 bytes


def turn_block(n):
    """n tuples (position p: id p, char p mod 251)"""
    return tc.build_block(TURN_B, [tc.form_tuple(TURN_ATTS, [p, p % 251 - 125]) for p in range(1, n + 1)])


TURN_KEYS = {"all": [], "none": [(1, fr.INT4, fr.LT, 0)]}            # every item matches, none does


def turn_block_alternating(n):
    """n tuples whose id is p at odd positions and -p at even ones: the key id > 0 picks every other item"""
    return tc.build_block(TURN_B, [tc.form_tuple(TURN_ATTS, [p if p & 1 else -p, p % 100]) for p in range(1, n + 1)])


ALTERNATING_KEYS = [(1, fr.INT4, fr.GT, 0)]


def descriptors():
    """[(name, atts, keys, cols, flags, patch, ok)]: every argument rule of the projection.  patch: None, or (which, field, index,
    value) to set a reserved field ("f" the filter struct, "a" atts, "k" keys, "p" the projection struct, "c" its columns)"""
    A = ATTS
    int4 = (1, fr.INT4, fr.EQ, 1)
    return [
        ("one column", A, [int4], [1], 0, None, True),
        ("no key", A, [], [4], 0, None, True),
        ("eight columns", A, [int4], EIGHT, 0, None, True),
        ("the same column twice", A, [], [2, 2], 0, None, True),
        ("a column that carries a key", A, [int4], [1], 0, None, True),
        ("a byte-string key beside it", A, BYTES_KEY, [1], 0, None, True),
        ("int2 column aligned to 4", [(2, 4)], [], [1], 0, None, True),
        ("column 1600", [(4, 4)] * 1600, [], [1600], 0, None, True),
        ("no column", A, [int4], [], 0, None, False),
        ("nine columns", A, [int4], EIGHT + [1], 0, None, False),
        ("att 0", A, [], [0], 0, None, False),
        ("att beyond natts", A, [], [9], 0, None, False),
        ("a varlena column", A, [], [3], 0, None, False),
        ("attlen 3", [(3, 1)], [], [1], 0, None, False),
        ("attlen 16", [(16, 8)], [], [1], 0, None, False),
        ("attalign below attlen", [(8, 4)], [], [1], 0, None, False),
        ("a bad column behind a good one", A, [], [1, 3], 0, None, False),
        ("count only", A, [int4], [1], fr.COUNT_ONLY, None, False),
        ("unknown flag", A, [int4], [1], 2, None, False),
        ("reserved field of the projection", A, [], [1], 0, ("p", "rsv", 0, 1), False),
        ("reserved half of a column", A, [], [1, 4], 0, ("c", "rsv", 1, 1), False),
        ("reserved word of a column", A, [], [1], 0, ("c", "rsv2", 0, 1), False),
        ("reserved field of the filter", A, [int4], [1], 0, ("f", "rsv", 0, 1), False),
        ("reserved field of an att", A, [int4], [1], 0, ("a", "rsv", 5, 1), False),
        ("reserved field of an integer key", A, [int4], [1], 0, ("k", "rsv", 0, 1), False),
        ("five keys", A, [int4] * 5, [1], 0, None, False),
        ("key on att 0", A, [(0, fr.INT4, fr.EQ, 1)], [1], 0, None, False),
    ]


def ref_ok(pr, atts, keys, cols, flags, patch):
    """project_ref.desc_ok on a descriptors() entry"""
    kw = {}
    if patch:
        which, field, index, value = patch
        at = [0] * index + [value]
        if which == "f":
            kw = dict(rsv=value)
        elif which == "p":
            kw = dict(prj_rsv=value)
        elif which == "a":
            kw = dict(att_rsv=at)
        elif which == "k":
            kw = dict(key_rsv=at)
        else:
            kw = dict(col_rsv=at) if field == "rsv" else dict(col_rsv2=at)
    return pr.desc_ok(atts, keys, cols, flags, **kw)
