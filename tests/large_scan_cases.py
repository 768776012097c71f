"""Blocks and tuples above 1 MiB for the four scan calls (filter, aggregate, group, project): the cases of
tests/test_large_scan_cpu.py and tests/test_gpu_large_scan.py.  Test infrastructure only, no GPU.

Where the scan code changes width, and the case that stands on the line:
  aliased(n)   n item ids that all name ONE tuple of 2^24 - 6 bytes (MAXALIGN: 2^24) in a block of B = upper + 2^24.  The
               matches' MAXALIGNed lengths sum to n * 2^24: for n = 256 exactly 2^32, which is 0 in 32 bits, for n = 257
               2^32 + 2^24, which is B - upper in 32 bits -- a wrapped sum says "fits" both times, the rule says OVERLAP.
               The aggregate, the grouping and the projection place no tuple and see n matches.  aliased(1) is the same tuple
               once: a plain match and one copy of 16 MiB.
  mixed()      B = 4 MiB + 24: varlena sizes on either side of the 1-byte / 4-byte header switch and of 2^16, payloads of
               1 MiB + 1 and 2.5 MiB in front of k, g and x (columns at tuple offsets above 2^16 and 2^20), a NULL body, a TOAST
               pointer, a short tuple, a tuple cut inside its varlena, a varlena that claims 0x3FFFFFFF bytes, an item that ends
               at B exactly and one that ends at B + 8.
  wide(B)      the generator's block of 290 tuples at 1 MiB + 8 and 4 MiB + 24, where the decode routes differ from 1 MiB.
  small(B)     six tuples of about 4 KiB in a block of the same B: the neighbour whose row and bytes a block's OVERLAP must leave
               alone.

The column layout is (id int4, body text with attalign 4, k int8, g int2, x float8); wide(B) has the generator's (id int4, body
text).  Payloads are periodic text, so every stream is small.  The longest constant a byte-string key takes is
CRYO_KEY_BYTES_MAX = 256 bytes, so the constants here are 256 bytes: PREFIX is a proper prefix of every long payload, which
leaves >, < and = to the lengths; NEAR_LOW and NEAR_HIGH differ from the payloads in their last byte, byte 255, alone.

expected() is the references' word on one block, computed once per (block, key set, call) and shared by every test of a
session; call_of() puts the per-block results together into a call's, with the references' own base arguments."""
import struct
import time

import numpy as np

import agg_ref
import fetch_ref
import float_ref as fl
import group_ref
import large_blocks as lb
import project_ref
import tuple_craft as tc
from pg_cryogen_amd import codec as cc

MIB = 1 << 20
TWO24, TWO32 = 1 << 24, 1 << 32
ATTS = [(4, 4), (-1, 4), (8, 8), (2, 2), (8, 8)]          # id int4, body text, k int8, g int2, x float8
ID, BODY, K, G, X = 1, 2, 3, 4, 5
WIDE_ATTS = [(4, 4), (-1, 4)]
LONG_LEN = TWO24 - 6                                      # the aliased tuple: MAXALIGN(LONG_LEN) = 2^24
LONG_K = -(1 << 40) - 5
MIXED_B = 4 * MIB + 24
WIDE_SIZES = (MIB + 8, 4 * MIB + 24)
LINE = b"the quick brown fox jumps over the lazy dog, "


def text(n):
    return (LINE * (n // len(LINE) + 1))[:n]


PREFIX = text(cc.KEY_BYTES_MAX)
NEAR_LOW = PREFIX[:-1] + bytes([PREFIX[-1] - 1])
NEAR_HIGH = PREFIX[:-1] + bytes([PREFIX[-1] + 1])
IN_LIST = [-3, 9, -9, 5, 1 << 40]

# name -> (keys, truth table or None).  Every set has matches and misses in mixed(); the integer, the float and the first
# byte-string set have both among its tuples above 2^16 bytes, the other byte-string sets tell those from the short ones
KEYSETS = {
    "int": ([(K, fl.INT8, fl.LT, 0), (G, fl.INT2, fl.EQ, 3)], None),
    "bytes_gt": ([(BODY, fl.BYTES, fl.GT, PREFIX), (K, fl.INT8, fl.LT, 0)], None),
    "bytes_lt": ([(BODY, fl.BYTES, fl.LT, PREFIX)], None),
    "bytes_eq": ([(BODY, fl.BYTES, fl.EQ, PREFIX)], None),
    "near": ([(BODY, fl.BYTES, fl.GT, NEAR_LOW), (BODY, fl.BYTES, fl.LT, NEAR_HIGH)], None),
    "float": ([(X, fl.FLOAT8, fl.GT, 0.5)], None),
    "truth": ([(K, fl.INT8, fl.IN, IN_LIST), (BODY, fl.BYTES, fl.GE, PREFIX)], cc.truth_dnf([1, 2], 2)),      # k IN (..) OR body >= const
    # the long tuple's match through the other two instantiations of the filter's kernel (a set key: the byte-string one; a float
    # key: the float one), without a read of its payload
    "set": ([(K, fl.INT8, fl.IN, [5, LONG_K, -21]), (G, fl.INT2, fl.EQ, 3)], None),
    "float_or": ([(X, fl.FLOAT8, fl.GT, 0.5), (K, fl.INT8, fl.LT, 0)], cc.truth_dnf([1, 2], 2)),              # x > 0.5 OR k < 0
}
WIDE_KEYSETS = {
    "int": ([(ID, fl.INT4, fl.GE, 100), (ID, fl.INT4, fl.LT, 200)], None),
    "bytes_gt": ([(BODY, fl.BYTES, fl.GT, b'{"ka": "'), (ID, fl.INT4, fl.LT, 50)], None),
    "truth": ([(ID, fl.INT4, fl.IN, [3, 17, 40, 289, 291]), (BODY, fl.BYTES, fl.LT, b'{"ka')], cc.truth_dnf([1, 2], 2)),
}
AGG_COLS = [(K, fl.INT8), (X, fl.FLOAT8), (G, fl.INT2)]
GROUP_BY = [(G, fl.INT2)]
PROJECT_COLS = [K, G, X, ID]
WIDE_AGG_COLS = [(ID, fl.INT4)]
WIDE_GROUP_BY = [(ID, fl.INT4)]
WIDE_PROJECT_COLS = [ID]


def row(i, body, k, g, x):
    """the bytes of one tuple; x a Python float or None"""
    return tc.form_tuple(ATTS, [i, body, k, g, None if x is None else fl.f8(x)])


def block_of(B, tuples, extra_items=()):
    """a block of the given tuples (bytes), the first at the block's end, zeros in every pad and in the gap; extra_items:
    (off, len) item ids behind the tuples' own, which name whatever lies there"""
    n = len(tuples) + len(extra_items)
    b = np.zeros(B, np.uint8)
    off = B
    for i, t in enumerate(tuples):
        off -= tc.maxalign(len(t))
        assert off >= 8 + 8 * n, "the tuples do not fit"
        b[off:off + len(t)] = np.frombuffer(t, np.uint8)
        b[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", off, len(t)), np.uint8)
    for j, item in enumerate(extra_items):
        i = len(tuples) + j
        b[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", *item), np.uint8)
    b[:8] = np.frombuffer(struct.pack("<II", 8 + 8 * n, off), np.uint8)
    return b


# ---- aliased(n) ----
def long_tuple():
    """(id, body, k, g) and x NULL: 24 header bytes, id, a 4-byte varlena header at 28, the payload, k at 2^24 - 16, g behind it.
    A tuple that ends with the int2 is the only one of this layout whose length is 2 mod 8"""
    t = row(7, tc.Long(text(TWO24 - 48)), LONG_K, 3, None)
    assert len(t) == LONG_LEN and tc.maxalign(len(t)) == TWO24
    return t


def aliased(n):
    """n item ids {upper, 2^24 - 6} on one tuple; lower = upper = 8 + 8n, B = upper + 2^24"""
    upper = tc.maxalign(8 + 8 * n)
    b = block_of(upper + TWO24, [long_tuple()], [(upper, LONG_LEN)] * (n - 1))
    assert struct.unpack_from("<II", b, 0) == (8 + 8 * n, upper) and b.size - upper == TWO24
    return b


# ---- mixed() ----
MIXED_N = 15
MIXED_ROWS = [                                            # (body payload bytes, k, g, x) of positions 1 .. 9
    (0, -1, 3, 1.0), (126, 5, 3, 0.25), (127, -7, 2, 2.5), (256, -2, 3, 0.5),
    (65531, -3, 3, -1.0), (65532, 9, 3, 7.0), (65533, -4, 1, 0.75),
    (MIB + 1, -5, 3, 3.5), (5 * MIB // 2, -6, 3, 0.125)]
# the filter's verdict per position, by hand: M a match, - no match, U undecided (9), T TUPLE (8), I ITEM (3)
MIXED_VERDICTS = {
    "int": "M--MM--MMMM-TTI",
    "bytes_gt": "----M-MMM-UMTTI",
    "bytes_lt": "MMM-------U-TTI",
    "bytes_eq": "---M------U-TTI",
    "near": "---MMMMMM-UMTTI",
    "float": "M-M--MMM-MM-TTI",
    "truth": "-M-MMMMMM-MMTTI",
    "set": "-M----------TTI",
    "float_or": "M-MMMMMMMMMMTTI",
}


def mixed(B=MIXED_B):
    """position 1 .. 9: MIXED_ROWS (1: its item ends at B exactly); 10: body NULL; 11: body a TOAST pointer; 12: (id, body, k)
    alone, g and x beyond the tuple's attributes; 13: the item's length 4 bytes short of where the varlena's 4-byte header says
    it ends; 14: the varlena's header claims 0x3FFFFFFF bytes; 15: an item id with off + MAXALIGN(len) = B + 8.  In a larger B
    the same tuples and a wider gap"""
    tuples = [row(i + 1, text(p), k, g, x) for i, (p, k, g, x) in enumerate(MIXED_ROWS)]
    tuples.append(row(10, None, -8, 3, 4.0))
    tuples.append(row(11, tc.Toast(), -9, 3, 5.0))
    tuples.append(tc.form_tuple(ATTS, [12, text(300), -10]))
    whole = row(13, text(1000), -11, 3, 6.0)
    assert struct.unpack_from("<I", whole, 28)[0] >> 2 == 1004
    tuples.append(whole[:28 + 1004 - 4])
    claim = bytearray(row(14, text(1000), -12, 3, 8.0))
    struct.pack_into("<I", claim, 28, 0x3FFFFFFF << 2)
    tuples.append(bytes(claim))
    b = block_of(B, tuples, [(B + 8 - 40, 40)])
    off, ln = struct.unpack_from("<II", b, 8)
    assert off + tc.maxalign(ln) == B
    off, ln = struct.unpack_from("<II", b, 8 + 8 * 14)
    assert off + tc.maxalign(ln) == B + 8 and off % 8 == 0 and off >= struct.unpack_from("<I", b, 4)[0]
    return b


def small(B):
    """six tuples at the end of a block of B bytes, four of about 4 KiB, one of 100 bytes of text and one whose body is PREFIX:
    matches and misses of every key set among them"""
    sizes = [4000, 100, 4002, len(PREFIX), 4004, 4005]
    return block_of(B, [row(100 + i, text(p), (-1) ** i * (20 + i), 3 if i % 3 else 2, 0.25 * i) for i, p in enumerate(sizes)])


def wide(oracle, B):
    return lb.build(oracle, "wide", B)


def narrow(oracle, B):
    """the generator's `narrow` block with the ids of wide(B)'s: block 0 of the seed"""
    return oracle.synth(lb.SEED, 0, B, lb.SYNTH.index("narrow"))


# ---- the cases ----
class Case:
    def __init__(self, name, block, wide_layout=False):
        self.name, self.block, self.B = name, block, block.size
        self.atts = WIDE_ATTS if wide_layout else ATTS
        self.keysets = WIDE_KEYSETS if wide_layout else KEYSETS
        self.agg_cols = WIDE_AGG_COLS if wide_layout else AGG_COLS
        self.group_by = WIDE_GROUP_BY if wide_layout else GROUP_BY
        self.project_cols = WIDE_PROJECT_COLS if wide_layout else PROJECT_COLS


_cases = {}
NAMES = ["aliased256", "aliased257", "aliased1", "mixed", "wide1m", "wide4m"]
# the key sets a case runs: every one where a reference call takes milliseconds, the match key alone on 256 aliases of 16 MiB
CASE_KEYSETS = {"aliased256": ["int"], "aliased257": ["int"], "aliased1": ["int", "bytes_gt", "near", "set", "float_or", "truth"],
                "mixed": list(KEYSETS), "wide1m": list(WIDE_KEYSETS), "wide4m": list(WIDE_KEYSETS)}
# key sets a case runs through the filter alone (with and without COUNT_ONLY)
FILTER_ONLY = {"aliased256": ["set", "float_or"], "aliased257": ["set", "float_or"]}


def case(oracle, name):
    """the named case, built once: .block, .B, .atts, .keysets, the columns of its aggregate, grouping and projection"""
    if name not in _cases:
        if name.startswith("aliased"):
            c = Case(name, aliased(int(name[7:])))
        elif name.startswith("mixed"):                     # "mixed", or "mixed@B": the same tuples in a block of B bytes
            c = Case(name, mixed(int(name[6:])) if "@" in name else mixed())
        else:
            c = Case(name, wide(oracle, WIDE_SIZES[0] if name == "wide1m" else WIDE_SIZES[1]), True)
        _cases[name] = c
    return _cases[name]


def neighbour(oracle, c):
    """the middle block of a case's batch of three: small(B), or for the generator's layout its `narrow` block of that B"""
    name = "small@%d" % c.B if c.atts is ATTS else "narrow@%d" % c.B
    if name not in _cases:
        _cases[name] = Case(name, small(c.B)) if c.atts is ATTS else Case(name, narrow(oracle, c.B), True)
    return _cases[name]


# ---- the references' word, once per (block, key set, call) ----
_expected = {}
seconds = {}                                              # (case, key set, call) -> what the reference call took


def expected(c, keyset, call):
    """the reference's result for the one block of case c: call is "filter", "count", "agg", "group" or "project" """
    key = (c.name, keyset, call)
    if key not in _expected:
        keys, W = c.keysets[keyset]
        t0 = time.time()
        if call == "filter":
            r = fl.filter_call([c.block], c.atts, keys, 0, W)
        elif call == "count":
            r = fl.filter_call([c.block], c.atts, keys, fl.COUNT_ONLY, W)
        elif call == "agg":
            r = fl.agg_call([c.block], c.atts, keys, c.agg_cols, W)
        elif call == "group":
            r = fl.group_call([c.block], c.atts, keys, c.group_by, c.agg_cols, W)
        else:
            r = fl.project_call([c.block], c.atts, keys, c.project_cols, W)
        seconds[key] = time.time() - t0
        _expected[key] = r
    return _expected[key]


def call_of(cases, keyset, call):
    """the reference's result for a call on the blocks of `cases`, in order, put together from expected(): the block table's
    running fields move by what the blocks before delivered, exactly as the references' own base arguments move them"""
    parts = [expected(c, keyset, call) for c in cases]
    if call == "agg":
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    if call == "group":
        rows = np.concatenate([p[0] for p in parts])
        at = 0
        for i, p in enumerate(parts):
            rows["first_group"][i] += at
            at += p[3]
        return rows, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), at
    first, second = ("row_first", "rec_first") if call == "project" else ("off", "rec_first")
    table = np.concatenate([p[0] for p in parts])
    a = b = 0
    for i, p in enumerate(parts):
        if call != "count":
            table[first][i] += a
            table[second][i] += b
        a, b = a + p[3][0], b + p[3][1]
    return table, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), (a, b)


def direct(cases, keyset, call):
    """the same call made on the references at once, for the cases where that is cheap: what call_of() must equal"""
    c = cases[0]
    keys, W = c.keysets[keyset]
    blocks = [x.block for x in cases]
    if call in ("filter", "count"):
        return fl.filter_call(blocks, c.atts, keys, fl.COUNT_ONLY if call == "count" else 0, W)
    if call == "agg":
        return fl.agg_call(blocks, c.atts, keys, c.agg_cols, W)
    if call == "group":
        return fl.group_call(blocks, c.atts, keys, c.group_by, c.agg_cols, W)
    return fl.project_call(blocks, c.atts, keys, c.project_cols, W)


def integer_only(c, keyset, call):
    """the integer key set through the references that know nothing of byte strings, sets, floats or truth tables: filter_ref,
    agg_ref, group_ref and project_ref as they are"""
    keys, W = c.keysets[keyset]
    assert W is None and all(k[1] in (fl.INT2, fl.INT4, fl.INT8) for k in keys)
    ints = [col for col in c.agg_cols if col[1] in (fl.INT2, fl.INT4, fl.INT8)]
    if call in ("filter", "count"):
        import filter_ref
        return filter_ref.filter_call([c.block], c.atts, keys, fl.COUNT_ONLY if call == "count" else 0)
    if call == "agg":
        return agg_ref.agg_call([c.block], c.atts, keys, ints)
    if call == "group":
        return group_ref.group_call([c.block], c.atts, keys, c.group_by, ints)
    return project_ref.project_call([c.block], c.atts, keys, c.project_cols)


def fetch_expected(c, positions):
    return fetch_ref.fetch_call([c.block], [positions])
