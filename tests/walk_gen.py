"""Wide random tuples for the walk that the four scan kernels share (filter, aggregate, group, projection), and expectations that
involve no walk.  Test infrastructure only.

A case is (atts, rows, tuples, B) and what a call names on it.  rows[i] is the list of Python values tuple i was made from -- None,
an int, bytes, Long, Toast or Compressed --, truncated to that tuple's own tnatts.  Every expectation below is computed from the
rows and the descriptor alone, never from tuple bytes: whether a row passes the keys is a comparison of Python values, its
aggregates are sums of Python integers, its projected row is laid out with project_ref.row_layout (laying out a row is not walking
a tuple).  The only use of tuple bytes is a length: the end of column j within the data area is
len(form_tuple(atts, row[:j + 1])) - hoff, valid because alignment counts from hoff -- which gives the cut rule: with `last` the
highest column a call references,
    need = max(23, hoff + end of the last non-NULL column <= min(last, tnatts)),
and the tuple cut to its first c bytes is TUPLE iff c < need; otherwise it has the uncut tuple's verdict and capture.

The newer calls stand on the same rows: the ordered scan (expect_topn: Python's sorted on the rows' values), the grouping by text
and by buckets (the key a Python bytes value, or the bucket's arithmetic stated here in Python integers), and keys of every later
kind -- set keys by Python's `in`, float keys on the stored integers read as float bits and compared as Python floats, pattern
keys by like_ref.match, the backtracking definition, on the row's bytes, and a truth table read as the header states it.  The
expectations share no code with the references they are held against, save that matcher and the table's three-line verdict.

Everything is seeded with fixed integers: the GPU run is the same every time.  The plans of the newer calls (Plan._newer) draw
from no generator at all, so the older cases keep their bytes."""
import operator
import random
import struct

import bytes_key_cases as bc
import group_text_ref as gt
import like_ref
import project_ref as pr
import truth_key_ref as tr
import tuple_craft as tc
from bytes_key_ref import BYTES, INT2, INT4, INT8, ISNULL, NOTNULL, OK, NOMATCH, TUPLE, UNDECIDED
from filter_ref import EQ, GE, GT, LE, LT, NE
from float_ref import FLOAT4, FLOAT8, IN, NOT_IN
from like_ref import LIKE, NOT_LIKE, P
from tuple_craft import Long, Toast

INT_TYPE = {2: INT2, 4: INT4, 8: INT8}
ODD = [(16, 1), (16, 8), (6, 2), (6, 4), (12, 4), (64, 1), (3, 1), (2, 4), (4, 8), (-1, 8)]
PLAIN = [(1, 1), (2, 2), (4, 4), (8, 8), (-1, 4)]
FLAGS = (0, 0x2000, 0x4000, 0x8000, 0xE000)          # bits 11 .. 15 of t_infomask2: what & 0x07FF must drop
INFO = (0, 0x0004, 0x0100, 0xFF0C)                   # t_infomask beside HASNULL and HASVARWIDTH
EXTRA_HOFF = (0, 8, 16)
RANDOM_N = (1, 7, 8, 9, 17, 64, 65, 200)
SWEEP_B = 16384
MAX_BLOCKS = 4
_OPS = {LT: operator.lt, LE: operator.le, EQ: operator.eq, GE: operator.ge, GT: operator.gt, NE: operator.ne}
FLOAT_TYPE = {4: FLOAT4, 8: FLOAT8}
DESC, NULLS_FIRST = 1, 2                                # an order column's flags
FLAG_SETS = (0, DESC, NULLS_FIRST, DESC | NULLS_FIRST)
TEXT_MAX = 32                                           # a text group key's bytes
LIKE_MAX = 2048                                         # the payload a pattern key reads
WIDTH, BOUNDS, INFINITE = 1, 2, 1                       # a bucket's kinds and its flag
RAW = (0, 0, 0, 0)
AWAY = "undecided"                                      # a group value that is no key
INT64_MIN = -(1 << 63)


class Compressed:
    """a varlena compressed in line: a 4-byte header with the low bits 10 (bytes_key_cases.compressed).  Its payload is unique
    within its tuple"""

    def __init__(self, payload):
        self.payload = bytes(payload)


def is_int(att):
    """a key, an aggregate or a group column may sit here"""
    return att[0] in INT_TYPE and att[1] >= att[0]


def is_narrow(att):
    """a projected column may sit here"""
    return att[0] in (1, 2, 4, 8) and att[1] >= att[0]


def typed(atts, col):
    return (col, INT_TYPE[atts[col - 1][0]])


def extremes(attlen):
    return -(1 << (8 * attlen - 1)), (1 << (8 * attlen - 1)) - 1


# ---- tuples ----
def make_tuple(atts, row, knobs=None):
    t = tc.form_tuple(atts, [Long(v.payload) if isinstance(v, Compressed) else v for v in row], **(knobs or {}))
    for v in row:
        if isinstance(v, Compressed):
            t = bc.compressed(t, v.payload)
    return t


def data_end(atts, row, j):
    """where column j (0-based, not NULL) ends, counted from hoff"""
    t = make_tuple(atts, row[:j + 1])
    return len(t) - t[22]


def need(atts, row, hoff, last):
    live = [j for j in range(min(last, len(row))) if row[j] is not None]
    return max(23, hoff + (data_end(atts, row, live[-1]) if live else 0))


def pad_before(atts, row, j):
    """the pad bytes in front of column j, a varlena with a 4-byte header"""
    live = [i for i in range(j) if row[i] is not None]
    return -(data_end(atts, row, live[-1]) if live else 0) % atts[j][1]


def has_long_header(v):
    return isinstance(v, (Long, Compressed)) or (isinstance(v, bytes) and len(v) > 126)


# ---- drawing ----
def draw_fixed(rng, attlen):
    lo, hi = extremes(attlen)
    return rng.choice((lo, hi, 0, -1, rng.randint(lo, hi)))


def draw_text(rng, uniq):
    kind = rng.random()
    if kind < 0.08:
        return Toast()
    if kind < 0.16:
        return Compressed(b"Z%06d" % uniq + bytes(rng.choice(b"ab\xe9") for _ in range(rng.choice((0, 3, 50)))))
    payload = bytes(rng.choice(b"ab\xe9") for _ in range(rng.choice((0, 1, 1, 2, 3, 8, 9, 40, 60, 126, 127, 188))))
    return Long(payload) if kind < 0.4 else payload


def draw_knobs(rng):
    return dict(infomask2_flags=rng.choice(FLAGS), infomask_flags=rng.choice(INFO), extra_hoff=rng.choice(EXTRA_HOFF),
                force_bitmap=rng.random() < 0.15)


def draw_row(rng, atts, uniq):
    kind = rng.random()
    n = len(atts) if kind < 0.7 else 0 if kind < 0.75 else rng.randint(0, len(atts))
    row = []
    for j, (attlen, _) in enumerate(atts[:n]):
        if rng.random() < 0.25:
            row.append(None)
        elif attlen > 0:
            row.append(draw_fixed(rng, attlen))
        else:
            row.append(draw_text(rng, 1000 * uniq + j))
    return row


def draw_atts(rng, n):
    atts = [rng.choice(ODD + PLAIN) for _ in range(n)]
    if not any(is_int(a) for a in atts):
        atts.append((4, 4))                                     # no column a key may sit on: append one, drop nothing
    return atts


# ---- what a call names ----
def spread(cols, prefer):
    """cols in the order they are handed out: the preferred ones, then those beyond bitmap byte 0 from both ends inwards, then
    the rest"""
    first = [c for c in prefer if c in cols]
    far = [c for c in cols if c > 8 and c not in first]
    mixed = []
    while far:
        mixed.append(far.pop())
        if far:
            mixed.append(far.pop(0))
    return first + mixed + [c for c in cols if c <= 8 and c not in first]


def most_common(values):
    return max(sorted(set(values)), key=values.count)


class Plan:
    """the key sets and the captured columns of the calls on a case: keysets of 0, 4, 2, 3 and 1 keys -- a range between two
    present values and a null test, an equality with a present value, a range at the type's extremes --, four aggregate columns,
    two group columns and four more, eight projected columns with the 1-byte ones among them, and, where a text column lies
    beyond column 8, key sets with byte-string keys on it.  For the newer calls (_newer): topn_by, four order specs with all four
    flag sets, and topn_cols, projected column lists of every row size the columns give, paired with four kinds of limit in
    topn_calls; float_keysets, float_agg and topn_float_by on an int4 / int8 column read as float4 / float8; like_keysets and
    text_by on text_col; set_keysets of at most and of more than eight members; table_keys under the table `table`; buckets,
    [(group columns, a bucket per column)]"""

    def __init__(self, atts, rows, prefer=(), bytes_col=None):
        n = len(atts)
        ints = spread([c for c in range(1, n + 1) if is_int(atts[c - 1])], prefer)
        ones = spread([c for c in range(1, n + 1) if atts[c - 1] == (1, 1)], prefer)
        anycol = spread(list(range(1, n + 1)), prefer)
        pick = lambda i: ints[i % len(ints)]                     # noqa: E731
        present = lambda c: sorted(r[c - 1] for r in rows if len(r) >= c and r[c - 1] is not None)  # noqa: E731
        a, b, c, nullcol = pick(0), pick(1), pick(2), anycol[1 % len(anycol)]
        pa, pb = present(a) or [0], present(b) or [0]
        lo, hi = pa[len(pa) // 4], pa[(3 * len(pa)) // 4]
        ta, tb, tcc = (INT_TYPE[atts[x - 1][0]] for x in (a, b, c))
        cmin, cmax = extremes(atts[c - 1][0])
        self.keysets = [
            [],
            [(a, ta, GE, lo), (a, ta, LE, hi), (nullcol, 0, NOTNULL, 0), (b, tb, NE, extremes(atts[b - 1][0])[0])],
            [(b, tb, EQ, most_common(pb)), (nullcol, 0, ISNULL, 0)],
            [(c, tcc, GE, cmin), (c, tcc, LE, cmax), (a, 0, NOTNULL, 0)],
            [(nullcol, 0, ISNULL, 0)],
        ]
        cap = [x for x in ints if x > 8] or ints                # the captures: beyond bitmap byte 0 wherever the descriptor is
        one = [x for x in ones if x > 8] or ones
        at = lambda i: typed(atts, cap[i % len(cap)])            # noqa: E731
        self.agg_cols = [at(i) for i in range(4)]
        self.by = [at(4), at(1)]
        self.group_cols = [at(i) for i in (5, 0, 2, 3)]
        narrow = cap[:6] + one[:2]
        self.project_cols = [narrow[i % len(narrow)] for i in range(8)]
        texts = spread([c for c in range(9, n + 1) if atts[c - 1][0] == -1], prefer)
        self.bytes_col = bytes_col or (texts[0] if texts else None)
        self.bytes_keysets = []
        if self.bytes_col:
            t = self.bytes_col
            inline = [v.payload if isinstance(v, Long) else v for v in present_any(rows, t) if isinstance(v, (bytes, Long))]
            self.bytes_keysets = [
                [(t, BYTES, GE, b"a"), (t, BYTES, LT, b"b"), (a, ta, GE, lo), (nullcol, 0, NOTNULL, 0)],
                [(t, BYTES, EQ, most_common(inline) if inline else b"a")],
                [(t, BYTES, NE, b"")],
            ]
        self._newer(atts, rows, ints, cap, (a, ta, lo), (b, tb), (c, tcc), nullcol)

    def _newer(self, atts, rows, ints, cap, a, b, c, nullcol):
        """what the newer calls name, from the same columns: order specs, projected column lists of every row size, float, pattern
        and set key sets, a truth table over four keys, buckets and text group columns.  Nothing above depends on it"""
        n = len(atts)
        (a, ta, lo), (b, tb), (c, tcc) = a, b, c
        at = lambda i: cap[i % len(cap)]                         # noqa: E731
        ot = lambda col: INT_TYPE[atts[col - 1][0]]              # noqa: E731
        self.topn_by = [[(at(0), ot(at(0)), 0)],
                        [(at(1), ot(at(1)), DESC), (at(2), ot(at(2)), NULLS_FIRST)],
                        [(at(3), ot(at(3)), DESC | NULLS_FIRST)],
                        [(at(2), ot(at(2)), NULLS_FIRST), (at(0), ot(at(0)), DESC)]]
        narrow = [x for x in range(1, n + 1) if is_narrow(atts[x - 1])]
        wide = sorted(narrow, key=lambda x: (-atts[x - 1][0], x <= 8, x))            # widest first, the far columns before the near
        if is_int(atts[wide[0] - 1]):                            # an order column that every column list below projects
            self.topn_by[3][1] = (wide[0], ot(wide[0]), DESC)
        thin = min(narrow, key=lambda x: (atts[x - 1][0], x <= 8, -x))
        self.topn_cols, sizes = [], set()
        for k in range(1, 9):
            cols = [wide[i % len(wide)] for i in range(k)]
            if k % 2 == 0:
                cols = [thin] + cols[:-1]                        # a narrow column in front: pads inside the row
            size = pr.row_layout(atts, cols)[1]
            if size not in sizes:
                sizes.add(size)
                self.topn_cols.append(cols)
        k = max(8, len(self.topn_cols))                          # every spec, every list and every kind of limit is used
        self.topn_calls = [(i % 4, i % len(self.topn_cols), (i + i // 4) % 4) for i in range(k)]
        floats = [x for x in cap + ints if atts[x - 1][0] in FLOAT_TYPE]
        self.float_col = self.float_agg = None
        self.float_keysets, self.topn_float_by = [], []
        if floats:
            f = floats[0]
            ft = FLOAT_TYPE[atts[f - 1][0]]
            g = next((x for x in floats if x != f), f)
            self.float_col, self.float_agg = (f, ft), (g, FLOAT_TYPE[atts[g - 1][0]])
            self.float_keysets = [[(f, ft, GE, 0.0), (nullcol, 0, NOTNULL, 0)], [(f, ft, LT, float("nan"))]]
            self.topn_float_by = [[(f, ft, 0)], [(f, ft, DESC | NULLS_FIRST), (at(0), ot(at(0)), 0)]]
        texts = [x for x in range(1, n + 1) if atts[x - 1][0] == -1]
        self.text_col = self.bytes_col or (texts[-1] if texts else None)
        t = self.text_col
        self.like_keysets, self.text_by = [], []
        if t:
            ends = (t, BYTES, LIKE, P(b"%b_", utf8=False))       # on the first text column that has a match for it
            tb_ = next((x for x in [t] + texts[::-1] if any(key_state(r, (x,) + ends[1:]) for r in rows)), t)
            self.like_keysets = [
                [(t, BYTES, LIKE, P(b"a%", utf8=True))],
                [(tb_,) + ends[1:]],
                [(t, BYTES, NOT_LIKE, P(b"%\\%%", utf8=True))],
                [(t, BYTES, LIKE, P(b"%", utf8=False))],
                [(t, BYTES, NOT_LIKE, P(b"_%\xe9", utf8=True)), (t, BYTES, LIKE, P(b"%a%", utf8=False))],
            ]
            self.text_by = [[(t, BYTES)], [(t, BYTES), typed(atts, at(0))]]
            if [x for x in texts if x != t]:                     # a second text column, behind an integer column
                self.text_by.append([typed(atts, at(1)), ([x for x in texts if x != t][-1], BYTES)])
        seen = lambda col: sorted({r[col - 1] for r in rows if len(r) >= col and r[col - 1] is not None})  # noqa: E731
        amin, amax = extremes(atts[a - 1][0])
        va, vb = seen(a), seen(b)
        small = sorted(set(va[1:7:2] + [amin, amax]))
        big = sorted(set(va[::2][:20] + [amin, amax] + [7 * i for i in range(-5, 5)]))       # every other present value
        bigb = sorted(set(vb[::2][:20] + list(extremes(atts[b - 1][0])) + [7 * i for i in range(-5, 5)]))
        assert len(small) <= 8 < len(big) and len(bigb) > 8
        self.set_keysets = [[(a, ta, IN, small)], [(a, ta, NOT_IN, small)], [(a, ta, IN, big)],
                            [(a, ta, NOT_IN, big)]]
        third = (t, BYTES, GE, b"a") if t else (c, tcc, LE, 0)
        self.table_keys = [(a, ta, GE, lo), (b, tb, IN, bigb), third, (nullcol, 0, ISNULL, 0)]
        self.table = tr.dnf([0b0011, 0b1100], 4)                 # (A AND B) OR (C AND D)
        eights = [x for x in cap + ints if atts[x - 1][0] == 8]
        bc = typed(atts, eights[0] if eights else at(0))
        oc = typed(atts, next((x for x in cap + ints if x != bc[0]), bc[0]))
        vs = seen(bc[0]) or [0]
        few = (BOUNDS, 0, 0, [-1000, 0, 1000, 1 << 20])
        many = (BOUNDS, 0, 0, list(range(-5000, 5001, 1000)) + [vs[len(vs) // 2]])
        self.buckets = [([bc], [(WIDTH, 0, 1, 1 << 40)]),        # the type's minimum falls below INT64_MIN
                        ([bc, oc] if oc != bc else [bc], [few, RAW] if oc != bc else [few]),
                        ([oc, bc] if oc != bc else [bc], [RAW, many] if oc != bc else [many]),
                        ([bc], [(WIDTH, INFINITE, 0, 1 << 16)])]

    def referenced(self):
        cols = {k[0] for ks in self.keysets + self.bytes_keysets for k in ks}
        return cols | {c for c, _ in self.agg_cols + self.by + self.group_cols} | set(self.project_cols)


def present_any(rows, c):
    return [r[c - 1] for r in rows if len(r) >= c and r[c - 1] is not None]


# ---- blocks ----
class Block:
    """items: [(index of the row, cut or None)]; data: the block's bytes"""

    def __init__(self, items, data):
        self.items, self.data = items, data


def pack(B, pieces, max_items=290):
    """[[index]] : pieces (their lengths) in order, a new block where the next does not fit or the block has max_items"""
    out, cur, room = [], [], B - 8
    for i, ln in enumerate(pieces):
        if cur and (room < tc.maxalign(ln) + 8 or len(cur) >= max_items):
            out.append(cur)
            cur, room = [], B - 8
        assert room >= tc.maxalign(ln) + 8, "a tuple larger than a block"
        cur.append(i)
        room -= tc.maxalign(ln) + 8
    return out + [cur] if cur else out


class Case:
    def __init__(self, name, atts, rows, knobs, B, prefer=(), call_natts=None, bytes_col=None, sweep=None):
        tuples = [make_tuple(atts, r, k) for r, k in zip(rows, knobs)]
        groups = pack(B, [len(t) for t in tuples], min(290, max(1, (len(tuples) + 1) // 2)))[:MAX_BLOCKS]
        kept = sum(len(g) for g in groups)                        # the rows that four blocks hold (all of them, or the first)
        self.name, self.atts, self.B = name, atts, B
        self.rows, self.knobs, self.tuples = rows[:kept], knobs[:kept], tuples[:kept]
        self.call_atts = atts[:call_natts] if call_natts else atts
        self.plan = Plan(self.call_atts, self.rows, prefer, bytes_col)
        self.blocks = [Block([(i, None) for i in g], tc.build_block(B, [tuples[i] for i in g])) for g in groups]
        self.sweep = sweep                                       # (row index, highest cut or None, plan or None) or None
        self._sweeps, self._need = None, {}

    def hoff(self, i):
        return self.tuples[i][22]

    def item_bytes(self, item):
        i, cut = item
        return self.tuples[i] if cut is None else self.tuples[i][:cut]

    def sweep_row(self):
        """the tuple of the cut sweep: as named, else the first full-width one of at most 400 bytes with a NULL in its bitmap that
        passes key set 3 (so that every cut at or beyond `need` has a capture)"""
        if self.sweep:
            return self.sweep[0]
        full = [i for i, r in enumerate(self.rows) if len(r) == len(self.atts) and len(self.tuples[i]) <= 400]
        best = [i for i in full if None in self.rows[i] and expect_match(self.rows[i], self.plan.keysets[3])]
        return (best or full or [min(range(len(self.rows)), key=lambda i: (len(self.rows[i]) != len(self.atts), len(self.tuples[i])))])[0]

    def sweep_plan(self):
        return (self.sweep[2] if self.sweep and self.sweep[2] else None) or self.plan

    def sweeps(self):
        """the blocks of the cut sweep: item c of the sequence is the tuple's first c bytes"""
        if self._sweeps is None:
            i = self.sweep_row()
            t = self.tuples[i]
            top = min(len(t), self.sweep[1]) if self.sweep and self.sweep[1] else len(t)
            groups = pack(SWEEP_B, list(range(1, top + 1)))
            self._sweeps = [Block([(i, c + 1) for c in g], tc.build_block(SWEEP_B, [t[:c + 1] for c in g])) for g in groups]
        return self._sweeps

    # the verdict on an item, by construction
    def verdict(self, item, keys, last, truth=None):
        i, cut = item
        if cut is not None:
            if (i, last) not in self._need:
                self._need[i, last] = need(self.atts, self.rows[i], self.hoff(i), last)
            if cut < self._need[i, last]:
                return TUPLE
        m = expect_match(self.rows[i], keys, truth)
        return UNDECIDED if m is None else OK if m else NOMATCH


# ---- the expectations ----
def as_float(v, typ):
    """the Python float of a float4 / float8 column's stored integer"""
    return struct.unpack("<f", struct.pack("<i", v))[0] if typ == FLOAT4 else struct.unpack("<d", struct.pack("<q", v))[0]


def float_rank(x):
    """what the float order compares: NaN equals NaN and is above everything, -0 equals 0 (as Python's == has it)"""
    return (1, 0.0) if x != x else (0, x)


def key_state(row, key):
    """True, False or None (undecided)"""
    att, typ, op, value = key
    v = row[att - 1] if att <= len(row) else None
    if op == ISNULL:
        return v is None
    if op == NOTNULL:
        return v is not None
    if v is None:
        return False
    if op in (IN, NOT_IN):
        return (v in value) == (op == IN)
    if op in (LIKE, NOT_LIKE):
        if isinstance(v, (Toast, Compressed)):
            return None
        text = v.payload if isinstance(v, Long) else v
        if len(text) > LIKE_MAX:
            return None
        return like_ref.match(bytes(text), value.pattern or b"", value.utf8) == (op == LIKE)
    if typ in (FLOAT4, FLOAT8):
        return _OPS[op](float_rank(as_float(v, typ)), float_rank(float(value)))
    if typ == BYTES:
        if isinstance(v, (Toast, Compressed)):
            return None
        return _OPS[op](v.payload if isinstance(v, Long) else v, value)      # Python orders bytes as unsigned memcmp, then length
    return _OPS[op](v, value)


def expect_match(row, keys, truth=None):
    """True, False or None (undecided: no key is false, and a byte-string key met a value whose bytes are not in the tuple).
    truth: a table W over the keys instead of their AND, read on the masks of the true and the undecided keys as the header
    states it -- tr.verdict_of, the helper truth_key_cases.state_expect reads its block of all key states with"""
    states = [key_state(row, k) for k in keys]
    if truth is not None:
        v = tr.verdict_of([tr.U if s is None else tr.T if s else tr.F for s in states], truth)
        return None if v == UNDECIDED else v == OK
    if any(s is False for s in states):
        return False
    return None if any(s is None for s in states) else True


def _cell(values):
    return (len(values), min(values, default=0), max(values, default=0), sum(values))


def _float_cell(values, typ):
    """what the construction says of a float column's cell: (n, min, max) in the float order, as ranks"""
    ranks = [float_rank(as_float(v, typ)) for v in values]
    return (len(ranks), min(ranks, default=(0, 0.0)), max(ranks, default=(0, 0.0)))


def _cell_of(values, typ):
    return _float_cell(values, typ) if typ in (FLOAT4, FLOAT8) else _cell(values)


def _column(rows, att):
    return [r[att - 1] for r in rows if att <= len(r) and r[att - 1] is not None]


def expect_agg(rows, keys, cols, truth=None):
    """per aggregate column (n, min, max, sum as a Python integer) over the matching rows whose column is not NULL; of a float
    column (n, min, max) as ranks of the float order"""
    hits = [r for r in rows if expect_match(r, keys, truth) is True]
    return [_cell_of(_column(hits, att), typ) for att, typ in cols]


def expect_groups(rows, keys, by, cols, truth=None):
    """{key tuple, None for NULL: (rows of the group, [cell per aggregate column])}"""
    groups = {}
    for r in rows:
        if expect_match(r, keys, truth) is True:
            groups.setdefault(tuple(r[att - 1] if att <= len(r) else None for att, _ in by), []).append(r)
    return {k: (len(rs), [_cell_of(_column(rs, att), typ) for att, typ in cols]) for k, rs in groups.items()}


def _row_bytes(atts, r, cols):
    """(nulls mask, row bytes) of the row r laid out by the projection's rule"""
    offsets, row_bytes = pr.row_layout(atts, cols)
    buf, nulls = bytearray(row_bytes), 0
    for j, att in enumerate(cols):
        v = r[att - 1] if att <= len(r) else None
        if v is None:
            nulls |= 1 << j
        else:
            w = atts[att - 1][0]
            buf[offsets[j]:offsets[j] + w] = int(v).to_bytes(w, "little", signed=True)
    return nulls, bytes(buf)


def expect_rows(atts, rows, keys, cols, truth=None):
    """[(nulls mask, row bytes)] of the matching rows"""
    offsets, row_bytes = pr.row_layout(atts, cols)
    out = []
    for r in rows:
        if expect_match(r, keys, truth) is not True:
            continue
        buf, nulls = bytearray(row_bytes), 0
        for j, att in enumerate(cols):
            v = r[att - 1] if att <= len(r) else None
            if v is None:
                nulls |= 1 << j
            else:
                w = atts[att - 1][0]
                buf[offsets[j]:offsets[j] + w] = int(v).to_bytes(w, "little", signed=True)
        out.append((nulls, bytes(buf)))
    return out


# ---- a call's result against the expectations ----
def _split(case, blk, keys, last, truth=None):
    """(verdict per item, [(pos, row)] of the items that are not TUPLE)"""
    v = [case.verdict(it, keys, last, truth) for it in blk.items]
    return v, [(pos, case.rows[it[0]]) for pos, (it, s) in enumerate(zip(blk.items, v), 1) if s != TUPLE]


def _counts(row, v, what, away=0):
    """away: the matches a group value made undecided, which count in n_bad instead of n_match"""
    got = (int(row["status"]), int(row["n_items"]), int(row["n_match"]), int(row["n_bad"]))
    assert got == (0, len(v), v.count(OK) - away, v.count(TUPLE) + v.count(UNDECIDED) + away), (what, got)


def _total(cell):
    return (int(cell["n"]), int(cell["min"]), int(cell["max"]), (int(cell["sum_hi"]) << 64) + int(cell["sum_lo"]))


def _total_of(cell, typ):
    """a cell as the construction states it: of a float column (n, min, max) as ranks -- the sum is the reference's to check"""
    if typ not in (FLOAT4, FLOAT8):
        return _total(cell)
    if not int(cell["n"]):
        return (0, (0, 0.0), (0, 0.0))
    return (int(cell["n"]), float_rank(as_float(int(cell["min"]), FLOAT8)), float_rank(as_float(int(cell["max"]), FLOAT8)))


def _last(keys, cols=()):
    return max([k[0] for k in keys] + [c[0] if isinstance(c, tuple) else c for c in cols], default=0)


def check_filter(case, blks, keys, result, what="", truth=None):
    table, records, dst = result[:3]
    assert len(table) == len(blks)
    for i, blk in enumerate(blks):
        v, _ = _split(case, blk, keys, _last(keys), truth)
        _counts(table[i], v, (what, i))
        first, n = int(table[i]["rec_first"]), int(table[i]["n_match"]) + int(table[i]["n_bad"])
        got = [(int(r["pos"]), int(r["status"])) for r in records[first:first + n]]
        assert got == [(pos, s) for pos, s in enumerate(v, 1) if s != NOMATCH], (what, i)
        at = int(table[i]["off"])
        for it, s in zip(blk.items, v):
            if s == OK:
                t = case.item_bytes(it)
                assert bytes(dst[at:at + len(t)]) == t and not dst[at + len(t):at + tc.maxalign(len(t))].any(), (what, i, it)
                at += tc.maxalign(len(t))


def check_agg(case, blks, keys, cols, result, what="", truth=None):
    rows, cells = result
    for i, blk in enumerate(blks):
        v, live = _split(case, blk, keys, _last(keys, cols), truth)
        _counts(rows[i], v, (what, i))
        got = [_total_of(c, typ) for c, (_, typ) in zip(cells[i], cols)]
        assert got == expect_agg([r for _, r in live], keys, cols, truth), (what, i)


def check_group(case, blks, keys, by, cols, result, what="", truth=None):
    rows, recs, cells, total = result
    for i, blk in enumerate(blks):
        v, live = _split(case, blk, keys, _last(keys, list(by) + list(cols)), truth)
        _counts(rows[i], v, (what, i))
        first, n = int(rows[i]["first_group"]), int(rows[i]["n_groups"])
        got = {}
        for g in range(first, first + n):
            nulls = int(recs[g]["nulls"])
            key = tuple(None if nulls >> j & 1 else int(recs[g]["key"][j]) for j in range(len(by)))
            assert key not in got, (what, i, key)
            got[key] = (int(recs[g]["n_rows"]), [_total_of(c, typ) for c, (_, typ) in zip(cells[g], cols)])
        assert got == expect_groups([r for _, r in live], keys, by, cols, truth), (what, i)
    assert total == sum(int(r["n_groups"]) for r in rows)


def check_project(case, blks, keys, cols, result, what="", truth=None):
    table, records, out = result[:3]
    for i, blk in enumerate(blks):
        v, live = _split(case, blk, keys, _last(keys, cols), truth)
        _counts(table[i], v, (what, i))
        first, n = int(table[i]["rec_first"]), int(table[i]["n_match"]) + int(table[i]["n_bad"])
        got = [(int(r["pos"]), int(r["status"])) for r in records[first:first + n]]
        assert got == [(pos, s) for pos, s in enumerate(v, 1) if s != NOMATCH], (what, i)
        want = expect_rows(case.call_atts, [r for _, r in live], keys, cols, truth)
        assert [(nulls, row) for _, nulls, row in pr.rows_of(table, records, out, i)] == want, (what, i)


# ---- the ordered scan ----
def _order_value(v, typ, flags):
    """what Python sorts a non-NULL order value by: the integer, or the float's rank; DESC negates"""
    if typ in (FLOAT4, FLOAT8):
        nan, x = float_rank(as_float(v, typ))
        return (-nan, -x) if flags & DESC else (nan, x)
    return -v if flags & DESC else v


def order_key(row, by):
    """((class, value under the direction) per order column) of a row: a NULL before or after every value by NULLS_FIRST"""
    out = []
    for att, typ, flags in by:
        v = row[att - 1] if att <= len(row) else None
        out.append((0 if flags & NULLS_FIRST else 2, 0) if v is None else (1, _order_value(v, typ, flags)))
    return tuple(out)


def expect_topn(rows_with_pos, keys, by, limit, cols, atts, truth=None):
    """(matches, [(pos, key_nulls, nulls, row bytes, [order value or None])] of the first `limit` matching rows in the order)"""
    hits = [(pos, r) for pos, r in rows_with_pos if expect_match(r, keys, truth) is True]
    kept = sorted(hits, key=lambda h: (order_key(h[1], by), h[0]))[:limit]
    out = []
    for pos, r in kept:
        vals = [r[att - 1] if att <= len(r) else None for att, _, _ in by]
        nulls, row = _row_bytes(atts, r, cols)
        out.append((pos, sum(1 << j for j, v in enumerate(vals) if v is None), nulls, row, vals))
    return len(hits), out


def check_topn(case, blks, keys, by, limit, cols, result, what="", truth=None):
    """the table's counts, then the kept rows' pos, key_nulls and nulls, then the row bytes; rec.key for integer order columns
    only -- a float column's reported key is the reference's to check"""
    table, records, rows, total = result
    assert len(table) == len(blks)
    for i, blk in enumerate(blks):
        v, live = _split(case, blk, keys, _last(keys, list(cols) + list(by)), truth)
        _counts(table[i], v, (what, i))
        n_match, want = expect_topn(live, keys, by, limit, cols, case.call_atts, truth)
        at, k = int(table[i]["row_first"]), int(table[i]["n_rows"])
        assert (n_match, k) == (v.count(OK), len(want)), (what, i, k, len(want))
        got = [(int(r["pos"]), int(r["key_nulls"]), int(r["nulls"])) for r in records[at:at + k]]
        assert got == [w[:3] for w in want], (what, i, got, [w[:3] for w in want])
        assert [bytes(r) for r in rows[at:at + k]] == [w[3] for w in want], (what, i)
        for r, w in zip(records[at:at + k], want):
            for j, (_, typ, _) in enumerate(by):
                if typ not in (FLOAT4, FLOAT8) and w[4][j] is not None:
                    assert int(r["key"][j]) == w[4][j], (what, i, w[0], j)
    assert total == sum(int(r["n_rows"]) for r in table)


# ---- grouping by text and by buckets ----
def text_key(v):
    """the group key of a non-NULL value of a text column: its bytes, or AWAY"""
    if isinstance(v, (Toast, Compressed)):
        return AWAY
    text = bytes(v.payload if isinstance(v, Long) else v)
    return AWAY if len(text) > TEXT_MAX else text


def bucket_key(bucket, attlen, v):
    """the group key of the non-NULL integer v of a column of attlen bytes under a bucket (kind, flags, origin, value), or AWAY:
    origin + w * floor((v - origin) / w) in Python integers, AWAY below INT64_MIN; or the greatest boundary <= v, AWAY below
    every boundary.  Under INFINITE the type's two extremes are their own keys and no other value may land on them"""
    kind, flags, origin, value = bucket
    if kind not in (WIDTH, BOUNDS):
        return v
    ends = extremes(attlen)
    if flags & INFINITE and v in ends:
        return v
    if kind == WIDTH:
        key = origin + value * ((v - origin) // value)
        if key < INT64_MIN:
            return AWAY
    else:
        below = [m for m in value if m <= v]
        if not below:
            return AWAY
        key = max(below)
    return AWAY if flags & INFINITE and key in ends else key


def _expect_keyed(rows, keys, by, cols, key_of, truth):
    """({key tuple: (rows of the group, [cell per aggregate column])}, matches that are in no group)"""
    groups, away = {}, 0
    for r in rows:
        if expect_match(r, keys, truth) is not True:
            continue
        key = tuple(None if att > len(r) or r[att - 1] is None else key_of(j, r[att - 1]) for j, (att, _) in enumerate(by))
        if AWAY in key:
            away += 1
        else:
            groups.setdefault(key, []).append(r)
    return {k: (len(rs), [_cell_of(_column(rs, att), typ) for att, typ in cols]) for k, rs in groups.items()}, away


def expect_text_groups(rows, keys, by, cols, truth=None):
    """the groups of a text-group call: a text column's key is its Python bytes, an integer column's its value, None for NULL;
    a match whose text is external, compressed or longer than 32 bytes is in no group"""
    return _expect_keyed(rows, keys, by, cols, lambda j, v: text_key(v) if by[j][1] == BYTES else v, truth)


def expect_bucket_groups(atts, rows, keys, by, cols, buckets, truth=None):
    return _expect_keyed(rows, keys, by, cols, lambda j, v: bucket_key(buckets[j], atts[by[j][0] - 1][0], v), truth)


def _check_keyed(case, blks, keys, by, cols, result, expect, read, what, truth):
    rows, recs, cells, total = result[:4]
    for i, blk in enumerate(blks):
        v, live = _split(case, blk, keys, _last(keys, list(by) + list(cols)), truth)
        want, away = expect([r for _, r in live])
        _counts(rows[i], v, (what, i), away)
        first = int(rows[i]["first_group"])
        got = {}
        for g, (key, n_rows) in enumerate(read(i), first):
            assert key not in got, (what, i, key)
            got[key] = (n_rows, [_total_of(c, typ) for c, (_, typ) in zip(cells[g], cols)])
        assert got == want, (what, i)
    assert total == sum(int(r["n_groups"]) for r in rows)


def check_group_text(case, blks, keys, by, cols, result, what="", truth=None):
    """result: (rows, records, cells, total, key cells); the keys are read back as bytes with group_text_ref.groups_of"""
    _check_keyed(case, blks, keys, by, cols, result, lambda rs: expect_text_groups(rs, keys, by, cols, truth),
                 lambda i: gt.groups_of(result, by, i), what, truth)


def check_group_bucket(case, blks, keys, by, cols, buckets, result, what="", truth=None):
    rows, recs = result[:2]

    def read(i):
        first, n = int(rows[i]["first_group"]), int(rows[i]["n_groups"])
        return [(tuple(None if int(recs[g]["nulls"]) >> j & 1 else int(recs[g]["key"][j]) for j in range(len(by))),
                 int(recs[g]["n_rows"])) for g in range(first, first + n)]
    _check_keyed(case, blks, keys, by, cols, result,
                 lambda rs: expect_bucket_groups(case.call_atts, rs, keys, by, cols, buckets, truth), read, what, truth)


# ---- the descriptors ----
def _random_case(name, atts, seed, B, n_rows, **kw):
    rng = random.Random(seed)
    rows = [draw_row(rng, atts, i) for i in range(n_rows)]
    return Case(name, atts, rows, [draw_knobs(rng) for _ in rows], B, **kw)


def bitmap_edges():
    """40 columns cycling through int2 / int4 / int8 / "char" / text: the referenced columns 8, 9, 16, 17, 32 and 33 sit on both
    sides of the bitmap's byte boundaries; the calls pass the first 34 columns of the 40"""
    atts = [[(2, 2), (4, 4), (8, 8), (1, 1), (-1, 4)][i % 5] for i in range(40)]
    return _random_case("bitmap-edges", atts, 101, 8192, 96, prefer=(8, 9, 16, 17, 32, 33), call_natts=34, bytes_col=10)


def odd_widths():
    """every odd column kind, each followed by an int2, int4 or int8 on which the keys and the captures sit"""
    atts = []
    for i, kind in enumerate(ODD):
        atts += [kind, [(2, 2), (4, 4), (8, 8)][i % 3]]
    return _random_case("odd-widths", atts, 102, 8192, 96, prefer=tuple(range(2, 21, 2)))


def varlena_8():
    """seven "char" columns and a short text shift a text aligned to 8 to every pos % 8; an int8 and an int4 follow it; a second
    text aligned to 8 and an int2 close the tuple.  The text runs through short, long, external and compressed values, 127 bytes
    and more, and 4-byte headers whose low byte is 0 (payloads of 60 and 188 bytes)"""
    atts = [(1, 1)] * 7 + [(-1, 4), (-1, 8), (8, 8), (4, 4), (-1, 8), (2, 2)]
    rng = random.Random(103)
    bodies = [b"abc", Long(b"abc"), Toast(), b"a" * 127, b"b" * 200, Long(b"a" * 60), b"\xe9" * 188, Long(b""), b""]
    rows = []
    for shift in range(8):
        for k, body in enumerate(bodies):
            rows.append([1] * 7 + [b"p" * shift, body, draw_fixed(rng, 8), draw_fixed(rng, 4), Long(b"ab"), k])
        rows.append([None] * (shift % 7) + [2] * (7 - shift % 7) + [None, Compressed(b"Z%d" % shift + b"a" * 20), shift, -shift, None, 5])
    rows += [draw_row(rng, atts, 50 + i) for i in range(24)]
    return Case("varlena-8", atts, rows, [draw_knobs(rng) for _ in rows], 8192, prefer=(10, 11, 13), bytes_col=9, sweep=(35, None, None))


def max_columns():
    """1600 columns: "char" fillers and int4 / int8 at 1593 .. 1600"""
    atts = [(1, 1)] * 1592 + [(4, 4), (8, 8)] * 4
    rng = random.Random(104)
    fill = lambda: [draw_fixed(rng, 1) for _ in range(1592)]                  # noqa: E731
    tail = lambda: [draw_fixed(rng, a[0]) for a in atts[1592:]]               # noqa: E731
    plain = dict(infomask2_flags=0, infomask_flags=0, extra_hoff=0, force_bitmap=False)
    rows, knobs = [], []
    for i in range(4):                                                         # full, no NULL: no bitmap, hoff 24
        rows.append(fill() + tail())
        knobs.append(dict(plain, infomask2_flags=FLAGS[i]))
    for at in (5, 800, 1593, 1600):                                            # full, one NULL: hoff 224
        r = fill() + tail()
        r[at - 1] = None
        rows.append(r)
        knobs.append(dict(plain, infomask2_flags=FLAGS[4], infomask_flags=INFO[3]))
    sweep = len(rows)                                                          # hoff 224, short data: the tuple of the cut sweep
    rows.append([3] * 20 + [None] * 1572 + [7, 1 << 40, None, -9, 11, None, 13, 15])
    knobs.append(plain)
    for at in (1, 9, 1000, 1594):                                              # NULL from some column on
        r = fill() + tail()
        rows.append(r[:at - 1] + [None] * (1601 - at))
        knobs.append(draw_knobs(rng))
    for n in (0, 1, 1592, 1599, 1600):                                         # short tnatts
        rows.append((fill() + tail())[:n])
        knobs.append(draw_knobs(rng))
    for i in range(6):
        rows.append([None if rng.random() < 0.25 else v for v in fill() + tail()])
        knobs.append(draw_knobs(rng))
    near = Plan(atts, rows, prefer=(1593, 1594, 1595))
    near.keysets[3] = [(1593, INT4, GE, extremes(4)[0]), (21, 0, ISNULL, 0)]
    near.agg_cols, near.by, near.group_cols = [(1593, INT4), (1594, INT8), (1593, INT4)], [(1593, INT4)], [(1594, INT8)]
    near.project_cols = [1593, 1594, 1595, 20, 1, 22]
    return Case("max-columns", atts, rows, knobs, 16384, prefer=tuple(range(1593, 1601)), sweep=(sweep, 224 + 64, near))


def random_n(n):
    return _random_case("random-%d" % n, draw_atts(random.Random(200 + n), n), 300 + n, 8192 if n <= 17 else 16384, 96)


def bitmap_edges_dense():
    """the 40 columns of bitmap-edges in blocks of 32 KiB: more than 64 items in a block, so that the index a match is compacted
    to crosses a turn of the wave with wide captures"""
    atts = [[(2, 2), (4, 4), (8, 8), (1, 1), (-1, 4)][i % 5] for i in range(40)]
    return _random_case("bitmap-edges-dense", atts, 1101, 32768, 192, prefer=(8, 9, 16, 17, 32, 33), call_natts=34, bytes_col=10)


NAMES = ["bitmap-edges", "odd-widths", "varlena-8", "max-columns"] + ["random-%d" % n for n in RANDOM_N]
NEW_NAMES = ["bitmap-edges-dense"]
BYTES_NAMES = ["bitmap-edges", "varlena-8", "random-64"]
SWEEP_NAMES = ["bitmap-edges", "odd-widths", "varlena-8", "max-columns"]
_cases = {}


def case(name):
    """the case of that name, made once"""
    if name not in _cases:
        make = {"bitmap-edges": bitmap_edges, "odd-widths": odd_widths, "varlena-8": varlena_8, "max-columns": max_columns,
                "bitmap-edges-dense": bitmap_edges_dense}
        _cases[name] = make[name]() if name in make else random_n(int(name.split("-")[1]))
    return _cases[name]


# ---- tuple-level draws for the property test ----
def draw_tuple_case(rng):
    """(atts, row, knobs, tuple, keys, agg columns, projected columns, newer) from any source of randomness with random.Random's
    methods; newer: (order spec, keys with a set key and -- where a column can carry one -- a float-typed key)"""
    atts = draw_atts(rng, rng.randint(1, 24))
    row = draw_row(rng, atts, 1)
    knobs = draw_knobs(rng)
    ints = [c for c in range(1, len(atts) + 1) if is_int(atts[c - 1])]
    narrow = [c for c in range(1, len(atts) + 1) if is_narrow(atts[c - 1])]
    keys = []
    for _ in range(rng.randint(0, 4)):
        if rng.random() < 0.3:
            keys.append((rng.randint(1, len(atts)), 0, rng.choice((ISNULL, NOTNULL)), 0))
        else:
            c = rng.choice(ints)
            v = row[c - 1] if c <= len(row) and row[c - 1] is not None and rng.random() < 0.5 else draw_fixed(rng, atts[c - 1][0])
            keys.append((c, INT_TYPE[atts[c - 1][0]], rng.randint(LT, NE), v))
    cols = [typed(atts, rng.choice(ints)) for _ in range(rng.randint(1, 4))]
    pcols = [rng.choice(narrow) for _ in range(rng.randint(1, 8))]
    here = lambda c: row[c - 1] if c <= len(row) and row[c - 1] is not None else None  # noqa: E731
    by = []
    for _ in range(rng.randint(1, 2)):
        c = rng.choice(ints)
        floaty = atts[c - 1][0] in FLOAT_TYPE and rng.random() < 0.4
        by.append((c, FLOAT_TYPE[atts[c - 1][0]] if floaty else INT_TYPE[atts[c - 1][0]], rng.choice(FLAG_SETS)))
    c = rng.choice(ints)
    members = [draw_fixed(rng, atts[c - 1][0]) for _ in range(rng.choice((1, 3, 8, 9, 20)))]
    if here(c) is not None and rng.random() < 0.5:
        members[rng.randrange(len(members))] = here(c)
    newer_keys = keys[:2] + [(c, INT_TYPE[atts[c - 1][0]], rng.choice((IN, NOT_IN)), members)]
    floats = [c for c in ints if atts[c - 1][0] in FLOAT_TYPE]
    if floats:
        c = rng.choice(floats)
        typ = FLOAT_TYPE[atts[c - 1][0]]
        consts = [0.0, -0.0, float("nan"), float("inf"), -1.5, as_float(draw_fixed(rng, atts[c - 1][0]), typ)]
        if here(c) is not None:
            consts += [as_float(here(c), typ)] * 3
        newer_keys.append((c, typ, rng.randint(LT, NE), rng.choice(consts)))
    return atts, row, knobs, make_tuple(atts, row, knobs), keys, cols, pcols, (by, newer_keys)
