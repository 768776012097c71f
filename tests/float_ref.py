"""Reference of the float scan keys and float aggregate columns (include/cryo_codec.h: "Float keys", "A float column's cell", "The
reduction"), in plain Python: what the filter, the aggregate, the grouped scan and the projection must report when a key's or an
aggregate column's type is CRYO_KEY_FLOAT4 or CRYO_KEY_FLOAT8.  Written from the header's comment, not from the kernel.  Python
floats are IEEE doubles and +, - round to nearest, so the reduction here is bit-exact.  Test infrastructure only.

A key is (att, type, op, value) as in truth_key_ref; the value of a float key is a Python float or, as an int, the 64 bits of a
double.  A float column's value travels as the signed integer of its bits (4 or 8 bytes), which is what tuple_craft.form_tuple
takes.  The walk, the loads, the byte-string and set keys and the truth table are truth_key_ref's; the filter's and the
projection's call layers are set_key_ref's run over this module's verdict, the aggregate's and the grouping's are restated here
because a float cell needs the matches' positions."""
import contextlib
import struct

import numpy as np

import truth_key_ref as tr
from truth_key_ref import (BYTES, COUNT_ONLY, EQ, GE, GT, HEADER, IN, INT2, INT4, INT8, ISNULL, ITEM, LE, LT, NE, NOMATCH, NOTNULL,  # noqa: F401
                           NOT_IN, OK, OVERLAP, STREAM, TUPLE, UNDECIDED)

sr = tr.sr
ar, br, fr, gr = sr.ar, sr.br, sr.fr, sr.gr

FLOAT4, FLOAT8 = 8, 9
SIZE = {INT2: 2, INT4: 4, INT8: 8, FLOAT4: 4, FLOAT8: 8}
NAN_BITS = 0x7FF8000000000000
INF_BITS = 0x7FF0000000000000
MAG = 0x7FFFFFFFFFFFFFFF
INT64_MAX = (1 << 63) - 1
INF = float("inf")


# ---- bits ----
def f8(x):
    """the signed integer of the bits of the double x: a float8 column's value for form_tuple"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def f4(x):
    """the signed integer of the bits of the single nearest x: a float4 column's value for form_tuple"""
    return struct.unpack("<i", struct.pack("<f", x))[0]


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def double_of(bits):
    return struct.unpack("<d", struct.pack("<Q", bits & (1 << 64) - 1))[0]


def is_float(typ):
    return typ in (FLOAT4, FLOAT8)


def widen(raw, typ):
    """the 64 bits of the double a column's raw value (the signed integer of its bytes) stands for: a float4 is widened, exactly"""
    if typ == FLOAT8:
        return raw & (1 << 64) - 1
    single = struct.unpack("<f", struct.pack("<I", raw & 0xFFFFFFFF))[0]  # struct widens exactly, subnormals included
    b = bits_of(single)
    if single != single:                                                  # a NaN's payload is no concern: every NaN maps alike
        return NAN_BITS | (raw & 0x80000000) << 32
    return b


def key_bits(value):
    """the 64 bits in a float key's value field"""
    return bits_of(value) if isinstance(value, float) else int(value) & (1 << 64) - 1


def fmap(b):
    """the header's map of double bits onto a signed integer in the float order"""
    if b & MAG > INF_BITS:
        return INT64_MAX
    if b & MAG == 0:
        return 0
    m = b ^ (MAG if b >> 63 else 0)
    return m - (1 << 64) if m >> 63 else m


def unmap(m):
    """the canonical double bits of a mapped value"""
    if m == INT64_MAX:
        return NAN_BITS
    u = m & (1 << 64) - 1
    return u ^ (MAG if u >> 63 else 0)


def compare(op, column_bits, constant_bits):
    """a float key's verdict on a non-NULL value, by float8_cmp_internal's order -- stated on doubles, not through the map"""
    a, b = double_of(column_bits), double_of(constant_bits)
    if a != a or b != b:
        c = 0 if (a != a and b != b) else 1 if a != a else -1             # NaN = NaN, NaN above everything else
    else:
        c = (a > b) - (a < b)                                             # -0 == +0, the infinities at the ends
    return fr._compare(op, c, 0)


# ---- the reduction ----
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fast_two_sum(s, t):
    h = s + t
    return h, t - (h - s)


def pair_add(x, y):
    s, t = two_sum(x[0], y[0])
    t = t + (x[1] + y[1])
    return fast_two_sum(s, t)


def reduce_agg(values):
    """the aggregate call's pair: values a list of (position, finite double) in ascending position"""
    leaf = [(0.0, 0.0)] * 64
    for pos, v in values:
        lane = (pos - 1) % 64
        leaf[lane] = pair_add(leaf[lane], (v, 0.0))
    d = 32
    while d:
        leaf = [pair_add(leaf[lane], leaf[lane ^ d]) for lane in range(64)]
        d >>= 1
    return leaf[0]


def reduce_group(values):
    """the grouped call's pair: values as for reduce_agg"""
    acc = (0.0, 0.0)
    for _, v in values:
        acc = pair_add(acc, (v, 0.0))
    return acc


def fold(flags, pair):
    """(sum bits, err bits) from P / M / Q (flags: a set of 'P', 'M', 'Q') and the finite values' pair"""
    if "Q" in flags or {"P", "M"} <= flags:
        return NAN_BITS, 0
    if flags:
        return (INF_BITS if "P" in flags else INF_BITS | 1 << 63), 0
    if any(x != x or abs(x) == INF for x in pair):
        return NAN_BITS, NAN_BITS
    return bits_of(pair[0]), bits_of(pair[1])


def cell_words(values, typ, grouped=False):
    """the five 64-bit words of a float column's cell: values a list of (position, raw value) of the non-NULL matches in
    ascending position"""
    if not values:
        return (0, 0, 0, 0, 0)
    bits = [(pos, widen(raw, typ)) for pos, raw in values]
    mapped = [fmap(b) for _, b in bits]
    flags = set()
    finite = []
    for pos, b in bits:
        if b & MAG > INF_BITS:
            flags.add("Q")
        elif b & MAG == INF_BITS:
            flags.add("M" if b >> 63 else "P")
        else:
            finite.append((pos, double_of(b)))
    s, e = fold(flags, (reduce_group if grouped else reduce_agg)(finite))
    return (len(values), unmap(min(mapped)), unmap(max(mapped)), s, e)


def as_cell(words):
    """five unsigned words as an agg_ref.CELL record"""
    return np.frombuffer(struct.pack("<5Q", *words), ar.CELL)[0]


def cell_of(values, typ, grouped=False):
    """the cell of a column of any type: values a list of (position, raw value)"""
    if is_float(typ):
        return as_cell(cell_words(values, typ, grouped))
    return np.array(ar.cell_of([v for _, v in values]), ar.CELL)


def combine_words(a, b):
    """the header's combination of two float cells (five words each), a before b"""
    if a[0] == 0 or b[0] == 0:
        return tuple(b if a[0] == 0 else a)

    def kind(c):
        s, e = c[3], c[4]
        if e & MAG > INF_BITS:
            return set("V")
        if s & MAG > INF_BITS:
            return set("Q")
        if s & MAG == INF_BITS:
            return set("M" if s >> 63 else "P")
        return set()
    flags = kind(a) | kind(b)
    if flags - {"V"}:
        s, e = fold(flags - {"V"}, (0.0, 0.0))
    elif flags:
        s, e = NAN_BITS, NAN_BITS
    else:
        s, e = fold(set(), pair_add((double_of(a[3]), double_of(a[4])), (double_of(b[3]), double_of(b[4]))))
    return (a[0] + b[0], unmap(min(fmap(a[1]), fmap(b[1]))), unmap(max(fmap(a[2]), fmap(b[2]))), s, e)


# ---- a tuple ----
def _value(data, at, typ):
    size = SIZE[typ]
    assert at % size == 0
    return int.from_bytes(fr.Tuple(data).bytes(at, size), "little", signed=True)


def and_table(nkeys):
    return 1 << ((1 << nkeys) - 1)


def key_states(data, atts, keys, last):
    """truth_key_ref.key_states with float keys: None when the walk fails, else T / F / U per key"""
    w = br.walk(data, atts, last)
    if w is None:
        return None
    out = []
    for key in keys:
        att, typ, op, value = key
        isnull = w[att - 1][0]
        if is_float(typ) and op not in (ISNULL, NOTNULL):
            hit = (not isnull) and compare(op, widen(_value(data, w[att - 1][1], typ), typ), key_bits(value))
            out.append(tr.T if hit else tr.F)
        else:
            out.append(tr.key_states(data, atts, [key], last)[0])
    return out


def tuple_verdict(data, atts, keys, cols=(), truth=None):
    """(TUPLE | NOMATCH | UNDECIDED | OK, [raw value or None per column of cols] when OK)"""
    last = max([k[0] for k in keys] + [c[0] for c in cols], default=0)
    states = key_states(data, atts, keys, last)
    if states is None:
        return TUPLE, None
    v = tr.verdict_of(states, and_table(len(keys)) if truth is None else truth)
    if v != OK:
        return v, None
    w = br.walk(data, atts, last)
    return OK, [None if w[att - 1][0] else _value(data, w[att - 1][1], typ) for att, typ in cols]


def desc_ok(atts, keys, flags=0, rsv=0, key_rsv=None):
    """the filter's descriptor rules with float keys"""
    others, other_rsv = [], []
    for i, key in enumerate(keys):
        att, typ, op, value = key
        if is_float(typ) and op not in (ISNULL, NOTNULL):
            if not 1 <= att <= len(atts) or op in (IN, NOT_IN) or not LT <= op <= NE or (key_rsv and key_rsv[i]):
                return False
            attlen, attalign = atts[att - 1]
            if attlen != SIZE[typ] or attalign < SIZE[typ]:
                return False
            others.append((att, 0, NOTNULL, 0))                          # the key's place among the four
            other_rsv.append(0)
        else:
            others.append(key)
            other_rsv.append(key_rsv[i] if key_rsv else 0)
    return tr.desc_ok(atts, others, flags, rsv, other_rsv if key_rsv else None)


def col_ok(atts, col, group=False):
    """the rule of one aggregate (group=False) or group column"""
    att, typ = col
    if typ not in SIZE or (group and is_float(typ)) or not 1 <= att <= len(atts):
        return False
    attlen, attalign = atts[att - 1]
    return attlen == SIZE[typ] and attalign >= SIZE[typ]


# ---- the calls ----
@contextlib.contextmanager
def _verdict(truth):
    saved = sr.tuple_verdict
    sr.tuple_verdict = lambda data, atts, keys, cols=(): tuple_verdict(data, atts, keys, cols, truth)
    try:
        yield
    finally:
        sr.tuple_verdict = saved


def filter_call(blocks, atts, keys, flags=0, truth=None, b_base=0, r_base=0):
    with _verdict(truth):
        return sr.filter_call(blocks, atts, keys, flags & COUNT_ONLY, b_base, r_base)


def project_call(blocks, atts, keys, cols, truth=None, w_base=0, r_base=0):
    with _verdict(truth):
        return sr.project_call(blocks, atts, keys, cols, w_base, r_base)


def _reduce(block, atts, keys, cols, truth):
    """((status, n_items, n_match, n_bad), [(position, [raw value or None per column])] of the matches in position order)"""
    status, n, items = br._items(block)
    if status != OK:
        return (status, 0, 0, 0), []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    n_bad, rows = 0, []
    for pos, bad, off, ln in items:
        if bad:
            n_bad += 1
            continue
        v, vals = tuple_verdict(b[off:off + ln].tobytes(), atts, keys, cols, truth)
        if v in (TUPLE, UNDECIDED):
            n_bad += 1
        elif v == OK:
            rows.append((pos, vals))
    return (OK, n, len(rows), n_bad), rows


def agg_call(blocks, atts, keys, cols, truth=None):
    """(rows, cells of shape (n, ncols)) of a call, a multi-handle call included"""
    rows, cells = np.zeros(len(blocks), ar.ROW), np.zeros((len(blocks), len(cols)), ar.CELL)
    for i, block in enumerate(blocks):
        rows[i], matches = _reduce(block, atts, keys, cols, truth)
        for j, (_, typ) in enumerate(cols):
            cells[i, j] = cell_of([(pos, m[j]) for pos, m in matches if m[j] is not None], typ)
    return rows, cells


def group_call(blocks, atts, keys, by, cols, truth=None):
    """(rows, records, cells of shape (groups, ncols), total) of a call, a multi-handle call included"""
    rows, recs, cells = np.zeros(len(blocks), gr.ROW), [], []
    for i, block in enumerate(blocks):
        row, matches = _reduce(block, atts, keys, list(by) + list(cols), truth)
        groups = {}
        for pos, m in matches:
            g = groups.setdefault(tuple(m[:len(by)]), [0, [[] for _ in cols]])
            g[0] += 1
            for j, v in enumerate(m[len(by):]):
                if v is not None:
                    g[1][j].append((pos, v))
        rows[i] = row + (len(groups), 0, len(recs))
        for key in sorted(groups, key=gr.order_key):
            k = [0 if v is None else v for v in key] + [0] * (2 - len(key))
            recs.append((k, groups[key][0], sum(1 << j for j, v in enumerate(key) if v is None)))
            cells.append([cell_of(v, cols[j][1], True) for j, v in enumerate(groups[key][1])])
    r = np.zeros(len(recs), gr.REC)
    c = np.zeros((len(recs), len(cols)), ar.CELL)
    for g, rec in enumerate(recs):
        r[g] = rec
        for j, cell in enumerate(cells[g]):
            c[g, j] = cell
    return rows, r, c, len(recs)
