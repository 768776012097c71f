"""Reference of the truth table over scan keys (include/cryo_codec.h, "filtering a scan": "Truth table"), in plain Python: what the
filter, the aggregate, the grouped scan and the projection must report when CRYO_FILTER_TRUTH combines the keys by a table W
instead of ANDing them.  Written from the header's comment, not from the kernel.  Test infrastructure only.

A key is (att, type, op, value) as in set_key_ref; the walk, the loads, the byte-string and the set keys are that module's.
Here a key has one of three states on a tuple -- T, F or U (a byte-string key on a value whose bytes are not in the tuple) --
and the verdict is read off W: a match if W[t], no match if not W[t | u], UNDECIDED otherwise, with t the mask of the keys that
are T and u of those that are U.  truth=None everywhere means "no flag": the keys are ANDed, which is the AND table's verdict.

The block, call and multi-handle layers are set_key_ref's, run over this module's verdict: every *_call below swaps
set_key_ref.tuple_verdict for the duration of the call (single-threaded test code)."""
import contextlib

import set_key_ref as sr
from set_key_ref import (BYTES, COUNT_ONLY, EQ, GE, GT, HEADER, IN, INT2, INT4, INT8, ISNULL, ITEM, LE, LT, NE, NOMATCH, NOTNULL,  # noqa: F401
                         NOT_IN, OK, OVERLAP, STREAM, TUPLE, UNDECIDED)

TRUTH = 4
MAX_KEYS = 4
T, F, U = "T", "F", "U"


# ---- tables ----
def and_table(nkeys):
    """the table of the flag-less rule: a match only when every key is true"""
    return 1 << ((1 << nkeys) - 1)


def monotone(W, nkeys):
    """W[m] implies W[m | 1 << k] for every k < nkeys"""
    return all(not W >> m & 1 or W >> (m | 1 << k) & 1 for m in range(1 << nkeys) for k in range(nkeys))


def table_ok(W, nkeys):
    """the header's rules for W under the flag"""
    return 1 <= nkeys <= MAX_KEYS and W != 0 and W >> (1 << nkeys) == 0 and monotone(W, nkeys)


def monotone_tables(nkeys):
    """every valid table of nkeys keys, ascending: the monotone Boolean functions less the constant false"""
    return [W for W in range(1, 1 << (1 << nkeys)) if monotone(W, nkeys)]


def dnf(terms, nkeys):
    """the table of an OR of ANDs by brute force: bit m is set when some term's keys are all in m"""
    return sum(1 << m for m in range(1 << nkeys) if any(t & m == t for t in terms))


def desc_ok(atts, keys, flags=0, rsv=0, key_rsv=None):
    """the filter's descriptor rules with the flag: rsv is the struct's rsv word -- the table under TRUTH, reserved without"""
    if flags & TRUTH:
        return table_ok(rsv, len(keys)) and sr.desc_ok(atts, keys, flags & ~TRUTH, 0, key_rsv)
    return sr.desc_ok(atts, keys, flags, rsv, key_rsv)


def reduce_flags_ok(flags):
    """what the aggregate, the grouping and the projection accept in flags"""
    return flags in (0, TRUTH)


# ---- a tuple ----
def key_states(data, atts, keys, last=None):
    """None when the walk fails up to column `last` (default: the highest key column), else the state T / F / U of every key"""
    w = sr.br.walk(data, atts, max([k[0] for k in keys], default=0) if last is None else last)
    if w is None:
        return None
    out = []
    for key in keys:
        att, typ, op, value = key
        isnull, at, _ = w[att - 1]
        if op == ISNULL:
            hit = isnull
        elif op == NOTNULL:
            hit = not isnull
        elif isnull:
            hit = False
        elif sr.is_set_key(key):
            hit = (sr.ar._value(data, at, typ) in value) == (op == IN)
        elif typ == BYTES:
            payload = sr.br.stored_value(data, at)
            hit = None if payload is None else sr.fr._compare(op, sr.br.compare_bytes(payload, value), 0)
        else:
            hit = sr.fr._compare(op, sr.ar._value(data, at, typ), value)
        out.append(U if hit is None else T if hit else F)
    return out


def verdict_of(states, W):
    """OK, NOMATCH or UNDECIDED of a good tuple from its keys' states"""
    t = sum(1 << k for k, s in enumerate(states) if s == T)
    u = sum(1 << k for k, s in enumerate(states) if s == U)
    if W >> t & 1:
        return OK                                                     # true even if every undecided key were false
    if not W >> (t | u) & 1:
        return NOMATCH                                                # false even if every undecided key were true
    return UNDECIDED


def tuple_verdict(data, atts, keys, cols=(), truth=None):
    """set_key_ref.tuple_verdict with a table: (TUPLE | NOMATCH | UNDECIDED | OK, [value or None per column of cols] when OK)"""
    if truth is None:
        return sr.tuple_verdict(data, atts, keys, cols)
    last = max([k[0] for k in keys] + [c[0] for c in cols], default=0)
    states = key_states(data, atts, keys, last)
    if states is None:
        return TUPLE, None
    v = verdict_of(states, truth)
    if v != OK:
        return v, None
    w = sr.br.walk(data, atts, last)
    return OK, [None if w[att - 1][0] else sr.ar._value(data, w[att - 1][1], typ) for att, typ in cols]


# ---- the calls ----
@contextlib.contextmanager
def _table(truth):
    if truth is None:
        yield
        return
    saved = sr.tuple_verdict
    sr.tuple_verdict = lambda data, atts, keys, cols=(): tuple_verdict(data, atts, keys, cols, truth)
    try:
        yield
    finally:
        sr.tuple_verdict = saved


def filter_block(block, atts, keys, truth=None, count_only=False):
    with _table(truth):
        return sr.filter_block(block, atts, keys, count_only)


def filter_call(blocks, atts, keys, flags=0, truth=None, b_base=0, r_base=0):
    """flags: COUNT_ONLY or 0 (TRUTH is implied by truth and ignored here)"""
    with _table(truth):
        return sr.filter_call(blocks, atts, keys, flags & COUNT_ONLY, b_base, r_base)


def multi_filter_call(blocks, atts, keys, G, B, flags=0, truth=None):
    with _table(truth):
        return sr.multi_filter_call(blocks, atts, keys, G, B, flags & COUNT_ONLY)


def agg_call(blocks, atts, keys, cols, truth=None):
    with _table(truth):
        return sr.agg_call(blocks, atts, keys, cols)


def group_call(blocks, atts, keys, by, cols, truth=None):
    with _table(truth):
        return sr.group_call(blocks, atts, keys, by, cols)


def project_call(blocks, atts, keys, cols, truth=None, w_base=0, r_base=0):
    with _table(truth):
        return sr.project_call(blocks, atts, keys, cols, w_base, r_base)


def multi_project_call(blocks, atts, keys, cols, G, truth=None):
    with _table(truth):
        return sr.multi_project_call(blocks, atts, keys, cols, G)
