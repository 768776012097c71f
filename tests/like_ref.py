"""Reference of the pattern scan keys (include/cryo_codec.h, "filtering a scan": "Pattern keys"), in plain Python: what the five
scan calls must report when a key's op is CRYO_OP_LIKE or CRYO_OP_NOT_LIKE.  Written from the header's comment, not from the
kernel.  Test infrastructure only.

A key is (att, BYTES, LIKE | NOT_LIKE, P) with P a pg_cryogen_amd.codec.like object: the pattern's bytes, the character rule and
the rsv word the call will carry.  The matcher is the definition taken literally: the pattern is cut into tokens -- a literal
byte, any one character, any run of characters -- and a memoised backtracking search asks whether the whole payload matches the
whole token list; a run of characters is tried at every length, counted in characters from where the '%' stands.  greedy() is
the other statement, the one the kernels are asked to compute: the segments between the '%', each at its leftmost place, no
backtracking; tests/test_like_cpu.py holds the two against each other.

The walk and the payload are bytes_key_ref's (walk, stored_value).  Every other kind of key, the truth table and the block,
call and multi-handle layers are float_ref's and its neighbours', run over this module's key states: every *_call below swaps
float_ref.key_states for the duration of the call (single-threaded test code)."""
import contextlib
import functools
import sys

import bucket_ref as bk
import bytes_key_ref as br
import float_ref as flr
import group_text_ref as gt
import topn_ref as tn
import truth_key_ref as tr
from float_ref import (BYTES, COUNT_ONLY, EQ, GE, GT, HEADER, IN, INT2, INT4, INT8, ISNULL, ITEM, LE, LT, NE, NOMATCH, NOTNULL,  # noqa: F401
                       OK, STREAM, TUPLE, UNDECIDED)
from pg_cryogen_amd.codec import like as P  # noqa: F401  (the value of a pattern key)

LIKE, NOT_LIKE = 11, 12
UTF8 = 0x10000
PATTERN_MAX = 256
TEXT_MAX = 2048
LIT, ANY, RUN = 0, 1, 2


def is_like_key(key):
    return key[2] in (LIKE, NOT_LIKE)


# ---- a pattern ----
def tokens(pattern):
    """[(LIT, byte) | (ANY, None) | (RUN, None)] of a pattern, or None when its last byte is an unescaped backslash"""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == 0x5C:
            if i + 1 == len(pattern):
                return None
            out.append((LIT, pattern[i + 1]))
            i += 2
            continue
        out.append((RUN, None) if c == 0x25 else (ANY, None) if c == 0x5F else (LIT, c))
        i += 1
    return out


def step(text, s, utf8):
    """one character on from s < len(text): one byte and, under utf8, every byte 10xxxxxx that directly follows it"""
    s += 1
    while utf8 and s < len(text) and text[s] & 0xC0 == 0x80:
        s += 1
    return s


def match(text, pattern, utf8):
    """whether the whole of `text` matches the whole of `pattern` (which has no trailing escape): backtracking, memoised"""
    toks, n = tokens(pattern), len(text)
    assert toks is not None
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * (len(toks) + n) + 1000))

    @functools.lru_cache(maxsize=None)
    def at(ti, s):
        if ti == len(toks):
            return s == n
        kind, b = toks[ti]
        if kind == LIT:
            return s < n and text[s] == b and at(ti + 1, s + 1)
        if kind == ANY:
            return s < n and at(ti + 1, step(text, s, utf8))
        while True:                                                       # a run of 0, 1, 2 .. characters from where the '%' stands
            if at(ti + 1, s):
                return True
            if s >= n:
                return False
            s = step(text, s, utf8)
    return at(0, 0)


def greedy(text, pattern, utf8):
    """the same question answered greedily by segments: the first segment at the start when no '%' stands before it; every other
    at its leftmost character start at or after the end of the one before; the last, when no '%' stands behind it, at the start
    from which it ends exactly at the text's end.  No backtracking"""
    toks, n = tokens(pattern), len(text)
    segs, cur, cuts = [], [], 0
    for t in toks:
        if t[0] == RUN:
            if cur:
                segs.append((cur, cuts == 0, False))
            cur, cuts = [], cuts + 1
        else:
            cur.append(t)
    if cur or cuts == 0:
        segs.append((cur, cuts == 0, True))

    def fits(seg, s):
        for kind, b in seg:
            if s >= n or (kind == LIT and text[s] != b):
                return None
            s = s + 1 if kind == LIT else step(text, s, utf8)
        return s
    pos = 0
    for seg, head, tail in segs:
        s = pos
        while True:
            e = fits(seg, s)
            if e is not None and (not tail or e == n):
                pos = e
                break
            if head or s >= n:
                return False
            s = step(text, s, utf8)
    return True


# ---- the descriptor ----
def key_ok(atts, key, rsv=None):
    """the argument rules of one pattern key; rsv: the key's rsv word when it is not P's own"""
    att, typ, op, p = key
    rsv = p.rsv if rsv is None else rsv
    n = rsv & 0xFFFF
    if typ != BYTES or not 1 <= att <= len(atts) or atts[att - 1][0] != -1:
        return False
    if rsv & ~(0xFFFF | UTF8) or n > PATTERN_MAX or (n > 0 and p.pattern is None):
        return False
    return tokens((p.pattern or b"")[:n]) is not None


def desc_ok(atts, keys, flags=0, rsv=0, key_rsv=None):
    """the filter's descriptor rules with pattern keys: every other key and the struct's words by float_ref's rules"""
    others, other_rsv = [], []
    for i, key in enumerate(keys):
        if is_like_key(key):
            if not isinstance(key[3], P) or not key_ok(atts, key, key_rsv[i] if key_rsv else None):
                return False
            others.append((key[0], 0, NOTNULL, 0))                        # the key's place among the four
            other_rsv.append(0)
        else:
            others.append(key)
            other_rsv.append(key_rsv[i] if key_rsv else 0)
    return flr.desc_ok(atts, others, flags, rsv, other_rsv if key_rsv else None)


# ---- a tuple ----
_float_key_states = flr.key_states


def key_states(data, atts, keys, last):
    """float_ref.key_states with pattern keys: None when the walk fails, else T / F / U per key.  A pattern key is F on a NULL
    column, U on a value whose bytes are not in the tuple or number more than TEXT_MAX, else what the matcher says"""
    w = br.walk(data, atts, last)
    if w is None:
        return None
    out = []
    for key in keys:
        if not is_like_key(key):
            out.append(_float_key_states(data, atts, [key], last)[0])
            continue
        att, _, op, p = key
        isnull, at, _ = w[att - 1]
        if isnull:
            out.append(tr.F)
            continue
        payload = br.stored_value(data, at)
        if payload is None or len(payload) > TEXT_MAX:
            out.append(tr.U)
            continue
        out.append(tr.T if match(bytes(payload), p.pattern or b"", p.utf8) == (op == LIKE) else tr.F)
    return out


@contextlib.contextmanager
def _states():
    saved = flr.key_states
    flr.key_states = key_states
    try:
        yield
    finally:
        flr.key_states = saved


def tuple_verdict(data, atts, keys, cols=(), truth=None):
    """(TUPLE | NOMATCH | UNDECIDED | OK, [raw value or None per column of cols] when OK)"""
    with _states():
        return flr.tuple_verdict(data, atts, keys, cols, truth)


# ---- the calls ----
def filter_call(blocks, atts, keys, flags=0, truth=None, b_base=0, r_base=0):
    with _states():
        return flr.filter_call(blocks, atts, keys, flags, truth, b_base, r_base)


def agg_call(blocks, atts, keys, cols, truth=None):
    with _states():
        return flr.agg_call(blocks, atts, keys, cols, truth)


def group_call(blocks, atts, keys, by, cols, truth=None):
    with _states():
        return flr.group_call(blocks, atts, keys, by, cols, truth)


def bucket_group_call(blocks, atts, keys, by, cols, buckets, truth=None):
    with _states():
        return bk.group_call(blocks, atts, keys, by, cols, buckets, truth)


def text_group_call(blocks, atts, keys, by, cols, truth=None):
    with _states():
        return gt.group_call(blocks, atts, keys, by, cols, truth)


def project_call(blocks, atts, keys, cols, truth=None, w_base=0, r_base=0):
    with _states():
        return flr.project_call(blocks, atts, keys, cols, truth, w_base, r_base)


def topn_call(blocks, atts, keys, by, limit, cols, truth=None):
    with _states():
        return tn.topn_call(blocks, atts, keys, by, limit, cols, truth)
