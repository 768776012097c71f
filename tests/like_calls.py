"""What the GPU tests of the pattern keys share: the batches around a hand-made block, the seeded random blocks and descriptors
of the per-call tests, and the device-resident filter call that also reads the caller's patterns back.  The other calls are
tests/truth_calls.py's and tests/topn_calls.py's, which drive pattern keys unchanged.  Test infrastructure only."""
import random
import struct

import numpy as np

import group_text_cases as gc
import like_ref as lr
import scan_calls
import tuple_craft as tc
from like_ref import P
from pg_cryogen_amd import codec as cc
from scan_calls import SENTINEL
from tuple_craft import Long, Toast

WIDE = gc.ATTS                                                          # (id int4, t text, x int8, u text, d int4, f float8)
WIDE_B = 16384
FLOAT8 = lr.flr.FLOAT8


def other_block(B, atts):
    """a block of other tuples over any descriptor: integers by position, varlenas 'de', 'needle' or an external pointer"""
    tuples = []
    for i in range(1, 31):
        vals = []
        for attlen, _ in atts:
            vals.append(i % 7 - 3 if attlen > 0 else Toast() if i % 6 == 0 else b"de" if i % 2 else b"xneedle" * (i % 4))
        tuples.append(tc.form_tuple(atts, vals))
    return tc.build_block(B, tuples)


def batch(idx, blk, B, atts, sizes=(1, 4, 5, 9)):
    """a lone wave, a full workgroup, one over, two over, alternating with a block of other tuples"""
    return [blk if j % 2 == 0 else other_block(B, atts) for j in range(sizes[idx % len(sizes)])]


def filter_batch(codec, method, comps, B, atts, keys, flags=0, truth=None, shift=1):
    """truth_calls.filter_batch with the constants and patterns at ptr + shift, read back after the call beside the key array:
    the library must have written neither"""
    n = len(comps)
    with scan_calls.Device(codec, comps, atts, keys, shift) as d:
        consts = cc.filter_desc_device(atts, keys)[2]
        dst, rec = d.alloc(n * B + 64, SENTINEL), d.alloc(8 * 290 * n + 64, SENTINEL)
        tab, tot = d.alloc(32 * n, 0xEE), d.alloc(16, 0xEE)
        codec.filter_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, flags, dst, n * B,
                           rec, 290 * n, tab, tot, truth=truth)
        codec.sync()
        d.keys_untouched()
        assert np.array_equal(d.consts.download(consts.nbytes + shift)[shift:], consts), "the caller's patterns were written"
        t = tot.download(dtype=np.uint64)
        return (tab.download(dtype=np.uint8).view(cc.FILTER_BLOCK).copy(), rec.download(dtype=np.uint8).view(cc.FILTER_REC).copy(),
                dst.download(), (int(t[0]), int(t[1])))


# ---- seeded random blocks over the wide descriptor ----
WORDS = [b"utm_source=", b"com.adjust.", b"bot", b"Mozilla/5.0", "café".encode(), "€uro".encode(), b"/path", b"?q=", b"x", b"", b"%", b"_"]
PATTERNS = ["%utm_source=%", "com.adjust.%", "%bot%", "%caf_", "_%€%", "%/path%?q=%", "%x", "Mozilla%bot", "%\\%%", "%\\_", "%_x_%", "%é%bot%"]


def f8(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def random_text(rnd):
    return b"".join(rnd.choice(WORDS) for _ in range(rnd.randrange(6)))


def random_block(rnd, B=WIDE_B, n=110):
    """n tuples (id, t, x, u, d, f): t a few words -- now and then NULL, external, under a 4-byte header or some loose bytes of
    UTF-8 --, u one of a few short texts, the numbers small"""
    tuples = []
    for i in range(1, n + 1):
        r = rnd.randrange(40)
        t = random_text(rnd)
        t = None if r == 0 else Toast() if r == 1 else Long(t) if r < 5 else t + bytes([rnd.choice([0x80, 0xC3, 0xE2])]) if r < 8 else t
        u = rnd.choice([b"de", b"fr", b"us", "österreich".encode(), None, b"bot"])
        tuples.append(tc.form_tuple(WIDE, [i, t, rnd.randrange(-50, 50), u, rnd.randrange(6), f8(rnd.choice([0.5, -1.25, 3.0, float("inf"), 1e300]))]))
    return tc.build_block(B, tuples)


def random_keys(rnd):
    """(keys, truth): one or two pattern keys on t and u, now and then beside an integer or a byte-string key, ANDed or ORed"""
    keys = [(2, lr.BYTES, rnd.choice([lr.LIKE, lr.LIKE, lr.NOT_LIKE]), P(rnd.choice(PATTERNS), utf8=rnd.random() < 0.7))]
    r = rnd.randrange(4)
    if r == 0:
        keys.append((4, lr.BYTES, rnd.choice([lr.LIKE, lr.NOT_LIKE]), P(rnd.choice(["%e%", "_r", "%bot", "ö%"]))))
    elif r == 1:
        keys.append((3, lr.INT8, lr.GE, rnd.randrange(-40, 0)))
    elif r == 2:
        keys.append((4, lr.BYTES, lr.NE, b"us"))
    truth = None if len(keys) == 1 or rnd.random() < 0.5 else 0b1110
    return keys, truth


def random_call(seed, nblocks=3):
    """(blocks, keys, truth) such that every block holds a match and a tuple that is none by the reference: a kernel that answers
    a constant cannot pass.  The seed decides everything"""
    rnd = random.Random(seed)
    blocks = [random_block(rnd) for _ in range(nblocks)]
    for _ in range(200):
        keys, truth = random_keys(rnd)
        table = lr.filter_call(blocks, WIDE, keys, lr.COUNT_ONLY, truth)[0]
        if (table["n_match"] > 0).all() and (table["n_match"] + table["n_bad"] < table["n_items"]).all():
            return blocks, keys, truth
    raise AssertionError("no descriptor with a match and a non-match in every block")
