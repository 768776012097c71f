#!/usr/bin/env python3
"""Cost of the truth table over scan keys (CRYO_FILTER_TRUTH) through host buffers on one MI355X, on the shape of
tools/set_key_cost.py: 1 024 x 1 MiB `narrow` (290 tuples of 61 bytes per block: an int4 rowid and a text of 32 hex digits), LZ4
streams of the GPU encoder (acceleration 1).  filter_blocks with CRYO_FILTER_COUNT_ONLY and agg_blocks over the rowid, each with:

  (a) rowid >= lo AND rowid <= hi (1 %), no flag: the <false> instantiation of the kernels
  (b) the same two keys with the flag and the AND table: <true>
  (c) (rowid >= lo AND rowid <= hi) OR rowid = x
  (d) rowid >= lo AND rowid <= hi2 AND (rowid IN (64 members) OR tag >= '8'): four keys, A AND B AND (C OR D)
  (s) tag >= '8', no flag: a byte-string key alone, which ran <true> before the table existed

Two questions: what moving an integer-only descriptor from <false> to <true> costs, (b) against (a); and whether flag-less
descriptors that ran <true> before got slower, (s) -- and (a), which must not move at all -- here against a build of the commit
before.  For the second, --flagless measures (a) and (s) alone, which the older library knows, and CRYO_CODEC_LIB (see
pg_cryogen_amd/_loader.py) names a libcryo_codec.so built from the commit before: run this file once per library and series,
alternating, in one session; the yardstick is the spread between the older build's own series, not a number fixed here.

One warm-up call of each, then --series series (default two: A, B) of --rounds rounds; a round runs every call once, wall ms
around the synchronous call; median / min / max per series.  The counts of every case are compared with what the decoded blocks
hold.

usage: [CRYO_CODEC_LIB=OLDER.so] python tools/truth_key_cost.py [--rounds N] [--series N] [--flagless] [--label TEXT] > OUT.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

ROUNDS, SERIES = int(_arg("--rounds", 12)), int(_arg("--series", 2))
FLAGLESS, LABEL = "--flagless" in sys.argv, _arg("--label", "")
ATTS = [(4, 4), (-1, 4)]
N, B = 1024, 1 << 20


def make_streams(c):
    cap = cc.bound(METHOD_LZ4, B)
    d_raw, d_dst, d_sz, d_st = c.alloc(N * B), c.alloc(N * cap), c.alloc(4 * N), c.alloc(4 * N)
    c.synth_batch(7, 0, N, B, cc.DIST_NARROW, d_raw)
    c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, N, d_dst, cap, d_sz, d_st)
    c.sync()
    assert (d_st.download(dtype=np.int32) == 0).all()
    sz = d_sz.download(dtype=np.uint32)
    comp = d_dst.download()
    raw = d_raw.download()
    out = [comp[i * cap:i * cap + int(sz[i])].copy() for i in range(N)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out, raw


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    L = cc.lib()
    with Codec(0) as c:
        comps, raw = make_streams(c)
        src = (C.c_void_p * N)(*[a.ctypes.data for a in comps])
        szs = (C.c_uint32 * N)(*[a.nbytes for a in comps])
        blocks = raw.reshape(N, B)
        items = blocks[:, 8:8 + 8 * 290].copy().view("<u4").reshape(N, 290, 2)
        assert (blocks[:, :4].copy().view("<u4") == 8 + 8 * 290).all() and (items[:, :, 1] == 61).all()
        base = (np.arange(N, dtype=np.int64)[:, None] * B + items[:, :, 0]).ravel()
        rowid = np.stack([raw[base + 24 + k] for k in range(4)], 1).copy().view("<i4").ravel()
        assert (raw[base + 28] == ((32 + 1) << 1 | 1)).all()                  # the tag: a 1-byte header and 32 bytes
        tag0 = raw[base + 29]                                                # its first digit
        rows = N * 290
        assert np.unique(rowid).size == rows and rowid.min() >= 0
        lo = rows // 3
        hi, hi2 = lo + rows // 100, lo + rows // 10
        in_range, in_wide, high = (rowid >= lo) & (rowid <= hi), (rowid >= lo) & (rowid <= hi2), tag0 >= ord("8")
        x = int(rowid[rows // 2 + 1])
        members = np.random.default_rng(17).choice(rowid[in_wide], 64, replace=False)
        dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * 290, cc.FILTER_REC)
        table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
        arows, acells = np.zeros(N, cc.AGG_BLOCK), np.zeros((N, 1), cc.AGG_CELL)
        adesc = cc.agg_desc([(1, cc.KEY_INT4)])

        def desc_of(keys, flags, truth):
            return cc.filter_desc(ATTS, keys, flags) if truth is None else cc.filter_desc(ATTS, keys, flags, truth)

        def count_call(keys, truth, want):
            desc = desc_of(keys, cc.FILTER_COUNT_ONLY, truth)

            def run():
                assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), dst.ctypes.data, dst.nbytes,
                                                  rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                assert int(table["n_match"].sum()) == want and int(table["n_bad"].sum()) == 0
            return run

        def agg_call(keys, truth, want):
            desc = desc_of(keys, 0, truth)

            def run():
                assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), C.byref(adesc[0]),
                                               arows.ctypes.data, acells.ctypes.data) == 0
                assert int(arows["n_match"].sum()) == want == int(acells["n"].sum()) and int(arows["n_bad"].sum()) == 0
            return run

        rng_keys = [(1, cc.KEY_INT4, cc.OP_GE, lo), (1, cc.KEY_INT4, cc.OP_LE, hi)]
        tag_key = (2, cc.KEY_BYTES, cc.OP_GE, b"8")
        cases = [("(a) range, no flag", rng_keys, None, int(in_range.sum())),
                 ("(s) tag >= '8', no flag", [tag_key], None, int(high.sum()))]
        if not FLAGLESS:
            wide = [(1, cc.KEY_INT4, cc.OP_GE, lo), (1, cc.KEY_INT4, cc.OP_LE, hi2), (1, cc.KEY_INT4, cc.OP_IN, members.tolist()), tag_key]
            cases[1:1] = [("(b) range, AND table", rng_keys, cc.truth_dnf([0b11], 2), int(in_range.sum())),
                          ("(c) range OR rowid = x", rng_keys + [(1, cc.KEY_INT4, cc.OP_EQ, x)], cc.truth_dnf([0b011, 0b100], 3),
                           int((in_range | (rowid == x)).sum())),
                          ("(d) A AND B AND (C OR D)", wide, cc.truth_dnf([0b0111, 0b1011], 4),
                           int((in_wide & (np.isin(rowid, members) | high)).sum()))]
        series = [("count only, " + name, count_call(keys, truth, want)) for name, keys, truth, want in cases]
        series += [("agg_blocks, " + name, agg_call(keys, truth, want)) for name, keys, truth, want in cases]
        for _, fn in series:
            fn()
        print("%-44s %8s %10s %10s %10s" % ("call (1 024 x 1 MiB narrow, LZ4, host buffers)", "series", "median ms", "min ms", "max ms"))
        for which in range(SERIES):
            times = {k: [] for k, _ in series}
            for _ in range(ROUNDS):
                for name, fn in series:
                    w = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - w) * 1e3)
            for name, _ in series:
                print("%-44s %8s %10.3f %10.3f %10.3f" % ((name, LABEL + chr(65 + which)) + stats(times[name])), flush=True)


main()
