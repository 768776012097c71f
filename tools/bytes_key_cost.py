#!/usr/bin/env python3
"""Cost of byte-string scan keys (CRYO_KEY_BYTES) through host buffers on one MI355X, beside the integer-key calls of
tools/filter_cost.py on the same shape: 1 024 x 1 MiB `narrow` (290 tuples of 61 bytes per block: an int4 rowid and a text of 32
hex digits under a 1-byte header), LZ4 streams of the GPU encoder (acceleration 1).

  Integer-only descriptors (what must not get slower): filter_blocks with an int4 range of 1 %, the same with
  CRYO_FILTER_COUNT_ONLY, agg_blocks and group_blocks with that range.
  Byte-string keys on the text column: COUNT_ONLY with = <the 32 bytes of one row>, COUNT_ONLY with the range >= '0' AND < '1',
  agg_blocks with the integer range plus =.

One warm-up call of each, then two series of ROUNDS rounds; a round runs every call once, wall ms around the synchronous call;
median / min / max per series -- the two series of one call give the spread of the measurement itself.  The counts of every case
are compared with what the decoded blocks hold.

usage: python tools/bytes_key_cost.py [--rounds N] [--int-only] > OUT.txt
       --int-only: the integer-only calls alone; uses nothing a build without byte-string keys lacks, so the same file measures
       the commit before them"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

INT_ONLY = "--int-only" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
ATTS = [(4, 4), (-1, 4)]
N, B = 1024, 1 << 20
KEY_BYTES = 16


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
        # every tuple's rowid and text, from the decoded blocks: item i of block b at its offset, 61 bytes
        blocks = raw.reshape(N, B)
        items = blocks[:, 8:8 + 8 * 290].copy().view("<u4").reshape(N, 290, 2)
        assert (blocks[:, :4].copy().view("<u4") == 8 + 8 * 290).all() and (items[:, :, 1] == 61).all()
        base = (np.arange(N, dtype=np.int64)[:, None] * B + items[:, :, 0]).ravel()
        rowid = np.stack([raw[base + 24 + k] for k in range(4)], 1).copy().view("<i4").ravel()
        assert (raw[base + 28] == ((32 + 1) << 1 | 1)).all()
        text = np.stack([raw[base + 29 + k] for k in range(32)], 1)
        rows = N * 290
        lo = rows // 3
        hi = lo + rows // 100
        in_range = (rowid >= lo) & (rowid < hi)
        int_keys = [(1, cc.KEY_INT4, cc.OP_GE, lo), (1, cc.KEY_INT4, cc.OP_LT, hi)]
        dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * 290, cc.FILTER_REC)
        table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
        arows, acells = np.zeros(N, cc.AGG_BLOCK), np.zeros((N, 1), cc.AGG_CELL)
        grows, grecs, gcells, gtot = np.zeros(N, cc.GROUP_BLOCK), np.zeros(N * 290, cc.GROUP_REC), np.zeros((N * 290, 1), cc.AGG_CELL), C.c_uint64()
        adesc, gdesc = cc.agg_desc([(1, cc.KEY_INT4)]), cc.group_desc([(1, cc.KEY_INT4)])

        def filter_call(keys, flags, want):
            desc = cc.filter_desc(ATTS, keys, flags)

            def run():
                assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), dst.ctypes.data, dst.nbytes,
                                                  rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                assert int(table["n_match"].sum()) == want and int(table["n_bad"].sum()) == 0
            return run

        def agg_call(keys, want):
            desc = cc.filter_desc(ATTS, keys)

            def run():
                assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), C.byref(adesc[0]),
                                               arows.ctypes.data, acells.ctypes.data) == 0
                assert int(arows["n_match"].sum()) == want == int(acells["n"].sum()) and int(arows["n_bad"].sum()) == 0
            return run

        def group_call(keys, want):
            desc = cc.filter_desc(ATTS, keys)

            def run():
                assert L.cryo_codec_group_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), C.byref(gdesc[0]), C.byref(adesc[0]),
                                                 grows.ctypes.data, grecs.ctypes.data, grecs.size, gcells.ctypes.data, C.byref(gtot)) == 0
                assert int(grows["n_match"].sum()) == want == gtot.value
            return run

        n_int = int(in_range.sum())
        series = [("filter_blocks, int4 range 1 %", filter_call(int_keys, 0, n_int)),
                  ("filter_blocks, int4 range 1 %, count only", filter_call(int_keys, cc.FILTER_COUNT_ONLY, n_int)),
                  ("agg_blocks, int4 range 1 %", agg_call(int_keys, n_int)),
                  ("group_blocks, int4 range 1 %", group_call(int_keys, n_int))]
        if not INT_ONLY:
            one = bytes(text[rows // 2])
            n_eq = int((text == np.frombuffer(one, np.uint8)).all(1).sum())
            n_rng = int((text[:, 0] == ord("0")).sum())                  # >= '0' AND < '1': the texts that begin with '0'
            mine = bytes(text[np.flatnonzero(in_range)[5]])                  # the text of a row inside the integer range
            n_both = int((in_range & (text == np.frombuffer(mine, np.uint8)).all(1)).sum())
            assert n_eq >= 1 and n_both >= 1
            text_eq = [(2, KEY_BYTES, cc.OP_EQ, one)]
            text_rng = [(2, KEY_BYTES, cc.OP_GE, b"0"), (2, KEY_BYTES, cc.OP_LT, b"1")]
            series += [("count only, text = 32 bytes", filter_call(text_eq, cc.FILTER_COUNT_ONLY, n_eq)),
                       ("count only, text >= '0' AND < '1'", filter_call(text_rng, cc.FILTER_COUNT_ONLY, n_rng)),
                       ("agg_blocks, int4 range 1 % AND text =", agg_call(int_keys + [(2, KEY_BYTES, cc.OP_EQ, mine)], n_both))]
            print("matches: int4 range %d, text = %d, text range %d, both %d of %d rows" % (n_int, n_eq, n_rng, n_both, rows), flush=True)
        for _, fn in series:
            fn()
        print("%-44s %6s %10s %10s %10s" % ("call (1 024 x 1 MiB narrow, LZ4, host buffers)", "series", "median ms", "min ms", "max ms"))
        for which in ("A", "B"):
            times = {k: [] for k, _ in series}
            for _ in range(ROUNDS):
                for name, fn in series:
                    w = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - w) * 1e3)
            for name, _ in series:
                print("%-44s %6s %10.3f %10.3f %10.3f" % ((name, which) + stats(times[name])), flush=True)


main()
