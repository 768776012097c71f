#!/usr/bin/env python3
"""Cost of set scan keys (CRYO_OP_IN, CRYO_OP_NOT_IN) through host buffers on one MI355X, on the shape of tools/filter_cost.py and
tools/bytes_key_cost.py: 1 024 x 1 MiB `narrow` (290 tuples of 61 bytes per block: an int4 rowid and a text of 32 hex digits),
LZ4 streams of the GPU encoder (acceleration 1).  The keys sit on the rowid, which is unique: a list of n members that are all
present matches n rows ("present"), one whose members are all negative matches none ("absent") -- the search runs its full
length either way, what differs is what comes back.

  filter_blocks with CRYO_FILTER_COUNT_ONLY and agg_blocks over the rowid, each with: no key; rowid >= lo AND rowid <= hi (1 %);
  rowid IN a list of 1, 8, 9, 64 and 1 024 members, present and absent.  8 and 9 stand on either side of the kernels' threshold
  between scanning a set and searching it (filter_walk.h, kSetLinear).

One warm-up call of each, then two series of ROUNDS rounds; a round runs every call once, wall ms around the synchronous call;
median / min / max per series -- the two series of one call give the spread of the measurement itself.  The counts of every case
are compared with what the decoded blocks hold.

usage: python tools/set_key_cost.py [--rounds N] > OUT.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
ATTS = [(4, 4), (-1, 4)]
N, B = 1024, 1 << 20
SIZES = (1, 8, 9, 64, 1024)


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
        rows = N * 290
        assert np.unique(rowid).size == rows and rowid.min() >= 0
        lo = rows // 3
        hi = lo + rows // 100
        dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * 290, cc.FILTER_REC)
        table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
        arows, acells = np.zeros(N, cc.AGG_BLOCK), np.zeros((N, 1), cc.AGG_CELL)
        adesc = cc.agg_desc([(1, cc.KEY_INT4)])

        def count_call(keys, want):
            desc = cc.filter_desc(ATTS, keys, cc.FILTER_COUNT_ONLY)

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

        cases = [("no key", [], rows),
                 ("rowid >= lo AND <= hi, 1 %", [(1, cc.KEY_INT4, cc.OP_GE, lo), (1, cc.KEY_INT4, cc.OP_LE, hi)], int(((rowid >= lo) & (rowid <= hi)).sum()))]
        rng = np.random.default_rng(17)
        for n in SIZES:
            present = rng.choice(rowid, n, replace=False).tolist()
            absent = (-1 - rng.choice(rows, n, replace=False)).tolist()
            cases.append(("IN %d members, present" % n, [(1, cc.KEY_INT4, cc.OP_IN, present)], n))
            cases.append(("IN %d members, absent" % n, [(1, cc.KEY_INT4, cc.OP_IN, absent)], 0))
        series = [("count only, " + name, count_call(keys, want)) for name, keys, want in cases]
        series += [("agg_blocks, " + name, agg_call(keys, want)) for name, keys, want in cases]
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
