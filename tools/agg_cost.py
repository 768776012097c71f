#!/usr/bin/env python3
"""Cost of the scan aggregate through host buffers (cryo_codec_agg_blocks) against what a caller does without it, on one MI355X.

  Shapes: (a) 1 024 x 1 MiB `narrow` with an int4 range on column 1 (the generator's rowid, which ascends through the relation as
  an append-only key does) at 1 % and 100 % selectivity; (b) 4 096 x 128 KiB `wide` at 1 %.  LZ4 streams of the GPU encoder
  (acceleration 1).
  Yardsticks, the calls a caller has without the aggregate, on the same streams and keys:
    filter + numpy   cryo_codec_filter_blocks, then count / sum / min / max of column 1 over the returned tuples in numpy
    count only       cryo_codec_filter_blocks with CRYO_FILTER_COUNT_ONLY: the floor -- the same decode, 32 bytes per block back
  Against them agg_blocks with one column and with four (the generator has one integer column: column 1 four times).
  One warm-up call of each, then per round: filter + numpy, count only, every aggregate case, count only and filter + numpy again
  (the second count only follows an aggregate call, the first a filter call with its host-side reduction) -- the two series of each yardstick give its own spread --, and filter_blocks without the reduction for reference; wall ms around the synchronous calls, median / min / max of the
  rounds; d2h bytes from the handle's transfer counters.  Every case's cells are compared with the numpy reduction first.

usage: python tools/agg_cost.py [--rounds N] > OUT.txt
       python tools/agg_cost.py --prof    (device-resident: decompress_batch and agg_batch at 1 % on (a) and (b), three calls each:
                                          run under rocprofv3 --kernel-trace --stats for k_agg_block next to the decode kernels of
                                          the same batch, no counters alongside)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

PROF = "--prof" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
ATTS = [(4, 4), (-1, 4)]
COL = (1, cc.KEY_INT4)
SHAPES = [("a", 1024, 1 << 20, cc.DIST_NARROW, "narrow", (("1 %", 0.01), ("100 %", 1.0))),
          ("b", 4096, 131072, cc.DIST_WIDE, "wide", (("1 %", 0.01),))]


def make_streams(c, n, B, dist):
    """n synthetic blocks LZ4-compressed (acceleration 1) on the device; (list of uint8 arrays, device sizes of the batch)"""
    cap = cc.bound(METHOD_LZ4, B)
    d_raw, d_dst, d_sz, d_st = c.alloc(n * B), c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n)
    c.synth_batch(7, 0, n, B, dist, d_raw)
    c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, n, d_dst, cap, d_sz, d_st)
    c.sync()
    assert (d_st.download(dtype=np.int32) == 0).all()
    sz = d_sz.download(dtype=np.uint32)
    raw = d_dst.download()
    out = [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(n)]
    for b in (d_raw, d_dst, d_st):
        b.free()
    return out, d_sz


def range_keys(n, share):
    """an int4 range over `share` of the n x 290 rowids, in the middle of the relation"""
    rows = n * 290
    if share >= 1.0:
        return [(1, cc.KEY_INT4, cc.OP_GE, 1), (1, cc.KEY_INT4, cc.OP_LT, rows + 1)]
    lo = rows // 3
    return [(1, cc.KEY_INT4, cc.OP_GE, lo), (1, cc.KEY_INT4, cc.OP_LT, lo + int(round(rows * share)))]


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def prof(c):
    for tag, n, B, dist, dname, cases in SHAPES:
        comps, d_sz = make_streams(c, n, B, dist)
        offs = np.zeros(n, np.uint64)
        at = 0
        for i, a in enumerate(comps):
            offs[i] = at
            at += (a.nbytes + 15) & ~15
        packed = np.zeros(at + 64, np.uint8)
        for i, a in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + a.nbytes] = a
        keys = range_keys(n, 0.01)
        _, a, k = cc.filter_desc(ATTS, keys)
        _, g = cc.agg_desc([COL] * 4)
        bufs = [c.alloc(packed.nbytes), c.alloc(8 * n), c.alloc(n * B), c.alloc(4 * n), c.alloc(a.nbytes), c.alloc(k.nbytes),
                c.alloc(g.nbytes), c.alloc(16 * n), c.alloc(160 * n)]
        d_src, d_off, d_dec, d_st, d_atts, d_keys, d_cols, d_rows, d_cells = bufs
        d_src.upload(packed); d_off.upload(offs); d_atts.upload(a); d_keys.upload(k); d_cols.upload(g)
        for _ in range(3):
            c.decompress_batch(METHOD_LZ4, d_src, d_off, d_sz, d_dec, B, B, n, d_st)
            c.agg_batch(METHOD_LZ4, d_src, d_off, d_sz, B, n, len(ATTS), d_atts, len(keys), d_keys, 4, d_cols, d_rows, d_cells)
            c.sync()
        rows = d_rows.download().view(cc.AGG_BLOCK)
        print("(%s) %d x %d %s, 1 %%, four columns: %d matches" % (tag, n, B, dname, int(rows["n_match"].sum())), flush=True)
        for b in bufs + [d_sz]:
            b.free()


def main():
    L = cc.lib()
    with Codec(0) as c:
        if PROF:
            return prof(c)
        print("%-3s %5s x %-8s %-7s %-34s %10s %10s %10s %14s" % ("", "n", "B", "dist", "call", "median ms", "min ms", "max ms", "d2h bytes"))
        for tag, n, B, dist, dname, cases in SHAPES:
            comps, d_sz = make_streams(c, n, B, dist)
            d_sz.free()
            src = (C.c_void_p * n)(*[a.ctypes.data for a in comps])
            szs = (C.c_uint32 * n)(*[a.nbytes for a in comps])
            dst, rec = np.zeros(n * B, np.uint8), np.zeros(n * 290, cc.FILTER_REC)
            table, tot = np.zeros(n, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
            rows, cells = np.zeros(n, cc.AGG_BLOCK), np.zeros((n, 4), cc.AGG_CELL)
            for name, share in cases:
                keys = range_keys(n, share)
                fdesc, cdesc = cc.filter_desc(ATTS, keys), cc.filter_desc(ATTS, keys, cc.FILTER_COUNT_ONLY)
                reduced = {}

                def filter_only():
                    assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(fdesc[0]), dst.ctypes.data, dst.nbytes,
                                                      rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0

                def filter_numpy():
                    filter_only()
                    nrec = int(tot[1])                                   # no bad item in these blocks: every record is a match
                    at = np.zeros(nrec, np.int64)                       # a tuple starts where the MAXALIGNed ones before it end
                    if nrec > 1:
                        np.cumsum((rec["len"][:nrec - 1].astype(np.int64) + 7) & ~7, out=at[1:])
                    v = dst.view("<i4")[(at + 24) >> 2].astype(np.int64)  # column 1 of a tuple: bytes 24 .. 27 (t_hoff = 24)
                    reduced["v"] = (v.size, int(v.sum()), int(v.min()) if v.size else 0, int(v.max()) if v.size else 0)

                def count_only():
                    assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(cdesc[0]), None, 0, None, 0,
                                                      table.ctypes.data, tot) == 0

                def make_agg(ncols):
                    adesc = cc.agg_desc([COL] * ncols)

                    def run():
                        assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(fdesc[0]), C.byref(adesc[0]),
                                                       rows.ctypes.data, cells.ctypes.data) == 0
                    return run

                aggs = [("agg_blocks, 1 column", make_agg(1), 1), ("agg_blocks, 4 columns", make_agg(4), 4)]
                series = ([("filter_blocks + numpy", filter_numpy), ("filter_blocks, count only", count_only)] +
                          [(nm, fn) for nm, fn, _ in aggs] +
                          [("filter_blocks, count only (again)", count_only), ("filter_blocks + numpy (again)", filter_numpy),
                           ("filter_blocks alone", filter_only)])
                for _, fn in series[:4]:
                    fn()
                assert (table["status"] == 0).all() and int(table["n_bad"].sum()) == 0
                for nm, fn, ncols in aggs:                               # what every case must have found
                    fn()
                    cs = cells.reshape(-1)[:n * ncols].reshape(n, ncols)
                    assert (rows["status"] == 0).all() and int(rows["n_bad"].sum()) == 0 and int(rows["n_match"].sum()) == reduced["v"][0]
                    for j in range(ncols):
                        has = cs["n"][:, j] > 0
                        got = (int(cs["n"][:, j].sum()), sum(cc.cell_sum(x) for x in cs[:, j]),
                               int(cs["min"][has, j].min()) if has.any() else 0, int(cs["max"][has, j].max()) if has.any() else 0)
                        assert got == reduced["v"], (nm, j, got, reduced["v"])
                times, d2h = {k: [] for k, _ in series}, {}
                for _ in range(ROUNDS):
                    for nm, fn in series:
                        t0 = c.transfer_counters()["d2h_bytes"]
                        w = time.perf_counter()
                        fn()
                        times[nm].append((time.perf_counter() - w) * 1e3)
                        d2h[nm] = c.transfer_counters()["d2h_bytes"] - t0
                base = stats(times["filter_blocks + numpy"])[0]
                for nm, _ in series:
                    med = stats(times[nm])
                    print("(%s) %5d x %-8d %-7s %-34s %10.2f %10.2f %10.2f %14d   %.2fx" %
                          ((tag, n, B, dname, nm) + med + (d2h[nm], base / med[0])), flush=True)
                print("        selectivity %s: %d matches; compressed in %d bytes, decoded %d bytes; last column: median of filter_blocks + "
                      "numpy over the call's median" % (name, reduced["v"][0], sum(a.nbytes for a in comps), n * B), flush=True)


main()
