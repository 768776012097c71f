#!/usr/bin/env python3
"""Cost of the projecting scan through host buffers (cryo_codec_project_blocks) against the call that did the same job before it
existed: cryo_codec_filter_blocks with the same keys plus a host-side deform of the returned tuples into the same rows, on one
MI355X.

  (a) 1 024 x 1 MiB `narrow` and (b) 4 096 x 128 KiB `wide` generator blocks, an int4 range on column 1 (the generator's rowid,
  which ascends through the relation as an append-only key does) at selectivity 1 % and 100 %, and 1, 3 and 8 projected columns.
  The generator's tuples have one fixed-width column (int4 rowid, text), so the 3- and 8-column projections name it three and
  eight times -- which the contract allows and which costs the kernel what distinct columns of that width would: the walk's
  length is the same, the row grows to 16 and 32 bytes.
  The filter route's deform is the cheapest a host can do for this descriptor, vectorised in numpy: the tuples' offsets from the
  records' MAXALIGNed lengths, then one gather of the four bytes at t_hoff (24: no tuple of the generator has a NULL) per column
  into the same row layout.  A row-at-a-time heap_deform_tuple costs more; the comparison is biased towards the filter.
  LZ4 streams of the GPU encoder (acceleration 1).  One warm-up call of each path, then per round every case -- wall ms around
  the synchronous calls, median / min / max of the rounds; bytes brought back from the handle's transfer counters.  The rows
  of both routes are compared with each other in every case.

usage: python tools/project_cost.py [--rounds N] > OUT.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 20
ATTS = [(4, 4), (-1, 4)]
SHAPES = [("a", 1024, 1 << 20, cc.DIST_NARROW, "narrow"), ("b", 4096, 131072, cc.DIST_WIDE, "wide")]
SHARES = [("1 %", 0.01), ("100 %", 1.0)]
NCOLS = [1, 3, 8]


def make_streams(c, n, B, dist):
    """n synthetic blocks LZ4-compressed (acceleration 1) on the device, as a list of uint8 arrays"""
    cap = cc.bound(METHOD_LZ4, B)
    d_raw, d_dst, d_sz, d_st = c.alloc(n * B), c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n)
    c.synth_batch(7, 0, n, B, dist, d_raw)
    c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, n, d_dst, cap, d_sz, d_st)
    c.sync()
    assert (d_st.download(dtype=np.int32) == 0).all()
    sz = d_sz.download(dtype=np.uint32)
    raw = d_dst.download()
    out = [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(n)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out


def range_keys(rows, share):
    """an int4 range over `share` of the rowids 1 .. rows, in the middle of the relation"""
    if share >= 1.0:
        return [(1, cc.KEY_INT4, cc.OP_GE, 1), (1, cc.KEY_INT4, cc.OP_LT, rows + 1)]
    lo = rows // 3
    return [(1, cc.KEY_INT4, cc.OP_GE, lo), (1, cc.KEY_INT4, cc.OP_LT, lo + int(round(rows * share)))]


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    L = cc.lib()
    with Codec(0) as c:
        print("%-3s %5s x %-8s %-7s %-6s %-5s %-30s %10s %10s %10s %14s" %
              ("", "n", "B", "dist", "share", "cols", "route", "median ms", "min ms", "max ms", "bytes back"))
        for tag, n, B, dist, dname in SHAPES:
            comps = make_streams(c, n, B, dist)
            src = (C.c_void_p * n)(*[a.ctypes.data for a in comps])
            szs = (C.c_uint32 * n)(*[a.nbytes for a in comps])
            dst, frec = np.zeros(n * B, np.uint8), np.zeros(n * 290, cc.FILTER_REC)
            ftable, ftot = np.zeros(n, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
            prec, ptable, ptot = np.zeros(n * 290, cc.PROJECT_REC), np.zeros(n, cc.PROJECT_BLOCK), (C.c_uint64 * 2)()
            # the rows of the relation: a count-only filter without keys
            count = cc.filter_desc(ATTS, [], cc.FILTER_COUNT_ONLY)
            assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(count[0]), None, 0, None, 0, ftable.ctypes.data,
                                              ftot) == 0
            rows_total = int(ftable["n_match"].sum())
            for sname, share in SHARES:
                keys = range_keys(rows_total, share)
                fdesc = cc.filter_desc(ATTS, keys)
                for ncols in NCOLS:
                    cols = [1] * ncols
                    offsets, rb = cc.project_row_layout(ATTS, cols)
                    pdesc = cc.project_desc(cols)
                    prow = np.zeros((n * 290, rb), np.uint8)
                    frow = np.zeros((n * 290, rb), np.uint8)
                    out = {}

                    def project():
                        assert L.cryo_codec_project_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(fdesc[0]), C.byref(pdesc[0]),
                                                           prow.ctypes.data, prow.shape[0], prec.ctypes.data, prec.size,
                                                           ptable.ctypes.data, ptot) == 0
                        out["project"] = int(ptot[0])

                    def filter_and_deform():
                        assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(fdesc[0]), dst.ctypes.data, dst.nbytes,
                                                          frec.ctypes.data, frec.size, ftable.ctypes.data, ftot) == 0
                        r = frec[:int(ftot[1])]
                        r = r[r["status"] == 0]
                        ln = (r["len"].astype(np.int64) + 7) & ~7
                        at = np.cumsum(ln) - ln + 24                       # packed back to back; column 1 at t_hoff = 24
                        val = dst[at[:, None] + np.arange(4)]
                        m = r.size
                        frow[:m] = 0
                        for o in offsets:
                            frow[:m, o:o + 4] = val
                        out["filter"] = m

                    series = [("project_blocks", project), ("filter_blocks + host deform", filter_and_deform)]
                    for _, fn in series:
                        fn()
                    assert out["project"] == out["filter"] > 0 and np.array_equal(prow[:out["project"]], frow[:out["filter"]]), \
                        (tag, sname, ncols)
                    assert (ptable["n_bad"] == 0).all() and (ptable["status"] == 0).all() and (ftable["status"] == 0).all()
                    times, back = {k: [] for k, _ in series}, {}
                    for _ in range(ROUNDS):
                        for name, fn in series:
                            t0 = c.transfer_counters()["d2h_bytes"]
                            w = time.perf_counter()
                            fn()
                            times[name].append((time.perf_counter() - w) * 1e3)
                            back[name] = c.transfer_counters()["d2h_bytes"] - t0
                    base = stats(times["filter_blocks + host deform"])[0]
                    for name, _ in series:
                        med = stats(times[name])
                        print("(%s) %5d x %-8d %-7s %-6s %-5d %-30s %10.2f %10.2f %10.2f %14d   %.2fx" %
                              ((tag, n, B, dname, sname, ncols, name) + med + (back[name], base / med[0])), flush=True)
            print("        %d rows, compressed in %d bytes, decoded %d bytes; last column: median of the filter route over the call's median"
                  % (rows_total, sum(a.nbytes for a in comps), n * B), flush=True)


main()
