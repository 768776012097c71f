#!/usr/bin/env python3
"""Cost of the scan filter through host buffers (cryo_codec_filter_blocks) against the call it replaces for a sequential scan
with a range predicate, cryo_codec_decompress_blocks of the same streams, on one MI355X.

  (a) 1 024 x 1 MiB `narrow` (290 tuples of 61 bytes per block) with an int4 range on column 1 at selectivity 0, 1 % and 100 %,
  and the 1 % range with CRYO_FILTER_COUNT_ONLY; (b) 4 096 x 128 KiB `wide` at 1 %.  The int4 column is the generator's rowid,
  which ascends through the relation as an append-only key does: a range of 1 % of the rows is one run of neighbouring blocks.
  LZ4 streams of the GPU encoder (acceleration 1).  One warm-up call of each path, then per round decompress_blocks, every
  filter case and decompress_blocks again -- the two decompress series give the spread of the yardstick itself -- wall ms
  around the synchronous calls, median / min / max of the rounds; d2h bytes from the handle's transfer counters.  The matches of
  every case are compared with the rowids found in the decoded blocks.

usage: python tools/filter_cost.py [--rounds N] > OUT.txt
       python tools/filter_cost.py --prof    (device-resident: decompress_batch and filter_batch at 1 % on (a) and (b), three calls
                                             each: run under rocprofv3 --kernel-trace --stats for the three filter kernels next to
                                             the decode kernels of the same batch, no counters alongside)"""
import ctypes as C
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

PROF = "--prof" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 20
ATTS = [(4, 4), (-1, 4)]
SHAPES = [("a", 1024, 1 << 20, cc.DIST_NARROW, "narrow", (("0 %", 0.0, 0), ("1 %", 0.01, 0), ("100 %", 1.0, 0),
                                                          ("1 %, count only", 0.01, cc.FILTER_COUNT_ONLY))),
          ("b", 4096, 131072, cc.DIST_WIDE, "wide", (("1 %", 0.01, 0),))]


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
        bufs = [c.alloc(packed.nbytes), c.alloc(8 * n), c.alloc(n * B), c.alloc(4 * n), c.alloc(a.nbytes), c.alloc(k.nbytes),
                c.alloc(n * B), c.alloc(8 * 290 * n), c.alloc(32 * n), c.alloc(16)]
        d_src, d_off, d_dec, d_st, d_atts, d_keys, d_dst, d_rec, d_tab, d_tot = bufs
        d_src.upload(packed); d_off.upload(offs); d_atts.upload(a); d_keys.upload(k)
        for _ in range(3):
            c.decompress_batch(METHOD_LZ4, d_src, d_off, d_sz, d_dec, B, B, n, d_st)
            c.filter_batch(METHOD_LZ4, d_src, d_off, d_sz, B, n, len(ATTS), d_atts, len(keys), d_keys, 0, d_dst, n * B, d_rec, 290 * n,
                           d_tab, d_tot)
            c.sync()
        tot = d_tot.download(dtype=np.uint64)
        print("(%s) %d x %d %s, 1 %%: %d records, packed total %d bytes" % (tag, n, B, dname, int(tot[1]), int(tot[0])), flush=True)
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
            raw, st = np.zeros(n * B, np.uint8), np.zeros(n, np.int32)
            dst, rec = np.zeros(n * B, np.uint8), np.zeros(n * 290, cc.FILTER_REC)
            table, tot = np.zeros(n, cc.FILTER_BLOCK), (C.c_uint64 * 2)()

            def decompress():
                assert L.cryo_codec_decompress_blocks(c.h, METHOD_LZ4, src, szs, n, raw.ctypes.data, B, st.ctypes.data) == 0

            def make_filter(share, flags):
                desc = cc.filter_desc(ATTS, range_keys(n, share), flags)

                def run():
                    assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, n, B, C.byref(desc[0]), dst.ctypes.data, dst.nbytes,
                                                      rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                return run

            filters = [("filter_blocks, " + name, make_filter(share, flags), share, flags) for name, share, flags in cases]
            series = [("decompress_blocks", decompress)] + [(nm, fn) for nm, fn, _, _ in filters] + [("decompress_blocks (again)", decompress)]
            times, d2h = {k: [] for k, _ in series}, {}
            for _, fn in series[:-1]:
                fn()
            assert (st == 0).all()
            # what every case must have found: the rowids of the decoded blocks (tuple i of block b: bytes 24 .. 27)
            for name, fn, share, flags in filters:
                fn()
                (_, _, _, lo), (_, _, _, hi) = range_keys(n, share)
                want = max(0, min(hi, n * 290 + 1) - max(lo, 1))
                assert int(table["n_match"].sum()) == want and int(table["n_bad"].sum()) == 0 and (table["status"] == 0).all(), name
                if flags:
                    assert (tot[0], tot[1]) == (0, 0)
                    continue
                assert tot[1] == want
                hit = np.flatnonzero(table["n_match"])
                for i in hit[::max(1, hit.size // 32)]:
                    blk, at = raw[i * B:(i + 1) * B], int(table["off"][i])
                    for r in rec[int(table["rec_first"][i]):int(table["rec_first"][i]) + int(table["n_match"][i])]:
                        off, ln = struct.unpack_from("<II", blk, 8 + 8 * (int(r["pos"]) - 1))
                        assert r["len"] == ln and np.array_equal(dst[at:at + ln], blk[off:off + ln])
                        assert lo <= struct.unpack_from("<i", dst, at + 24)[0] < hi
                        at += (ln + 7) & ~7
            for _ in range(ROUNDS):
                for name, fn in series:
                    t0 = c.transfer_counters()["d2h_bytes"]
                    w = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - w) * 1e3)
                    d2h[name] = c.transfer_counters()["d2h_bytes"] - t0
            base = stats(times["decompress_blocks"])[0]
            for name, _ in series:
                med = stats(times[name])
                print("(%s) %5d x %-8d %-7s %-34s %10.2f %10.2f %10.2f %14d   %.2fx" % ((tag, n, B, dname, name) + med + (d2h[name], base / med[0])),
                      flush=True)
            print("        compressed in %d bytes, decoded %d bytes; last column: median of decompress_blocks over the call's median" %
                  (sum(a.nbytes for a in comps), n * B), flush=True)


main()
