#!/usr/bin/env python3
"""Cost of the tuple fetch through host buffers (cryo_codec_fetch_blocks) against the call it replaces for a bitmap scan,
cryo_codec_decompress_blocks of the same streams, on one MI355X.

  (a) 4 096 x 128 KiB `wide`, 8 tuples per block (an exact bitmap page); (b) 1 024 x 1 MiB `narrow`, all 290 per block (a lossy
  page).  LZ4 streams of the GPU encoder (acceleration 1).  One warm-up call of each path, then per round decompress_blocks,
  fetch_blocks and decompress_blocks again -- the two decompress series give the spread of the yardstick itself -- wall ms
  around the synchronous calls, median / min / max of 20; d2h bytes from the handle's transfer counters.  The fetched tuples of
  a sample of blocks are compared with slices of the decoded blocks after every shape.
  (c) one 1 MiB `narrow` block and one TID per call against cryo_codec_decompress_block: the case that is expected to lose.

usage: python tools/fetch_cost.py > OUT.txt
       python tools/fetch_cost.py --prof    (device-resident: decompress_batch, compare_batch and fetch_batch on (a) and (b), three
                                             calls each: run under rocprofv3 --kernel-trace --stats for the three fetch kernels
                                             next to the decode kernels and k_compare on the same batch)"""
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
SHAPES = [("a", 4096, 131072, cc.DIST_WIDE, "wide", [3, 40, 77, 114, 151, 188, 225, 262]),
          ("b", 1024, 1 << 20, cc.DIST_NARROW, "narrow", list(range(1, 291)))]


def make_streams(c, n, B, dist):
    """n synthetic blocks LZ4-compressed (acceleration 1) on the device; (list of uint8 arrays, device buffers of the batch)"""
    cap = cc.bound(METHOD_LZ4, B)
    d_raw, d_dst, d_sz, d_st = c.alloc(n * B), c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n)
    c.synth_batch(7, 0, n, B, dist, d_raw)
    c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, n, d_dst, cap, d_sz, d_st)
    c.sync()
    assert (d_st.download(dtype=np.int32) == 0).all()
    sz = d_sz.download(dtype=np.uint32)
    raw = d_dst.download()
    out = [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(n)]
    for b in (d_dst, d_st):
        b.free()
    return out, d_raw, d_sz


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def prof(c):
    for tag, n, B, dist, dname, want in SHAPES:
        comps, d_raw, d_sz = make_streams(c, n, B, dist)
        offs = np.zeros(n, np.uint64)
        at = 0
        for i, a in enumerate(comps):
            offs[i] = at
            at += (a.nbytes + 15) & ~15
        packed = np.zeros(at + 64, np.uint8)
        for i, a in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + a.nbytes] = a
        first, pos = cc.request_table([want] * n)
        bufs = [c.alloc(packed.nbytes), c.alloc(8 * n), c.alloc(n * B), c.alloc(4 * n), c.alloc(first.nbytes), c.alloc(pos.nbytes),
                c.alloc(n * B), c.alloc(16 * pos.size), c.alloc(8), c.alloc(8)]
        d_src, d_off, d_dec, d_st, d_first, d_pos, d_dst, d_res, d_tot, d_mis = bufs
        d_src.upload(packed); d_off.upload(offs); d_first.upload(first); d_pos.upload(pos); d_mis.memset(0)
        for _ in range(3):
            c.decompress_batch(METHOD_LZ4, d_src, d_off, d_sz, d_dec, B, B, n, d_st)
            c.compare_batch(d_dec, B, d_raw, B, B, n, d_mis)
            c.fetch_batch(METHOD_LZ4, d_src, d_off, d_sz, B, n, d_first, d_pos, pos.size, d_dst, n * B, d_res, d_tot)
            c.sync()
        assert int(d_mis.download(dtype=np.uint64)[0]) == 0
        print("(%s) %d x %d %s, %d tuples per block: packed total %d bytes" % (tag, n, B, dname, len(want),
                                                                              int(d_tot.download(dtype=np.uint64)[0])), flush=True)
        for b in bufs + [d_raw, d_sz]:
            b.free()


def main():
    L = cc.lib()
    with Codec(0) as c:
        if PROF:
            return prof(c)
        print("%-3s %5s x %-8s %-7s %-26s %10s %10s %10s %14s" % ("", "n", "B", "dist", "call", "median ms", "min ms", "max ms", "d2h bytes"))
        for tag, n, B, dist, dname, want in SHAPES:
            comps, d_raw, d_sz = make_streams(c, n, B, dist)
            d_raw.free(); d_sz.free()
            src = (C.c_void_p * n)(*[a.ctypes.data for a in comps])
            szs = (C.c_uint32 * n)(*[a.nbytes for a in comps])
            raw, st = np.zeros(n * B, np.uint8), np.zeros(n, np.int32)
            first, pos = cc.request_table([want] * n)
            dst, res, tot = np.zeros(n * B, np.uint8), np.zeros(pos.size, cc.FETCH_RESULT), C.c_uint64()

            def decompress():
                assert L.cryo_codec_decompress_blocks(c.h, METHOD_LZ4, src, szs, n, raw.ctypes.data, B, st.ctypes.data) == 0

            def fetch():
                assert L.cryo_codec_fetch_blocks(c.h, METHOD_LZ4, src, szs, n, B, first.ctypes.data, pos.ctypes.data, dst.ctypes.data,
                                                 dst.nbytes, res.ctypes.data, C.byref(tot)) == 0

            series = (("decompress_blocks", decompress), ("fetch_blocks", fetch), ("decompress_blocks (again)", decompress))
            times, d2h = {k: [] for k, _ in series}, {}
            decompress(); fetch()
            for _ in range(20):
                for name, fn in series:
                    t0 = c.transfer_counters()["d2h_bytes"]
                    w = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - w) * 1e3)
                    d2h[name] = c.transfer_counters()["d2h_bytes"] - t0
            assert (st == 0).all() and (res["status"] == 0).all()
            for i in range(0, n, max(1, n // 64)):
                blk = raw[i * B:(i + 1) * B]
                for k, p in enumerate(want):
                    off, ln = struct.unpack_from("<II", blk, 8 + 8 * (p - 1))
                    r = res[i * len(want) + k]
                    assert r["len"] == ln and np.array_equal(dst[int(r["off"]):int(r["off"]) + ln], blk[off:off + ln])
            for name, _ in series:
                print("(%s) %5d x %-8d %-7s %-26s %10.2f %10.2f %10.2f %14d" % ((tag, n, B, dname, name) + stats(times[name]) + (d2h[name],)),
                      flush=True)
            print("        %d tuples per block, packed total %d bytes, compressed in %d bytes, decoded %d bytes" %
                  (len(want), tot.value, sum(a.nbytes for a in comps), n * B), flush=True)
        # (c) one block, one TID
        B = 1 << 20
        comps, d_raw, d_sz = make_streams(c, 1, B, cc.DIST_NARROW)
        d_raw.free(); d_sz.free()
        a = comps[0]
        src, szs = (C.c_void_p * 1)(a.ctypes.data), (C.c_uint32 * 1)(a.nbytes)
        raw = np.zeros(B, np.uint8)
        first, pos = cc.request_table([[145]])
        dst, res, tot = np.zeros(B, np.uint8), np.zeros(1, cc.FETCH_RESULT), C.c_uint64()

        def one_block():
            assert L.cryo_codec_decompress_block(c.h, METHOD_LZ4, a.ctypes.data, a.nbytes, raw.ctypes.data, B) == 0

        def one_tid():
            assert L.cryo_codec_fetch_blocks(c.h, METHOD_LZ4, src, szs, 1, B, first.ctypes.data, pos.ctypes.data, dst.ctypes.data,
                                             dst.nbytes, res.ctypes.data, C.byref(tot)) == 0

        series = (("decompress_block", one_block), ("fetch_blocks, one TID", one_tid), ("decompress_block (again)", one_block))
        times = {k: [] for k, _ in series}
        one_block(); one_tid()
        for _ in range(50):
            for name, fn in series:
                w = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - w) * 1e3)
        assert res[0]["status"] == 0
        for name, _ in series:
            print("(c) %5d x %-8d %-7s %-26s %10.3f %10.3f %10.3f" % ((1, B, "narrow", name) + stats(times[name])), flush=True)


main()
