#!/usr/bin/env python3
"""Encode latency of few-block calls with the segment-parallel encoders (CRYO_OPT_ENCODE_SEGMENT_BYTES).

For K = 1 .. 64 blocks per cryo_codec_compress_blocks call (host buffers both ways, PCIe included: what
host/compression.c's cryo_compress and the write-behind staging call), S in {0 (the byte-identical encoders), 8, 16,
32 KiB}, 128 KiB and 1 MiB blocks, `wide`, `narrow` and `int4` data, LZ4 (acceleration 1) and zstd (level 1): the
median wall time of the call, the compressed size against the identical path's (S = 0) on the same blocks, and stock
liblz4 / libzstd on ONE host thread doing the same K blocks one after the other.  Every stream is checked to decode to
its input (device decoder) before it is timed.  Then, for information, the device-resident throughput of 65 536 x 128 KiB
`wide` blocks per call with S = 16 KiB against S = 0.  Not the bench metric.

--strategies: the zstd levels above `fast` instead (CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY = 6, so that every level up to
btlazy2 takes segment mode): one level per strategy and block size (1 MiB: 3 dfast, 5 greedy, 7 lazy, 9 lazy2, 13 btlazy2;
128 KiB: 3, 5, 6, 8, 11), K = 1, 4, 16, 64, S in {4, 16, 32 KiB}; each row has the identical path's latency (S = 0),
segment mode's latency and size against the identical path per S, and stock libzstd at the same level on one host
thread for the K blocks one after the other."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from pg_cryogen_amd import Codec, METHOD_LZ4, METHOD_ZSTD, bound, codec as cc  # noqa: E402
import oracle_lib  # noqa: E402

DIST_NAMES = {0: "wide", 1: "narrow", 2: "int4"}


def med(f, reps):
    v = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        v.append(time.perf_counter() - t0)
    return sorted(v)[len(v) // 2]


def latency_table(c, stock, ora, Ks, Ss, reps):
    L = c.L
    for B in (131072, 1 << 20):
        for dist in (0, 1, 2):
            raws = [ora.synth(3, i, B, dist) for i in range(max(Ks))]
            for method, param, name in ((METHOD_LZ4, 1, "lz4"), (METHOD_ZSTD, 1, "zstd-1")):
                cap = bound(method, B)
                enc1 = (lambda r: stock.lz4_compress(r, param)) if method == METHOD_LZ4 else (lambda r: stock.zstd_compress(r, param))
                cpu = med(lambda: [enc1(r) for r in raws[:8]], 3) / 8 if (stock.lz4 if method == METHOD_LZ4 else stock.zstd) else float("nan")
                print("== %s, %d KiB blocks, %s: stock library on one host thread %.3f ms per block" % (name, B >> 10, DIST_NAMES[dist], cpu * 1e3), flush=True)
                print("   %5s  %s" % ("K", "  ".join("S=%-3s ms     size" % (s >> 10) for s in Ss)) + "    host thread ms", flush=True)
                for K in Ks:
                    raw = np.concatenate(raws[:K])
                    row, base_size = [], None
                    for S in Ss:
                        c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
                        comp = np.zeros(K * cap, np.uint8)
                        sizes = np.zeros(K, np.uint32)

                        def enc():
                            assert L.cryo_codec_compress_blocks(c.h, method, param, raw.ctypes.data, B, K, comp.ctypes.data, cap, sizes.ctypes.data) == 0
                        enc()
                        outs, st = c.decompress_blocks(method, [comp[i * cap:i * cap + int(sizes[i])] for i in range(K)], B)
                        assert (st == 0).all() and all(np.array_equal(o, r) for o, r in zip(outs, raws[:K])), (name, B, S, K)
                        t = med(enc, reps)
                        tot = int(sizes.sum())
                        if S == 0:
                            base_size = tot
                        row.append("%9.3f  %5.3fx" % (t * 1e3, tot / base_size))
                    print("   %5d  %s    %9.3f" % (K, "  ".join(row), cpu * K * 1e3), flush=True)
                c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)


STRATEGY_LEVELS = {1 << 20: [(3, "dfast"), (5, "greedy"), (7, "lazy"), (9, "lazy2"), (13, "btlazy2")],
                   131072: [(3, "dfast"), (5, "greedy"), (6, "lazy"), (8, "lazy2"), (11, "btlazy2")]}


def strategy_table(c, stock, ora, Ks, Ss, sizes, dists, reps):
    L = c.L
    c.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 6)
    for B in sizes:
        cap = bound(METHOD_ZSTD, B)
        for lvl, strat in STRATEGY_LEVELS[B]:
            for dist in dists:
                raws = [ora.synth(3, i, B, dist) for i in range(max(Ks))]
                cpu = med(lambda: [stock.zstd_compress(r, lvl) for r in raws[:4]], 3) / 4 if stock.zstd else float("nan")
                print("== zstd-%d (%s), %d KiB blocks, %s: stock libzstd on one host thread %.3f ms per block"
                      % (lvl, strat, B >> 10, DIST_NAMES[dist], cpu * 1e3), flush=True)
                print("   %5s  %s    host thread ms" % ("K", "  ".join("S=%-3s ms     size  speedup" % (s >> 10) for s in Ss)), flush=True)
                for K in Ks:
                    raw = np.concatenate(raws[:K])
                    row, base_size, base_t = [], None, None
                    for S in Ss:
                        c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
                        comp = np.zeros(K * cap, np.uint8)
                        sizes_ = np.zeros(K, np.uint32)

                        def enc():
                            assert L.cryo_codec_compress_blocks(c.h, METHOD_ZSTD, lvl, raw.ctypes.data, B, K, comp.ctypes.data, cap, sizes_.ctypes.data) == 0
                        enc()
                        outs, st = c.decompress_blocks(METHOD_ZSTD, [comp[i * cap:i * cap + int(sizes_[i])] for i in range(K)], B)
                        assert (st == 0).all() and all(np.array_equal(o, r) for o, r in zip(outs, raws[:K])), (lvl, B, S, K)
                        t = med(enc, reps)
                        tot = int(sizes_.sum())
                        if S == 0:
                            base_size, base_t = tot, t
                        row.append("%9.3f  %5.3fx  %6.1fx" % (t * 1e3, tot / base_size, base_t / t))
                    print("   %5d  %s    %9.3f" % (K, "  ".join(row), cpu * K * 1e3), flush=True)
                c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
    c.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 1)


def throughput(c, n, B, S_list):
    """device-resident: synth on the device, compress_batch timed with the handle's events"""
    print("== device-resident throughput, %d x %d KiB `wide` blocks per call" % (n, B >> 10), flush=True)
    d_src = c.alloc(n * B)
    c.synth_batch(0, 0, n, B, 0, d_src)
    for method, name in ((METHOD_LZ4, "lz4"), (METHOD_ZSTD, "zstd-1")):
        cap = bound(method, B)
        d_dst, d_sz, d_st = c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n)
        for S in S_list:
            c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
            c.compress_batch(method, 1, d_src, B, B, n, d_dst, cap, d_sz, d_st)
            c.sync()
            ts = []
            for _ in range(3):
                c.timer_start()
                c.compress_batch(method, 1, d_src, B, B, n, d_dst, cap, d_sz, d_st)
                ts.append(c.timer_stop())
            st = d_st.download(dtype=np.int32)
            assert (st == 0).all()
            tot = int(d_sz.download(dtype=np.uint32).astype(np.int64).sum())
            ms = sorted(ts)[1]
            print("   %-6s S=%3d KiB: %8.2f ms  %7.2f GB/s  ratio %.4f" % (name, S >> 10, ms, n * B / ms / 1e6, n * B / tot), flush=True)
        c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
        for b in (d_dst, d_sz, d_st):
            b.free()
    d_src.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--throughput-blocks", type=int, default=65536)
    ap.add_argument("--strategies", action="store_true", help="the zstd levels above `fast` (see above)")
    ap.add_argument("--ks", default="1,4,16,64", help="--strategies: blocks per call")
    ap.add_argument("--segs", default="4,16,32", help="--strategies: segment sizes, KiB")
    ap.add_argument("--sizes", default="1048576,131072", help="--strategies: block sizes")
    ap.add_argument("--dists", default="0,1,2", help="--strategies: 0 wide, 1 narrow, 2 int4")
    a = ap.parse_args()
    stock, ora = oracle_lib.StockLibs(), oracle_lib.Oracle()
    ints = lambda v: [int(x) for x in v.split(",")]  # noqa: E731
    with Codec(0) as c:
        if a.strategies:
            strategy_table(c, stock, ora, ints(a.ks), [0] + [k << 10 for k in ints(a.segs)], ints(a.sizes), ints(a.dists), a.reps)
            return
        latency_table(c, stock, ora, [1, 2, 4, 8, 16, 32, 64], [0, 8192, 16384, 32768], a.reps)
        if a.throughput_blocks:
            throughput(c, a.throughput_blocks, 131072, [0, 16384])


if __name__ == "__main__":
    main()
