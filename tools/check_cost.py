#!/usr/bin/env python3
"""Cost of the stored-block check (cryo_codec_check_batch, cryo_codec_check_blocks) against the decode of the same streams.

  device  65 536 x 128 KiB, every distribution, LZ4 acceleration 1 and zstd level 1 (streams of the GPU encoders):
          cryo_codec_check_batch against cryo_codec_decompress_batch, device-resident, HIP events, median of 3
  host    1 024 x 1 MiB `narrow` and `wide`, LZ4-1 and zstd-1: cryo_codec_check_blocks against cryo_codec_decompress_blocks
          (host buffers, the pipelined staging), wall ms, median of 5

usage: python tools/check_cost.py OUT.txt
       python tools/check_cost.py --trace     (one decoded LZ4 batch of 16 384 x 128 KiB per distribution, checked once and
                                               compared once with cryo_codec_compare_batch: run under
                                               rocprofv3 --kernel-trace --stats for k_check_* against k_compare)"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, METHOD_ZSTD, codec as cc  # noqa: E402

LEVEL = 1  # LZ4 acceleration 1, zstd level 1
MNAME = {METHOD_LZ4: "lz4-1", METHOD_ZSTD: "zstd-1"}


def timed(c, fn, reps):
    fn()  # warm-up (workspace)
    c.sync()
    ts = []
    for _ in range(reps):
        c.timer_start()
        fn()
        ts.append(c.timer_stop())
    return statistics.median(ts)


def device_rows(c, reps):
    n, B = 65536, 131072
    rows = []
    cap = (max(cc.bound(METHOD_LZ4, B), cc.bound(METHOD_ZSTD, B)) + 15) & ~15
    bufs = [c.alloc(n * B), c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n), c.alloc(8 * n), c.alloc(n * B), c.alloc(4 * n),
            c.alloc(8 * n)]
    d_src, d_comp, d_sz, d_st, d_off, d_out, d_st2, d_res = bufs
    d_off.upload(np.arange(n, dtype=np.uint64) * np.uint64(cap))
    try:
        for dist in range(5):
            c.synth_batch(0, 0, n, B, dist, d_src)
            for method in (METHOD_LZ4, METHOD_ZSTD):
                c.compress_batch(method, LEVEL, d_src, B, B, n, d_comp, cap, d_sz, d_st)
                c.sync()
                assert (d_st.download(dtype=np.int32) == 0).all(), "encode statuses"
                t_dec = timed(c, lambda: c.decompress_batch(method, d_comp, d_off, d_sz, d_out, B, B, n, d_st2), reps)
                assert (d_st2.download(dtype=np.int32) == 0).all(), "decode statuses"
                t_chk = timed(c, lambda: c.check_batch(method, d_comp, d_off, d_sz, B, n, d_res), reps)
                res = d_res.download(dtype=np.uint32).reshape(n, 2)
                assert (res[:, 0] == cc.CHECK_OK).all(), "check verdicts"
                rows.append(("%s %-6s 65536 x 128KiB device" % (MNAME[method], cc.DIST_NAMES[dist]), t_dec, t_chk, n * B / 1e9))
                print(rows[-1], flush=True)
    finally:
        for x in bufs:
            x.free()
    return rows


def host_rows(c, reps):
    n, B = 1024, 1 << 20
    L = cc.lib()
    rows = []
    d = c.alloc(n * B)
    try:
        for dist in (cc.DIST_NARROW, cc.DIST_WIDE):
            c.synth_batch(0, 0, n, B, dist, d)
            c.sync()
            raws = d.download().reshape(n, B)
            for method in (METHOD_LZ4, METHOD_ZSTD):
                comps = c.compress_blocks(method, LEVEL, [raws[i] for i in range(n)])
                src = (C.c_void_p * n)(*[a.ctypes.data for a in comps])
                szs = (C.c_uint32 * n)(*[a.nbytes for a in comps])
                out = np.empty(n * B, np.uint8)
                st = (C.c_int32 * n)()
                res = np.empty((n, 2), np.uint32)

                def dec():
                    assert L.cryo_codec_decompress_blocks(c.h, method, src, szs, n, out.ctypes.data, B, st) == 0

                def chk():
                    assert L.cryo_codec_check_blocks(c.h, method, src, szs, n, B, res.ctypes.data) == 0

                t = {}
                for name, fn in (("dec", dec), ("chk", chk)):
                    ts = []
                    for r in range(1 + reps):  # the first call is the warm-up
                        t0 = time.perf_counter()
                        fn()
                        if r:
                            ts.append((time.perf_counter() - t0) * 1e3)
                    t[name] = statistics.median(ts)
                assert all(s == 0 for s in st) and np.array_equal(out.reshape(n, B)[n - 1], raws[n - 1])
                assert (res[:, 0] == cc.CHECK_OK).all()
                rows.append(("%s %-6s 1024 x 1MiB host" % (MNAME[method], cc.DIST_NAMES[dist]), t["dec"], t["chk"], n * B / 1e9))
                print(rows[-1], flush=True)
    finally:
        d.free()
    return rows


def trace(c):
    n, B = 16384, 131072
    cap = (cc.bound(METHOD_LZ4, B) + 15) & ~15
    bufs = [c.alloc(n * B), c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n), c.alloc(8 * n), c.alloc(n * B), c.alloc(8 * n),
            c.alloc(8)]
    d_src, d_comp, d_sz, d_st, d_off, d_out, d_res, d_mis = bufs
    d_off.upload(np.arange(n, dtype=np.uint64) * np.uint64(cap))
    try:
        for dist in range(5):
            c.synth_batch(0, 0, n, B, dist, d_src)
            c.compress_batch(METHOD_LZ4, LEVEL, d_src, B, B, n, d_comp, cap, d_sz, d_st)
            c.decompress_batch(METHOD_LZ4, d_comp, d_off, d_sz, d_out, B, B, n, d_st)
            c.check_batch(METHOD_LZ4, d_comp, d_off, d_sz, B, n, d_res)
            d_mis.memset(0)
            c.compare_batch(d_src, B, d_out, B, B, n, d_mis)
            c.sync()
            assert int(d_mis.download(dtype=np.uint64)[0]) == 0
            assert (d_res.download(dtype=np.uint32).reshape(n, 2)[:, 0] == cc.CHECK_OK).all()
    finally:
        for x in bufs:
            x.free()


def main(argv):
    with Codec(0) as c:
        if "--trace" in argv:
            trace(c)
            print("trace shapes done")
            return
        rows = device_rows(c, 3) + host_rows(c, 5)
        version = cc.version()
    lines = ["# r11: stored-block check against the decode of the same streams, %s" % version,
             "# device: HIP-event ms, median of 3; host buffers: wall ms, median of 5; GB/s of decoded (uncompressed) bytes",
             "%-34s %10s %10s %9s %10s %10s" % ("shape", "decode_ms", "check_ms", "delta", "dec_GB/s", "chk_GB/s")]
    for shape, a, b, gb in rows:
        lines.append("%-34s %10.3f %10.3f %+8.1f%% %10.1f %10.1f" % (shape, a, b, 100.0 * (b - a) / a, gb / a * 1e3, gb / b * 1e3))
    txt = "\n".join(lines) + "\n"
    print(txt)
    out = [a for a in argv if not a.startswith("--")]
    with open(out[0] if out else "r11_check.txt", "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main(sys.argv[1:])
