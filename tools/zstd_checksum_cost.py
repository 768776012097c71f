#!/usr/bin/env python3
"""Cost of zstd content checksums (CRYO_OPT_ZSTD_CHECKSUM): the same work with frames without and with a checksum.

  encode  65 536 x 128 KiB `wide`, zstd level 1, cryo_codec_compress_batch (device-resident), HIP events, median of 3
  decode  those frames, cryo_codec_decompress_batch (device-resident), HIP events, median of 3
  read    one 1 MiB `wide` / `narrow` frame per call through cryo_codec_decompress_block (host buffers: PCIe both ways
          included), wall ms, median of 50
  K=8     8 x 1 MiB `wide` frames per call, cryo_codec_decompress_batch (device-resident), HIP events, median of 30

usage: python tools/zstd_checksum_cost.py OUT.txt
       python tools/zstd_checksum_cost.py --trace     (the shapes alone, once each with checksums: run under
                                                       rocprofv3 --kernel-trace --stats for the kernels' own times)"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_ZSTD, codec as cc  # noqa: E402

LEVEL = 1


def encode(c, d_src, n, B, d_dst, d_sz, d_st, reps):
    cap = cc.bound(METHOD_ZSTD, B)
    c.compress_batch(METHOD_ZSTD, LEVEL, d_src, B, B, n, d_dst, cap, d_sz, d_st)  # warm-up (workspace)
    c.sync()
    ts = []
    for _ in range(reps):
        c.timer_start()
        c.compress_batch(METHOD_ZSTD, LEVEL, d_src, B, B, n, d_dst, cap, d_sz, d_st)
        ts.append(c.timer_stop())
    assert (d_st.download(dtype=np.int32) == 0).all(), "encode statuses"
    return statistics.median(ts) if ts else 0.0


def decode(c, d_comp, d_off, d_sz, n, B, d_out, d_st, reps, d_src=None):
    c.decompress_batch(METHOD_ZSTD, d_comp, d_off, d_sz, d_out, B, B, n, d_st)  # warm-up (workspace)
    c.sync()
    ts = []
    for _ in range(reps):
        c.timer_start()
        c.decompress_batch(METHOD_ZSTD, d_comp, d_off, d_sz, d_out, B, B, n, d_st)
        ts.append(c.timer_stop())
    assert (d_st.download(dtype=np.int32) == 0).all(), "decode statuses"
    if d_src is not None:   # a sample of blocks back against the input
        for i in (0, n // 2, n - 1):
            assert np.array_equal(d_out.download(B, i * B), d_src.download(B, i * B)), i
    return statistics.median(ts) if ts else 0.0


def read_one(c, comp, B, want, reps):
    ts = []
    for r in range(5 + reps):
        t0 = time.perf_counter()
        out = c.decompress_block(METHOD_ZSTD, comp, B)
        if r >= 5:
            ts.append((time.perf_counter() - t0) * 1e3)
    assert out is not None and np.array_equal(out, want)
    return statistics.median(ts) if ts else 0.0


def run(trace=False):
    rows = []
    reps_bulk, reps_read, reps_k8 = (0, 0, 0) if trace else (3, 50, 30)
    with Codec(0) as c:
        # bulk: 65 536 x 128 KiB
        n, B = 65536, 131072
        cap = cc.bound(METHOD_ZSTD, B)
        d_src, d_dst, d_sz, d_st = c.alloc(n * B), c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n)
        d_off, d_out, d_dst_st = c.alloc(8 * n), c.alloc(n * B), c.alloc(4 * n)
        c.synth_batch(0, 0, n, B, cc.DIST_WIDE, d_src)
        d_off.upload(np.arange(n, dtype=np.uint64) * np.uint64(cap))
        t_enc, t_dec, total = [], [], []
        for v in ((1,) if trace else (0, 1)):
            c.set_option(cc.OPT_ZSTD_CHECKSUM, v)
            t_enc.append(encode(c, d_src, n, B, d_dst, d_sz, d_st, reps_bulk))
            total.append(int(d_sz.download(dtype=np.uint32).astype(np.uint64).sum()))
            t_dec.append(decode(c, d_dst, d_off, d_sz, n, B, d_out, d_dst_st, reps_bulk, d_src))
        if not trace:
            gb = n * B / 1e9
            rows.append(("encode 65536 x 128KiB wide (device)", t_enc[0], t_enc[1], gb))
            rows.append(("decode 65536 x 128KiB wide (device)", t_dec[0], t_dec[1], gb))
            assert total[1] == total[0] + 4 * n
        for x in (d_src, d_dst, d_sz, d_st, d_off, d_out, d_dst_st):
            x.free()
        # one 1 MiB frame per call (host buffers)
        B1 = 1 << 20
        d = c.alloc(8 * B1)
        blocks = {}
        for dist in (cc.DIST_WIDE, cc.DIST_NARROW):
            c.synth_batch(0, 7, 1, B1, dist, d)
            c.sync()
            blocks[cc.DIST_NAMES[dist]] = d.download(B1).copy()
        for name, blk in blocks.items():
            t = []
            for v in ((1,) if trace else (0, 1)):
                c.set_option(cc.OPT_ZSTD_CHECKSUM, v)
                comp = c.compress_block(METHOD_ZSTD, LEVEL, blk)
                t.append(read_one(c, comp, B1, blk, reps_read) if not trace else c.decompress_block(METHOD_ZSTD, comp, B1) is not None)
            if not trace:
                rows.append(("read 1 x 1MiB %s (host buffers)" % name, t[0], t[1], B1 / 1e9))
        # K = 8 x 1 MiB per call (device-resident)
        k = 8
        cap1 = cc.bound(METHOD_ZSTD, B1)
        d_dst, d_sz, d_st, d_off, d_out, d_st2 = c.alloc(k * cap1), c.alloc(4 * k), c.alloc(4 * k), c.alloc(8 * k), c.alloc(k * B1), c.alloc(4 * k)
        c.synth_batch(0, 100, k, B1, cc.DIST_WIDE, d)
        d_off.upload(np.arange(k, dtype=np.uint64) * np.uint64(cap1))
        t = []
        for v in ((1,) if trace else (0, 1)):
            c.set_option(cc.OPT_ZSTD_CHECKSUM, v)
            encode(c, d, k, B1, d_dst, d_sz, d_st, 0)
            t.append(decode(c, d_dst, d_off, d_sz, k, B1, d_out, d_st2, reps_k8, d))
        if not trace:
            rows.append(("decode 8 x 1MiB wide (device)", t[0], t[1], k * B1 / 1e9))
        for x in (d, d_dst, d_sz, d_st, d_off, d_out, d_st2):
            x.free()
        c.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
        version = cc.version()
    return rows, version


def main(argv):
    if "--trace" in argv:
        run(trace=True)
        print("trace shapes done")
        return
    rows, version = run()
    lines = ["# r10: zstd content checksums (CRYO_OPT_ZSTD_CHECKSUM) off vs on, level %d, %s" % (LEVEL, version),
             "# device shapes: HIP-event ms (bulk median of 3, K=8 median of 30); host-buffer read: wall ms, median of 50",
             "%-38s %10s %10s %9s %10s %10s" % ("shape", "off_ms", "on_ms", "delta", "off_GB/s", "on_GB/s")]
    for shape, a, b, gb in rows:
        lines.append("%-38s %10.3f %10.3f %+8.1f%% %10.1f %10.1f" % (shape, a, b, 100.0 * (b - a) / a, gb / a * 1e3, gb / b * 1e3))
    txt = "\n".join(lines) + "\n"
    print(txt)
    out = [a for a in argv if not a.startswith("--")]
    with open(out[0] if out else "r10_zstd_checksum.txt", "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main(sys.argv[1:])
