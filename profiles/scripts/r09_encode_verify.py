"""Cost of write verification (CRYO_OPT_ENCODE_VERIFY): compress time with verification off and on.

  K = 1 x 1 MiB `wide` / `narrow` through cryo_codec_compress_block (host buffers: PCIe both ways included), median of 30
  65 536 x 128 KiB `wide` through cryo_codec_compress_batch (device-resident), HIP events, median of 3
for LZ4 (acceleration 1) and zstd level 1, on the byte-identical encoders and in segment mode (S = 16 KiB); and what a later
read of those 1 MiB blocks costs: cryo_codec_decompress_block of the stream each mode wrote, median of 30.

usage: python profiles/scripts/r09_encode_verify.py OUT.txt"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, METHOD_ZSTD, codec as cc  # noqa: E402

METHODS = [("lz4-1", METHOD_LZ4, 1), ("zstd-1", METHOD_ZSTD, 1)]
MODES = [("identical", 0), ("segment16k", 16384)]


def one_block(c, method, param, block, reps=30, warm=5):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        c.compress_block(method, param, block)
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def read_block(c, method, comp, B, reps=30, warm=5):
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        out = c.decompress_block(method, comp, B)
        if r >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    assert out is not None
    return statistics.median(ts)


def bulk(c, method, param, d_src, d_dst, d_sz, d_st, n, B, reps=3):
    cap = cc.bound(method, B)
    c.compress_batch(method, param, d_src, B, B, n, d_dst, cap, d_sz, d_st)  # warm-up (workspace)
    c.sync()
    ts = []
    for _ in range(reps):
        c.timer_start()
        c.compress_batch(method, param, d_src, B, B, n, d_dst, cap, d_sz, d_st)
        ts.append(c.timer_stop())
    st = d_st.download(dtype=np.int32)
    assert (st == 0).all(), "statuses"
    return statistics.median(ts)


def main(out_path):
    lines = ["# r09: write verification (CRYO_OPT_ENCODE_VERIFY) off vs on, %s" % cc.version(),
             "# K=1: cryo_codec_compress_block, 1 MiB, host buffers (H2D + encode [+ verify] + D2H), wall ms, median of 30",
             "# bulk: cryo_codec_compress_batch, 65536 x 128 KiB `wide`, device-resident, HIP-event ms, median of 3",
             "%-8s %-11s %-28s %10s %10s %9s" % ("method", "mode", "shape", "off_ms", "on_ms", "overhead")]
    with Codec(0) as c:
        B1 = 1 << 20
        d = c.alloc(B1)
        blocks = {}
        for dist in (cc.DIST_WIDE, cc.DIST_NARROW):
            c.synth_batch(0, 7, 1, B1, dist, d)
            c.sync()
            blocks[cc.DIST_NAMES[dist]] = d.download().copy()
        d.free()
        rows, reads = [], []
        for mname, method, param in METHODS:
            for mode, S in MODES:
                c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
                for dname, blk in blocks.items():
                    t = []
                    for v in (0, 1):
                        c.set_option(cc.OPT_ENCODE_VERIFY, v)
                        t.append(one_block(c, method, param, blk))
                    rows.append((mname, mode, "K=1 x 1MiB %s" % dname, t[0], t[1]))
                    c.set_option(cc.OPT_ENCODE_VERIFY, 0)
                    comp = c.compress_block(method, param, blk)
                    reads.append((mname, mode, "read 1MiB %s (%d B)" % (dname, len(comp)), read_block(c, method, comp, B1)))
        c.set_option(cc.OPT_ENCODE_VERIFY, 0)
        n, B = 65536, 131072
        d_src = c.alloc(n * B)
        c.synth_batch(0, 0, n, B, cc.DIST_WIDE, d_src)
        for mname, method, param in METHODS:
            cap = cc.bound(method, B)
            d_dst, d_sz, d_st = c.alloc(n * cap), c.alloc(4 * n), c.alloc(4 * n)
            for mode, S in MODES:
                c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
                t = []
                for v in (0, 1):
                    c.set_option(cc.OPT_ENCODE_VERIFY, v)
                    t.append(bulk(c, method, param, d_src, d_dst, d_sz, d_st, n, B))
                rows.append((mname, mode, "65536 x 128KiB wide (device)", t[0], t[1]))
            for x in (d_dst, d_sz, d_st):
                x.free()
            c.set_option(cc.OPT_ENCODE_VERIFY, 0)
        d_src.free()
        c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
    for mname, mode, shape, a, b in rows:
        lines.append("%-8s %-11s %-28s %10.3f %10.3f %8.1f%%" % (mname, mode, shape, a, b, 100.0 * (b - a) / a))
    lines.append("# a later read of the same 1 MiB blocks: cryo_codec_decompress_block (H2D + decode + D2H), wall ms, median of 30")
    lines.append("%-8s %-11s %-28s %10s" % ("method", "mode", "shape", "read_ms"))
    for mname, mode, shape, t in reads:
        lines.append("%-8s %-11s %-28s %10.3f" % (mname, mode, shape, t))
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(out_path, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "r09_encode_verify.txt")
