#!/usr/bin/env python3
"""Cost of recompression through host buffers (cryo_codec_recode_blocks) against the only alternative without it:
cryo_codec_decompress_blocks followed by cryo_codec_compress_blocks, on one MI355X.

  4 096 x 128 KiB and 1 024 x 1 MiB blocks of `wide` and `narrow`, LZ4 acceleration 1 (streams of the GPU encoder) to zstd
  level 1 and level 9; one warm-up call of each path, then the two paths alternating, wall ms around the synchronous calls,
  median / min / max of 20 (level 9: of 5); h2d / d2h bytes from the handle's transfer counters (cryo_codec_compress_blocks
  does not count its transfers: n x B up and n bound-sized slots back are added from its code).  Sizes and a sample of the
  streams of the two paths are compared after every row.

usage: python tools/recode_cost.py > OUT.txt
       python tools/recode_cost.py --prof    (4 096 x 128 KiB `wide`, LZ4 to zstd-1, recode_blocks only, three calls: run under
                                              rocprofv3 --kernel-trace --stats for k_recode_pack against the encode kernels)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, METHOD_ZSTD, codec as cc  # noqa: E402

PROF = "--prof" in sys.argv
DIST = {"wide": cc.DIST_WIDE, "narrow": cc.DIST_NARROW}


def make_streams(c, n, B, dist):
    """n synthetic blocks LZ4-compressed (acceleration 1) on the device; list of uint8 arrays"""
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


def main():
    L = cc.lib()
    shapes = [(4096, 131072), (1024, 1 << 20)] if not PROF else [(4096, 131072)]
    targets = [1, 9] if not PROF else [1]
    reps = 20 if not PROF else 2
    reps9 = 5
    print("%-7s %5s x %-8s %-8s %-22s %10s %10s %10s %14s %14s" % ("dist", "n", "B", "target", "path", "median ms", "min ms", "max ms",
                                                                   "h2d bytes", "d2h bytes"))
    with Codec(0) as c:
        for n, B in shapes:
            for dname in (("wide", "narrow") if not PROF else ("wide",)):
                comps = make_streams(c, n, B, DIST[dname])
                src = (C.c_void_p * n)(*[a.ctypes.data for a in comps])
                szs = (C.c_uint32 * n)(*[a.nbytes for a in comps])
                cap = cc.bound(METHOD_ZSTD, B)
                slot = (cap + 15) & ~15
                raw = np.zeros(n * B, np.uint8)
                st = np.zeros(n, np.int32)
                out2 = np.zeros(n * cap, np.uint8)
                osz2 = np.zeros(n, np.uint32)
                packed = np.zeros(n * slot, np.uint8)
                off, osz, st3 = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.int32)
                for level in targets:
                    def two_calls():
                        assert L.cryo_codec_decompress_blocks(c.h, METHOD_LZ4, src, szs, n, raw.ctypes.data, B, st.ctypes.data) == 0
                        assert L.cryo_codec_compress_blocks(c.h, METHOD_ZSTD, level, raw.ctypes.data, B, n, out2.ctypes.data, cap,
                                                            osz2.ctypes.data) == 0

                    def recode():
                        assert L.cryo_codec_recode_blocks(c.h, METHOD_LZ4, src, szs, n, B, METHOD_ZSTD, level, packed.ctypes.data,
                                                          packed.nbytes, off.ctypes.data, osz.ctypes.data, st3.ctypes.data) == 0

                    paths = (("decompress+compress", two_calls), ("recode_blocks", recode)) if not PROF else (("recode_blocks", recode),)
                    times = {name: [] for name, _ in paths}
                    xfer = {}
                    for name, fn in paths:      # warm-up: buffers, code objects, first touches of the host arrays
                        fn()
                    for r in range(reps if level == 1 else reps9):       # alternating
                        for name, fn in paths:
                            t0 = c.transfer_counters()
                            w = time.perf_counter()
                            fn()
                            times[name].append((time.perf_counter() - w) * 1e3)
                            t1 = c.transfer_counters()
                            xfer[name] = (t1["h2d_bytes"] - t0["h2d_bytes"], t1["d2h_bytes"] - t0["d2h_bytes"])
                    if not PROF:
                        assert (st == 0).all() and (st3 == 0).all() and np.array_equal(osz, osz2)
                        for i in range(0, n, max(1, n // 64)):
                            assert np.array_equal(packed[int(off[i]):int(off[i]) + int(osz[i])], out2[i * cap:i * cap + int(osz2[i])])
                    for name, _ in paths:
                        t = sorted(times[name])
                        # the two-call sequence's compress does not count its transfers: n * B up, (n - 1) * stride + bound back
                        h2d, d2h = xfer[name]
                        if name != "recode_blocks":
                            h2d += n * B
                            d2h += (n - 1) * cap + cap
                        print("%-7s %5d x %-8d zstd-%-3d %-22s %10.1f %10.1f %10.1f %14d %14d" % (dname, n, B, level, name, t[len(t) // 2],
                                                                                                 t[0], t[-1], h2d, d2h), flush=True)
                    print("        compressed: in %d bytes, out %d bytes, raw %d bytes" % (sum(a.nbytes for a in comps), int(osz.sum()), n * B),
                          flush=True)


main()
