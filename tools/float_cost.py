#!/usr/bin/env python3
"""Cost of float aggregate columns and float scan keys (CRYO_KEY_FLOAT8) through host buffers on one MI355X, on the shape of
tools/set_key_cost.py: 1 024 x 1 MiB blocks of 290 narrow tuples (int4 rowid, float8 x, int8 k; 48 bytes each), LZ4 streams of
the GPU encoder (acceleration 1).  x is a seeded mix of signs and of magnitudes over sixty binades; k is x rounded, so that the
integer column has as many distinct values.

  agg_blocks with sum(x) -- the float kernel, k_aggf_block -- without a key and with x > 0 (about half of the rows);
  agg_blocks with sum(k), the same call on an integer column -- k_agg_block;
  the route sum(float8) had before: filter_blocks without a key (every tuple comes back), then the host adds up x of the
  returned tuples (numpy over the packed bytes: one pass, plain double summation) -- the call and the reduction timed together.

One warm-up call of each, its result checked, then two series of ROUNDS rounds; a round runs every call once, wall ms around the
synchronous call; median / min / max per series -- the two series of one call give the spread of the measurement itself.  The check compares the
counts of every case with what the blocks hold and the float sum -- the blocks' cells combined with codec.cell_float_combine --
with math.fsum over the same values; it is not timed.

usage: python tools/float_cost.py [--rounds N] > OUT.txt"""
import ctypes as C
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
ATTS = [(4, 4), (8, 8), (8, 8)]
N, B, ITEMS, TLEN = 1024, 1 << 20, 290, 48


def make_blocks():
    """(blocks of shape (N, B), x of shape (N * ITEMS,), k likewise): tuple i of a block at B - 48 (i + 1), t_hoff 24, no NULL"""
    rng = np.random.default_rng(23)
    rows = N * ITEMS
    x = rng.choice((-1.0, 1.0), rows) * rng.random(rows) * 2.0 ** rng.integers(-30, 30, rows)
    k = np.rint(x).astype(np.int64)
    t = np.zeros((rows, TLEN), np.uint8)
    t[:, 18:20] = np.frombuffer(np.uint16(3).tobytes(), np.uint8)            # t_infomask2: three attributes
    t[:, 20:22] = np.frombuffer(np.uint16(0x0800).tobytes(), np.uint8)       # t_infomask: HEAP_XMAX_INVALID
    t[:, 22] = 24
    t[:, 24:28] = np.arange(rows, dtype="<i4").view(np.uint8).reshape(rows, 4)
    t[:, 32:40] = x.astype("<f8").view(np.uint8).reshape(rows, 8)
    t[:, 40:48] = k.astype("<i8").view(np.uint8).reshape(rows, 8)
    blocks = np.zeros((N, B), np.uint8)
    head = np.zeros(2 + 2 * ITEMS, "<u4")
    head[0], head[1] = 8 + 8 * ITEMS, B - TLEN * ITEMS
    head[2::2] = B - TLEN * (np.arange(ITEMS) + 1)
    head[3::2] = TLEN
    blocks[:, :head.nbytes] = head.view(np.uint8)
    blocks[:, B - TLEN * ITEMS:] = t.reshape(N, ITEMS, TLEN)[:, ::-1].reshape(N, ITEMS * TLEN)
    return blocks, x, k


def make_streams(c, blocks):
    cap = cc.bound(METHOD_LZ4, B)
    d_raw, d_dst, d_sz, d_st = c.alloc(N * B), c.alloc(N * cap), c.alloc(4 * N), c.alloc(4 * N)
    d_raw.upload(blocks.reshape(-1))
    c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, N, d_dst, cap, d_sz, d_st)
    c.sync()
    assert (d_st.download(dtype=np.int32) == 0).all()
    sz = d_sz.download(dtype=np.uint32)
    comp = d_dst.download()
    out = [comp[i * cap:i * cap + int(sz[i])].copy() for i in range(N)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    L = cc.lib()
    blocks, x, k = make_blocks()
    rows = N * ITEMS
    exact_all, exact_pos = math.fsum(x), math.fsum(x[x > 0])
    bound_all, bound_pos = 2.0 ** -90 * math.fsum(np.abs(x)), 2.0 ** -90 * math.fsum(x[x > 0])
    with Codec(0) as c:
        comps = make_streams(c, blocks)
        del blocks
        src = (C.c_void_p * N)(*[a.ctypes.data for a in comps])
        szs = (C.c_uint32 * N)(*[a.nbytes for a in comps])
        dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * ITEMS, cc.FILTER_REC)
        table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
        arows, acells = np.zeros(N, cc.AGG_BLOCK), np.zeros((N, 1), cc.AGG_CELL)

        def agg_float(keys, want, exact, bound):
            desc, adesc = cc.filter_desc(ATTS, keys), cc.agg_desc([(2, cc.KEY_FLOAT8)])

            def run():
                assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), C.byref(adesc[0]),
                                               arows.ctypes.data, acells.ctypes.data) == 0

            def check():
                total = (0, 0.0, 0.0, 0.0, 0.0)
                for i in range(N):
                    total = cc.cell_float_combine(total, cc.cell_float(acells[i, 0]))
                assert total[0] == want == int(arows["n_match"].sum()) and int(arows["n_bad"].sum()) == 0
                assert abs(total[3] - exact) <= bound + abs(exact) * 2.0 ** -52, (total, exact)    # math.fsum rounds once
            return run, check

        def agg_int():
            desc, adesc = cc.filter_desc(ATTS, []), cc.agg_desc([(3, cc.KEY_INT8)])

            def run():
                assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), C.byref(adesc[0]),
                                               arows.ctypes.data, acells.ctypes.data) == 0

            def check():
                assert sum(cc.cell_sum(acells[i, 0]) for i in range(N)) == int(k.sum()) and int(arows["n_match"].sum()) == rows
            return run, check

        def filter_and_add():
            desc = cc.filter_desc(ATTS, [])
            got = [0.0]

            def run():
                assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), dst.ctypes.data, dst.nbytes,
                                                  rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                got[0] = float(dst[:tot[0]].reshape(-1, TLEN)[:, 32:40].copy().view("<f8").sum())

            def check():
                assert tot[0] == rows * TLEN and tot[1] == rows
                assert abs(got[0] - exact_all) <= 1e-9 * bound_all * 2.0 ** 90                    # plain summation: n eps sum |x|
            return run, check

        series = [("agg_blocks, sum(float8 x), no key", agg_float([], rows, exact_all, bound_all)),
                  ("agg_blocks, sum(float8 x), x > 0", agg_float([(2, cc.KEY_FLOAT8, cc.OP_GT, 0.0)], int((x > 0).sum()), exact_pos, bound_pos)),
                  ("agg_blocks, sum(int8 k), no key", agg_int()),
                  ("filter_blocks, no key, + host sum(x)", filter_and_add())]
        for _, (fn, check) in series:                                       # the warm-up call of each, and its result checked
            fn()
            check()
        print("%-44s %6s %10s %10s %10s" % ("call (1 024 x 1 MiB, 290 x 48 B, LZ4, host buffers)", "series", "median ms", "min ms", "max ms"))
        for which in ("A", "B"):
            times = {name: [] for name, _ in series}
            for _ in range(ROUNDS):
                for name, (fn, _) in series:
                    w = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - w) * 1e3)
            for name, _ in series:
                print("%-44s %6s %10.3f %10.3f %10.3f" % ((name, which) + stats(times[name])), flush=True)


main()
