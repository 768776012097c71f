#!/usr/bin/env python3
"""Cost of grouping a scan by time buckets through host buffers (cryo_codec_group_blocks with CRYO_GROUP_BUCKETS) against what a
caller does without it, on one MI355X.

  Shape: built here with numpy as tools/group_cost.py builds its blocks: one fixed-width row type (ts int8, g int4, x int8 and --
  for yardstick (b) alone -- day int8, which already stores the start of ts's day), 290 rows per 1 MiB block, 1 024 blocks; ts
  ascends through the relation in microseconds, 4 640 rows per day, so the relation spans 64 days and a block lies in one day or
  across one midnight; g drawn from 16 values; x uniform in +-2^40; LZ4 streams of the GPU encoder (acceleration 1).  The keys are
  a range on ts that every row passes.  The query: GROUP BY day of ts, g with count(*) and count / sum / min / max of x.
  The bucketed calls, on these streams:
    WIDTH    the day as a width of 86 400 000 000 from origin 0
    BOUNDS   the same days as a list of the 64 midnights (searched: more than 8 boundaries)
  Yardsticks, on the same streams and keys:
    (a) filter + numpy   cryo_codec_filter_blocks, then a floor division of ts and the GROUP BY of the returned tuples in numpy:
                         the only route without the buckets
    (b) group, stored    cryo_codec_group_blocks on the columns (day, g), no bucket: the same groups, no bucket arithmetic -- the
                         floor
  One warm-up call of each, then per round: (a), (b), WIDTH, BOUNDS, (b) again, (a) again -- the two series of each yardstick give
  its own spread (a call's place in the round moves it); wall ms around the synchronous calls, median / min / max of the rounds;
  d2h bytes from the handle's transfer counters.  At the warm-up the three group calls must return the same rows, records and
  cells byte for byte, and their groups merged across blocks must be (a)'s.

usage: python tools/bucket_cost.py [--rounds N] > profiles/bucket_host_calls.txt"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
N, B, ROWS = 1024, 1 << 20, 290
DAYS = 64
US_PER_DAY = 86_400_000_000
STEP = US_PER_DAY * DAYS // (N * ROWS)                  # microseconds between two rows
ATTS = [(8, 8), (4, 4), (8, 8), (8, 8)]
TS, G, X, DAY = (1, cc.KEY_INT8), (2, cc.KEY_INT4), (3, cc.KEY_INT8), (4, cc.KEY_INT8)
TUPLE = np.dtype([("hdr", "u1", (24,)), ("ts", "<i8"), ("g", "<i4"), ("pad", "<i4"), ("x", "<i8"), ("day", "<i8")])   # 56 bytes
KEYS = [(1, cc.KEY_INT8, cc.OP_GE, 0), (1, cc.KEY_INT8, cc.OP_LT, N * ROWS * STEP)]


def raw_blocks(k0, cnt, rng):
    """blocks k0 .. k0 + cnt - 1 as one uint8 array: header {lower, upper}, 290 items {off, len}, the tuples at the block's end"""
    out = np.zeros((cnt, B), np.uint8)
    upper = B - ROWS * TUPLE.itemsize
    hdr = np.zeros(24, np.uint8)
    hdr[18:20] = np.frombuffer(np.uint16(4).tobytes(), np.uint8)          # t_infomask2: four attributes
    hdr[20:22] = np.frombuffer(np.uint16(0x0800).tobytes(), np.uint8)     # t_infomask: HEAP_XMAX_INVALID
    hdr[22] = 24                                                          # t_hoff
    items = np.zeros((ROWS, 2), "<u4")
    items[:, 0] = upper + TUPLE.itemsize * np.arange(ROWS)
    items[:, 1] = TUPLE.itemsize
    for i in range(cnt):
        blk = out[i]
        blk[:8].view("<u4")[:] = (8 + 8 * ROWS, upper)
        blk[8:8 + 8 * ROWS] = items.view(np.uint8).reshape(-1)
        t = blk[upper:].view(TUPLE)
        t["hdr"] = hdr
        t["ts"] = ((k0 + i) * ROWS + np.arange(ROWS)) * STEP
        t["g"] = rng.integers(0, 16, ROWS)
        t["x"] = rng.integers(-(1 << 40), 1 << 40, ROWS)
        t["day"] = t["ts"] // US_PER_DAY * US_PER_DAY
    return out.reshape(-1)


def make_streams(c):
    """the N blocks LZ4-compressed (acceleration 1) on the device, 128 at a time; list of uint8 arrays"""
    rng = np.random.default_rng(2000)
    cap = cc.bound(METHOD_LZ4, B)
    step = 128
    d_raw, d_dst, d_sz, d_st = c.alloc(step * B), c.alloc(step * cap), c.alloc(4 * step), c.alloc(4 * step)
    out = []
    for k0 in range(0, N, step):
        d_raw.upload(raw_blocks(k0, step, rng))
        c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, step, d_dst, cap, d_sz, d_st)
        c.sync()
        assert (d_st.download(dtype=np.int32) == 0).all()
        sz = d_sz.download(dtype=np.uint32)
        raw = d_dst.download()
        out += [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(step)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out


def group_by(k1, k2, x):
    """GROUP BY k1, k2 in numpy: (k1, k2, count(*), sum, min, max of x), ascending"""
    order = np.lexsort((k2, k1))
    k1, k2, x = k1[order], k2[order], x[order]
    first = np.flatnonzero(np.concatenate(([True], (k1[1:] != k1[:-1]) | (k2[1:] != k2[:-1]))))
    return (k1[first], k2[first], np.diff(np.concatenate((first, [k1.size]))), np.add.reduceat(x, first), np.minimum.reduceat(x, first),
            np.maximum.reduceat(x, first))


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    L = cc.lib()
    with Codec(0) as c:
        comps = make_streams(c)
        src = (C.c_void_p * N)(*[a.ctypes.data for a in comps])
        szs = (C.c_uint32 * N)(*[a.nbytes for a in comps])
        dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * ROWS, cc.FILTER_REC)
        table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
        fdesc, adesc = cc.filter_desc(ATTS, KEYS), cc.agg_desc([X])
        result = {}

        def filter_numpy():
            assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), dst.ctypes.data, dst.nbytes,
                                              rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
            t = dst[:int(tot[0])].view(TUPLE)                           # no bad item, every tuple 56 bytes: packed back to back
            result["a"] = group_by(t["ts"] // US_PER_DAY * US_PER_DAY, t["g"], t["x"])

        def make_group(name, gdesc):
            rows, recs = np.zeros(N, cc.GROUP_BLOCK), np.zeros(N * ROWS, cc.GROUP_REC)
            cells, total = np.zeros(N * ROWS, cc.AGG_CELL), C.c_uint64()

            def run():
                assert L.cryo_codec_group_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), C.byref(gdesc[0]), C.byref(adesc[0]),
                                                 rows.ctypes.data, recs.ctypes.data, recs.size, cells.ctypes.data, C.byref(total)) == 0
                result[name] = (rows, recs[:total.value], cells[:total.value])
            return run

        stored = make_group("b", cc.group_desc([DAY, G]))
        width = make_group("w", cc.group_desc([TS, G], [(cc.BUCKET_WIDTH, 0, 0, US_PER_DAY), (cc.BUCKET_NONE, 0, 0, 0)]))
        bounds = make_group("l", cc.group_desc([TS, G], [(cc.BUCKET_BOUNDS, 0, 0, [d * US_PER_DAY for d in range(DAYS)]),
                                                         (cc.BUCKET_NONE, 0, 0, 0)]))
        series = [("(a) filter_blocks + numpy floor and GROUP BY", filter_numpy), ("(b) group_blocks on the stored day", stored),
                  ("group_blocks, WIDTH day of ts", width), ("group_blocks, BOUNDS 64 midnights", bounds),
                  ("(b) group_blocks on the stored day (again)", stored), ("(a) filter_blocks + numpy floor and GROUP BY (again)", filter_numpy)]
        for _, fn in series[:4]:                                          # warm-up, and what every case must have found
            fn()
        rows, recs, cells = result["b"]
        assert (rows["status"] == 0).all() and int(rows["n_bad"].sum()) == 0 and int(rows["n_match"].sum()) == N * ROWS
        for other in ("w", "l"):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(result["b"], result[other])), other
        order = np.lexsort((recs["key"][:, 1], recs["key"][:, 0]))
        k1, k2, cnt, sm, mn, mx = group_by(recs["key"][order, 0], recs["key"][order, 1], np.zeros(order.size, np.int64))
        first = np.flatnonzero(np.concatenate(([True], (recs["key"][order][1:] != recs["key"][order][:-1]).any(axis=1))))
        merged = (k1, k2, np.add.reduceat(recs["n_rows"][order].astype(np.int64), first),
                  np.add.reduceat(cells["sum_lo"][order].view(np.int64), first), np.minimum.reduceat(cells["min"][order], first),
                  np.maximum.reduceat(cells["max"][order], first))
        assert all(np.array_equal(x, y) for x, y in zip(merged, result["a"]))
        times, d2h = {k: [] for k, _ in series}, {}
        for _ in range(ROUNDS):
            for nm, fn in series:
                t0 = c.transfer_counters()["d2h_bytes"]
                w = time.perf_counter()
                fn()
                times[nm].append((time.perf_counter() - w) * 1e3)
                d2h[nm] = c.transfer_counters()["d2h_bytes"] - t0
        print("%-54s %10s %10s %10s %14s" % ("call (1 024 x 1 MiB, 290 x 56 B, LZ4, host buffers)", "median ms", "min ms", "max ms", "d2h bytes"))
        base = stats(times[series[0][0]])[0]
        for nm, _ in series:
            med = stats(times[nm])
            print("%-54s %10.2f %10.2f %10.2f %14d   %.2fx" % ((nm,) + med + (d2h[nm], base / med[0])), flush=True)
        b1, b2 = stats(times[series[1][0]])[0], stats(times[series[4][0]])[0]
        print("%d rounds; %d groups in the call, %d per block on average, %d in the relation; compressed in %d bytes, decoded %d bytes; "
              "last column: median of (a), first series, over the call's median" %
              (ROUNDS, recs.size, recs.size // N, k1.size, sum(a.nbytes for a in comps), N * B))
        print("(b)'s two series differ by %.3f ms; WIDTH lies %+.3f ms and BOUNDS %+.3f ms from the mean of (b)'s two medians" %
              (abs(b1 - b2), stats(times[series[2][0]])[0] - (b1 + b2) / 2, stats(times[series[3][0]])[0] - (b1 + b2) / 2))


main()
