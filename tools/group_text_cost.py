#!/usr/bin/env python3
"""Cost of grouping a scan by a text column through host buffers (cryo_codec_group_blocks with CRYO_GROUP_TEXT) against the
integer grouping and against what a caller did before it, on one MI355X.

  Shape: built here with numpy as tools/bucket_cost.py builds its blocks: one narrow row type (g int4, country text, x int8;
  40 bytes a tuple), 290 rows per 1 MiB block, 1 024 blocks; g drawn from 16 values and country the two-letter code of g under
  a 1-byte varlena header, so both columns have the same 16 groups and the codes ascend with g; x uniform in +-2^40; LZ4 streams
  of the GPU encoder (acceleration 1).  No key: every row matches, 290 matches a block -- the most the rank pass can meet.  The
  query: GROUP BY the column with count(*) and count / sum / min / max of x.
    TEXT     cryo_codec_group_blocks by country under CRYO_GROUP_TEXT: a key cell beside the aggregate cell
  Yardsticks, on the same streams:
    (a) filter + numpy   cryo_codec_filter_blocks, then the deform of the returned tuples and the GROUP BY country in numpy: the
                         only route before
    (b) group, int       cryo_codec_group_blocks by g: the same groups without a byte of text -- the floor
  One warm-up call of each, then per round: (a), (b), TEXT, (b) again, (a) again -- the two series of each yardstick give its own
  spread (a call's place in the round moves it); wall ms around the synchronous calls, median / min / max of the rounds; d2h
  bytes from the handle's transfer counters.  At the warm-up TEXT must return (b)'s rows, n_rows and aggregate cells byte for
  byte, every key cell must hold the code of (b)'s key, and the groups merged across blocks must be (a)'s.

usage: python tools/group_text_cost.py [--rounds N] > profiles/group_text_host_calls.txt"""
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
ATTS = [(4, 4), (-1, 4), (8, 8)]
G, T, X = (1, cc.KEY_INT4), (2, cc.KEY_BYTES), (3, cc.KEY_INT8)
TUPLE = np.dtype([("hdr", "u1", (24,)), ("g", "<i4"), ("vl", "u1"), ("code", "u1", (2,)), ("pad", "u1"), ("x", "<i8")])   # 40 bytes
CODES = np.array([list(c) for c in sorted([b"at", b"be", b"ch", b"de", b"es", b"fr", b"gb", b"it", b"jp", b"kr", b"nl", b"pl", b"pt",
                                           b"se", b"tr", b"us"])], np.uint8)


def raw_blocks(cnt, rng):
    """cnt blocks as one uint8 array: header {lower, upper}, 290 items {off, len}, the tuples at the block's end"""
    out = np.zeros((cnt, B), np.uint8)
    upper = B - ROWS * TUPLE.itemsize
    hdr = np.zeros(24, np.uint8)
    hdr[18:20] = np.frombuffer(np.uint16(3).tobytes(), np.uint8)          # t_infomask2: three attributes
    hdr[20:22] = np.frombuffer(np.uint16(0x0802).tobytes(), np.uint8)     # t_infomask: HEAP_XMAX_INVALID | HEAP_HASVARWIDTH
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
        t["g"] = rng.integers(0, 16, ROWS)
        t["vl"] = (3 << 1) | 1                                            # a 1-byte header: three bytes with it
        t["code"] = CODES[t["g"]]
        t["x"] = rng.integers(-(1 << 40), 1 << 40, ROWS)
    return out.reshape(-1)


def make_streams(c):
    """the N blocks LZ4-compressed (acceleration 1) on the device, 128 at a time; list of uint8 arrays"""
    rng = np.random.default_rng(2024)
    cap = cc.bound(METHOD_LZ4, B)
    step = 128
    d_raw, d_dst, d_sz, d_st = c.alloc(step * B), c.alloc(step * cap), c.alloc(4 * step), c.alloc(4 * step)
    out = []
    for _ in range(0, N, step):
        d_raw.upload(raw_blocks(step, rng))
        c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, step, d_dst, cap, d_sz, d_st)
        c.sync()
        assert (d_st.download(dtype=np.int32) == 0).all()
        sz = d_sz.download(dtype=np.uint32)
        raw = d_dst.download()
        out += [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(step)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out


def group_by(k, x):
    """GROUP BY k in numpy: (k, count(*), sum, min, max of x), ascending"""
    order = np.argsort(k, kind="stable")
    k, x = k[order], x[order]
    first = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    return (k[first], np.diff(np.concatenate((first, [k.size]))), np.add.reduceat(x, first), np.minimum.reduceat(x, first),
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
        fdesc, adesc = cc.filter_desc(ATTS, []), cc.agg_desc([X])
        result = {}

        def filter_numpy():
            assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), dst.ctypes.data, dst.nbytes,
                                              rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
            t = dst[:int(tot[0])].view(TUPLE)                           # no bad item, every tuple 40 bytes: packed back to back
            code = t["code"].astype(np.uint16)
            result["a"] = group_by(code[:, 0] << 8 | code[:, 1], t["x"])    # the code as a big-endian number: memcmp's order

        def make_group(name, gdesc, cpg):
            rows, recs = np.zeros(N, cc.GROUP_BLOCK), np.zeros(N * ROWS, cc.GROUP_REC)
            cells, total = np.zeros((N * ROWS, cpg, 40), np.uint8), C.c_uint64()

            def run():
                assert L.cryo_codec_group_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), C.byref(gdesc[0]), C.byref(adesc[0]),
                                                 rows.ctypes.data, recs.ctypes.data, recs.shape[0], cells.ctypes.data, C.byref(total)) == 0
                result[name] = (rows, recs[:total.value], cells[:total.value])
            return run

        by_int = make_group("b", cc.group_desc([G]), 1)
        by_text = make_group("t", cc.group_desc([T], text=True), 2)
        series = [("(a) filter_blocks + numpy deform and GROUP BY", filter_numpy), ("(b) group_blocks by the int4 column", by_int),
                  ("group_blocks by the text column, CRYO_GROUP_TEXT", by_text), ("(b) group_blocks by the int4 column (again)", by_int),
                  ("(a) filter_blocks + numpy deform and GROUP BY (again)", filter_numpy)]
        for _, fn in series[:3]:                                          # warm-up, and what every case must have found
            fn()
        rows, recs, cells = result["b"]
        trows, trecs, tcells = result["t"]
        assert (rows["status"] == 0).all() and int(rows["n_bad"].sum()) == 0 and int(rows["n_match"].sum()) == N * ROWS
        assert rows.tobytes() == trows.tobytes() and recs["n_rows"].tobytes() == trecs["n_rows"].tobytes()
        assert cells[:, 0].tobytes() == tcells[:, 0].tobytes()            # the aggregate cell of every group
        key = np.ascontiguousarray(tcells[:, 1]).view(cc.GROUP_KEY)[:, 0]
        assert (key["len"] == 2).all() and (trecs["key"][:, 0] == 2).all() and not key["bytes"][:, 2:].any() and not key["rsv"].any()
        assert np.array_equal(key["bytes"][:, :2], CODES[recs["key"][:, 0]])
        agg = np.ascontiguousarray(tcells[:, 0]).view(cc.AGG_CELL)[:, 0]
        code = key["bytes"][:, :2].astype(np.uint16)
        k = code[:, 0] << 8 | code[:, 1]
        order = np.argsort(k, kind="stable")
        first = np.flatnonzero(np.concatenate(([True], k[order][1:] != k[order][:-1])))
        merged = (k[order][first], np.add.reduceat(trecs["n_rows"][order].astype(np.int64), first),
                  np.add.reduceat(agg["sum_lo"][order].view(np.int64), first), np.minimum.reduceat(agg["min"][order], first),
                  np.maximum.reduceat(agg["max"][order], first))
        assert all(np.array_equal(x, y) for x, y in zip(merged, result["a"]))
        times, d2h = {k: [] for k, _ in series}, {}
        for _ in range(ROUNDS):
            for nm, fn in series:
                t0 = c.transfer_counters()["d2h_bytes"]
                w = time.perf_counter()
                fn()
                times[nm].append((time.perf_counter() - w) * 1e3)
                d2h[nm] = c.transfer_counters()["d2h_bytes"] - t0
        print("%-54s %10s %10s %10s %14s" % ("call (1 024 x 1 MiB, 290 x 40 B, LZ4, host buffers)", "median ms", "min ms", "max ms", "d2h bytes"))
        base = stats(times[series[0][0]])[0]
        for nm, _ in series:
            med = stats(times[nm])
            print("%-54s %10.2f %10.2f %10.2f %14d   %.2fx" % ((nm,) + med + (d2h[nm], base / med[0])), flush=True)
        b1, b2 = stats(times[series[1][0]])[0], stats(times[series[3][0]])[0]
        print("%d rounds; %d groups in the call, %d per block on average, %d in the relation; %d matches a block; compressed in %d bytes, "
              "decoded %d bytes; last column: median of (a), first series, over the call's median" %
              (ROUNDS, trecs.size, trecs.size // N, merged[0].size, ROWS, sum(a.nbytes for a in comps), N * B))
        print("(b)'s two series differ by %.3f ms; TEXT lies %+.3f ms from the mean of (b)'s two medians, at %d matches a block" %
              (abs(b1 - b2), stats(times[series[2][0]])[0] - (b1 + b2) / 2, ROWS))


main()
