#!/usr/bin/env python3
"""Cost of the ordered scan through host buffers (cryo_codec_topn_blocks) against the only route the query had before it:
cryo_codec_project_blocks on the same streams plus a sort and cut per block on the host, on one MI355X.

  Shape: built here with numpy as tools/bucket_cost.py builds its blocks: one fixed-width row type (ts int8, app int4, id int4,
  revenue int8: 48-byte tuples), 290 rows per 1 MiB block, 1 024 blocks; ts is drawn per row from the block's own hour, so a
  block's rows are in no order and blocks overlap in no key; LZ4 streams of the GPU encoder (acceleration 1).  The keys are a
  range on ts that every row passes: 290 matches per block, the case the projection brings back whole.  The query:
  SELECT id, ts, revenue ... ORDER BY ts DESC LIMIT n, rows of 24 bytes.
  The calls, on these streams:
    topn_blocks, limit 1 / 10 / 100 / 290     32 bytes per block and 24 + 24 bytes per kept row come back
  Yardsticks, on the same streams and keys:
    (a) project + numpy   cryo_codec_project_blocks, then per block a stable argsort of the returned ts and a gather of the first
                          n rows, vectorised over all blocks at once: the only route before, and the cheapest a host can do
                          (a sort per block as each arrives costs more; the comparison is biased towards this route)
    (b) project, bare     the same call without the host's work: against limit 290 it shows what the rank pass and the wider
                          records cost
  One warm-up call of each, then per round: (a) at limit 10, the four limits, (b), (a) again -- the two series of (a) give its
  own spread (a call's place in the round moves it); wall ms around the synchronous calls, median / min / max of the rounds; d2h
  bytes from the handle's transfer counters.  At the warm-up every limit's rows must be (a)'s rows for that limit, byte for byte.

usage: python tools/topn_cost.py [--rounds N] > profiles/topn_host_calls.txt"""
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
HOUR = 3_600_000_000
ATTS = [(8, 8), (4, 4), (4, 4), (8, 8)]
TUPLE = np.dtype([("hdr", "u1", (24,)), ("ts", "<i8"), ("app", "<i4"), ("id", "<i4"), ("revenue", "<i8")])   # 48 bytes
ROW = np.dtype([("id", "<i4"), ("pad", "<i4"), ("ts", "<i8"), ("revenue", "<i8")])                           # the projected row
COLS = [3, 1, 4]
KEYS = [(1, cc.KEY_INT8, cc.OP_GE, 0), (1, cc.KEY_INT8, cc.OP_LT, N * HOUR)]
LIMITS = [1, 10, 100, 290]


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
        t["ts"] = (k0 + i) * HOUR + rng.integers(0, HOUR, ROWS)
        t["app"] = rng.integers(0, 20, ROWS)
        t["id"] = (k0 + i) * ROWS + np.arange(ROWS)
        t["revenue"] = rng.integers(0, 1 << 30, ROWS)
    return out.reshape(-1)


def make_streams(c):
    """the N blocks LZ4-compressed (acceleration 1) on the device, 128 at a time; list of uint8 arrays"""
    rng = np.random.default_rng(2100)
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


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    L = cc.lib()
    with Codec(0) as c:
        comps = make_streams(c)
        src = (C.c_void_p * N)(*[a.ctypes.data for a in comps])
        szs = (C.c_uint32 * N)(*[a.nbytes for a in comps])
        _, rb = cc.project_row_layout(ATTS, COLS)
        assert rb == ROW.itemsize
        fdesc, pdesc = cc.filter_desc(ATTS, KEYS), cc.project_desc(COLS)
        prow, prec = np.zeros((N * ROWS, rb), np.uint8), np.zeros(N * ROWS, cc.PROJECT_REC)
        ptable, ptot = np.zeros(N, cc.PROJECT_BLOCK), (C.c_uint64 * 2)()
        trow, trec = np.zeros((N * ROWS, rb), np.uint8), np.zeros(N * ROWS, cc.TOPN_REC)
        ttable, ttot = np.zeros(N, cc.TOPN_BLOCK), C.c_uint64()
        odesc = {n: cc.order_desc([(1, cc.KEY_INT8, cc.ORDER_DESC)], n) for n in LIMITS}
        result = {}

        def project():
            assert L.cryo_codec_project_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), C.byref(pdesc[0]), prow.ctypes.data,
                                               prow.shape[0], prec.ctypes.data, prec.size, ptable.ctypes.data, ptot) == 0
            result["project"] = int(ptot[0])

        def project_numpy(n):
            project()
            rows = prow.view(ROW).reshape(N, ROWS)                       # every block has its 290 rows: no bad item, every row passes
            order = np.argsort(-rows["ts"], axis=1, kind="stable")[:, :n]
            result["a", n] = np.take_along_axis(rows, order, axis=1).reshape(-1)

        def topn(n):
            assert L.cryo_codec_topn_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), C.byref(odesc[n][0]), C.byref(pdesc[0]),
                                            trow.ctypes.data, trec.ctypes.data, trec.size, ttable.ctypes.data, C.byref(ttot)) == 0
            result["topn", n] = int(ttot.value)

        # the warm-up, and the calls held against each other
        for n in LIMITS:
            project_numpy(n)
            topn(n)
            assert result["project"] == N * ROWS and (ptable["n_bad"] == 0).all() and (ptable["status"] == 0).all()
            assert result["topn", n] == N * n and (ttable["n_rows"] == n).all() and (ttable["n_match"] == ROWS).all()
            assert np.array_equal(trow[:N * n].view(ROW).reshape(-1), result["a", n]), n
            assert np.array_equal(trec["key"][:N * n, 0], result["a", n]["ts"])
        series = [("(a) project_blocks + numpy sort and cut, limit 10", lambda: project_numpy(10))]
        series += [("topn_blocks, limit %d" % n, (lambda n=n: topn(n))) for n in LIMITS]
        series += [("(b) project_blocks, bare", project), ("(a) project_blocks + numpy sort and cut, limit 10 (again)", lambda: project_numpy(10))]
        times, back = {k: [] for k, _ in series}, {}
        for _ in range(ROUNDS):
            for name, fn in series:
                t0 = c.transfer_counters()["d2h_bytes"]
                w = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - w) * 1e3)
                back[name] = c.transfer_counters()["d2h_bytes"] - t0
        print("%-62s %10s %10s %10s %14s" % ("call (1 024 x 1 MiB, 290 x 48 B, LZ4, host buffers)", "median ms", "min ms", "max ms", "d2h bytes"))
        base = stats(times[series[0][0]])[0]
        for name, _ in series:
            med = stats(times[name])
            print("%-62s %10.2f %10.2f %10.2f %14d   %.2fx" % ((name,) + med + (back[name], base / med[0])), flush=True)
        a1, a2 = stats(times[series[0][0]])[0], stats(times[series[-1][0]])[0]
        bare, full = stats(times["(b) project_blocks, bare"])[0], stats(times["topn_blocks, limit 290"])[0]
        print("%d rounds; %d rows in the relation, 290 matches per block; compressed in %d bytes, decoded %d bytes; last column: median of (a), "
              "first series, over the call's median" % (ROUNDS, N * ROWS, sum(a.nbytes for a in comps), N * B))
        print("(a)'s two series differ by %.3f ms; topn_blocks at limit 290 lies %+.3f ms from the bare project_blocks" % (abs(a1 - a2), full - bare))


main()
