#!/usr/bin/env python3
"""Cost of the grouped scan through host buffers (cryo_codec_group_blocks) against what a caller does without it, on one MI355X.

  Shape: the generator has no low-cardinality column, so the blocks are built here with numpy: one fixed-width row type (ts int8,
  g int4, x int8), 290 rows per 1 MiB block, 1 024 blocks, ts ascending through the relation, g drawn from 1, 16 and 290 distinct
  values per block, x uniform in +-2^40; LZ4 streams of the GPU encoder (acceleration 1).  The keys are a range on ts that every
  row passes (100 % selectivity).
  Yardsticks, the calls a caller has without the grouping, on the same streams and keys:
    (a) filter + numpy   cryo_codec_filter_blocks, then GROUP BY g of the returned tuples in numpy (np.unique + reduceat): count(*)
                         and count / sum / min / max of x per group -- what a caller does today
    (b) agg_blocks       cryo_codec_agg_blocks with the same aggregate columns: the floor -- the same decode and one sweep, no
                         grouping
  Against them group_blocks with one aggregate column and with four (x four times), alone and followed by the merge of the
  per-block groups across blocks in numpy, which a caller of group_blocks still has to do.
  One warm-up call of each, then per round: (a) with 1 and 4 columns, (b) with 1 and 4, every group case, (b) again, (a) again --
  the two series of each yardstick give its own spread (a call's place in the round moves it); wall ms around the synchronous
  calls, median / min / max of the rounds; d2h bytes from the handle's transfer counters.  Every case's merged groups are compared
  with the numpy GROUP BY first.

usage: python tools/group_cost.py [--rounds N] > OUT.txt
       python tools/group_cost.py --prof    (device-resident: decompress_batch, agg_batch and group_batch with four columns at each
                                            cardinality, three calls each: run under rocprofv3 --kernel-trace --stats for
                                            k_group_block next to k_agg_block and the decode kernels of the same batch, no counters
                                            alongside)"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

PROF = "--prof" in sys.argv
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
N, B, ROWS = 1024, 1 << 20, 290
ATTS = [(8, 8), (4, 4), (8, 8)]
BY = [(2, cc.KEY_INT4)]
COL = (3, cc.KEY_INT8)
CARDS = (1, 16, 290)
TUPLE = np.dtype([("hdr", "u1", (24,)), ("ts", "<i8"), ("g", "<i4"), ("pad", "<i4"), ("x", "<i8")])   # t_hoff = 24; 48 bytes
KEYS = [(1, cc.KEY_INT8, cc.OP_GE, 0), (1, cc.KEY_INT8, cc.OP_LT, N * ROWS)]


def raw_blocks(k0, cnt, card, rng):
    """blocks k0 .. k0 + cnt - 1 as one uint8 array: header {lower, upper}, 290 items {off, len}, the tuples at the block's end"""
    out = np.zeros((cnt, B), np.uint8)
    upper = B - ROWS * TUPLE.itemsize
    hdr = np.zeros(24, np.uint8)
    hdr[18:20] = np.frombuffer(np.uint16(3).tobytes(), np.uint8)          # t_infomask2: three attributes
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
        t["ts"] = (k0 + i) * ROWS + np.arange(ROWS)
        t["g"] = rng.permutation(ROWS) if card == ROWS else rng.integers(0, card, ROWS)
        t["x"] = rng.integers(-(1 << 40), 1 << 40, ROWS)
    return out.reshape(-1)


def make_streams(c, card):
    """the N blocks of one cardinality LZ4-compressed (acceleration 1) on the device, 128 at a time; list of uint8 arrays"""
    rng = np.random.default_rng(1000 + card)
    cap = cc.bound(METHOD_LZ4, B)
    step = 128
    d_raw, d_dst, d_sz, d_st = c.alloc(step * B), c.alloc(step * cap), c.alloc(4 * step), c.alloc(4 * step)
    out = []
    for k0 in range(0, N, step):
        d_raw.upload(raw_blocks(k0, step, card, rng))
        c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, step, d_dst, cap, d_sz, d_st)
        c.sync()
        assert (d_st.download(dtype=np.int32) == 0).all()
        sz = d_sz.download(dtype=np.uint32)
        raw = d_dst.download()
        out += [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(step)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out


def group_by(g, cols):
    """GROUP BY g in numpy: (keys, count(*), [(sum, min, max) per column]), keys ascending"""
    order = np.argsort(g, kind="stable")
    keys, first, counts = np.unique(g[order], return_index=True, return_counts=True)
    return keys, counts, [(np.add.reduceat(v[order], first), np.minimum.reduceat(v[order], first), np.maximum.reduceat(v[order], first))
                          for v in cols]


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def prof(c):
    for card in CARDS:
        comps = make_streams(c, card)
        sizes = np.array([a.nbytes for a in comps], np.uint32)
        offs = np.zeros(N, np.uint64)
        offs[1:] = np.cumsum((sizes[:-1].astype(np.uint64) + 15) & ~np.uint64(15))
        packed = np.zeros(int(offs[-1]) + int(sizes[-1]) + 64, np.uint8)
        for i, a in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + a.nbytes] = a
        _, a, k = cc.filter_desc(ATTS, KEYS)
        _, r = cc.group_desc(BY)
        _, g = cc.agg_desc([COL] * 4)
        cap = N * ROWS
        bufs = [c.alloc(packed.nbytes), c.alloc(8 * N), c.alloc(4 * N), c.alloc(N * B), c.alloc(4 * N), c.alloc(a.nbytes),
                c.alloc(k.nbytes), c.alloc(r.nbytes), c.alloc(g.nbytes), c.alloc(32 * N), c.alloc(24 * cap), c.alloc(160 * cap),
                c.alloc(8), c.alloc(16 * N), c.alloc(160 * N)]
        d_src, d_off, d_sz, d_dec, d_st, d_atts, d_keys, d_by, d_cols, d_rows, d_recs, d_cells, d_total, d_arows, d_acells = bufs
        for d, h in ((d_src, packed), (d_off, offs), (d_sz, sizes), (d_atts, a), (d_keys, k), (d_by, r), (d_cols, g)):
            d.upload(h)
        for _ in range(3):
            c.decompress_batch(METHOD_LZ4, d_src, d_off, d_sz, d_dec, B, B, N, d_st)
            c.agg_batch(METHOD_LZ4, d_src, d_off, d_sz, B, N, len(ATTS), d_atts, len(KEYS), d_keys, 4, d_cols, d_arows, d_acells)
            c.group_batch(METHOD_LZ4, d_src, d_off, d_sz, B, N, len(ATTS), d_atts, len(KEYS), d_keys, 1, d_by, 4, d_cols, d_rows,
                          d_recs, cap, d_cells, d_total)
            c.sync()
        rows = d_rows.download().view(cc.GROUP_BLOCK)
        print("%d x %d, %d groups per block drawn, four columns: %d matches, %d groups" %
              (N, B, card, int(rows["n_match"].sum()), int(d_total.download().view("<u8")[0])), flush=True)
        for b in bufs:
            b.free()


def main():
    L = cc.lib()
    with Codec(0) as c:
        if PROF:
            return prof(c)
        print("%4s %-36s %10s %10s %10s %14s" % ("g", "call", "median ms", "min ms", "max ms", "d2h bytes"))
        for card in CARDS:
            comps = make_streams(c, card)
            src = (C.c_void_p * N)(*[a.ctypes.data for a in comps])
            szs = (C.c_uint32 * N)(*[a.nbytes for a in comps])
            dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * ROWS, cc.FILTER_REC)
            table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
            arows, acells = np.zeros(N, cc.AGG_BLOCK), np.zeros((N, 4), cc.AGG_CELL)
            rows, recs = np.zeros(N, cc.GROUP_BLOCK), np.zeros(N * ROWS, cc.GROUP_REC)
            cells, total = np.zeros(N * ROWS * 4, cc.AGG_CELL), C.c_uint64()
            fdesc, gdesc = cc.filter_desc(ATTS, KEYS), cc.group_desc(BY)
            result = {}

            def make_filter_numpy(ncols):
                def run():
                    assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), dst.ctypes.data, dst.nbytes,
                                                      rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                    t = dst[:int(tot[0])].view(TUPLE)                   # no bad item, every tuple 48 bytes: packed back to back
                    result["a"] = group_by(t["g"], [t["x"]] * ncols)
                return run

            def make_agg(ncols):
                adesc = cc.agg_desc([COL] * ncols)

                def run():
                    assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), C.byref(adesc[0]),
                                                   arows.ctypes.data, acells.ctypes.data) == 0
                return run

            def make_group(ncols, merge):
                adesc = cc.agg_desc([COL] * ncols)

                def run():
                    assert L.cryo_codec_group_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(fdesc[0]), C.byref(gdesc[0]),
                                                     C.byref(adesc[0]), rows.ctypes.data, recs.ctypes.data, recs.size, cells.ctypes.data,
                                                     C.byref(total)) == 0
                    if not merge:
                        return
                    # the per-block groups merged across blocks: n_rows and the sums added (they fit in 64 bits here), min / max
                    r = recs[:total.value]
                    cs = cells[:total.value * ncols].reshape(total.value, ncols)
                    order = np.argsort(r["key"][:, 0], kind="stable")
                    keys, first = np.unique(r["key"][order, 0], return_index=True)
                    result["g"] = (keys, np.add.reduceat(r["n_rows"][order].astype(np.int64), first),
                                   [(np.add.reduceat(cs["sum_lo"][order, j].view(np.int64), first),
                                     np.minimum.reduceat(cs["min"][order, j], first), np.maximum.reduceat(cs["max"][order, j], first))
                                    for j in range(ncols)])
                return run

            a1, a4, b1, b4 = make_filter_numpy(1), make_filter_numpy(4), make_agg(1), make_agg(4)
            series = [("(a) filter_blocks + numpy, 1 column", a1), ("(a) filter_blocks + numpy, 4 columns", a4),
                      ("(b) agg_blocks, 1 column", b1), ("(b) agg_blocks, 4 columns", b4),
                      ("group_blocks, 1 column", make_group(1, False)), ("group_blocks + merge, 1 column", make_group(1, True)),
                      ("group_blocks, 4 columns", make_group(4, False)), ("group_blocks + merge, 4 columns", make_group(4, True)),
                      ("(b) agg_blocks, 1 column (again)", b1), ("(b) agg_blocks, 4 columns (again)", b4),
                      ("(a) filter_blocks + numpy, 1 column (again)", a1), ("(a) filter_blocks + numpy, 4 columns (again)", a4)]
            for nm, fn in series[:8]:                                    # warm-up, and what every case must have found
                fn()
                if "merge" in nm:
                    ncols = 1 if "1 column" in nm else 4
                    make_filter_numpy(ncols)()
                    (ka, na, ca), (kg, ng, cg) = result["a"], result["g"]
                    assert np.array_equal(ka, kg) and np.array_equal(na, ng), nm
                    assert all(np.array_equal(x, y) for j in range(ncols) for x, y in zip(ca[j], cg[j])), nm
                    assert (rows["status"] == 0).all() and int(rows["n_bad"].sum()) == 0 and int(rows["n_match"].sum()) == N * ROWS
            times, d2h = {k: [] for k, _ in series}, {}
            for _ in range(ROUNDS):
                for nm, fn in series:
                    t0 = c.transfer_counters()["d2h_bytes"]
                    w = time.perf_counter()
                    fn()
                    times[nm].append((time.perf_counter() - w) * 1e3)
                    d2h[nm] = c.transfer_counters()["d2h_bytes"] - t0
            for nm, _ in series:
                med = stats(times[nm])
                base = stats(times["(a) filter_blocks + numpy, %s" % ("1 column" if "1 column" in nm else "4 columns")])[0]
                print("%4d %-46s %10.2f %10.2f %10.2f %14d   %.2fx" % ((card, nm) + med + (d2h[nm], base / med[0])), flush=True)
            print("     %d distinct values of g per block drawn: %d groups per block on average, %d in the relation; compressed in %d "
                  "bytes, decoded %d bytes; last column: median of (a) with as many columns over the call's median" %
                  (card, total.value // N, len(result["g"][0]), sum(a.nbytes for a in comps), N * B), flush=True)


main()
