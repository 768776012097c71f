#!/usr/bin/env python3
"""Every kernel route of the grouped scan under a kernel trace, on one MI355X: the cost tools (tools/group_cost.py, bucket_cost.py,
group_text_cost.py) reach k_group_block<false>, k_groupb_block<false> and k_groupt_block<false> alone.

  Shape: built here with numpy as tools/group_text_cost.py builds its blocks: 256 x 1 MiB blocks of 290 rows (g int4, f float4 = 1,
  x int8, t text = "kk"; 48 bytes a tuple), g with 1, 16 or 290 distinct values a block (--card); LZ4 streams of the GPU encoder.
  Every row matches; count / sum / min / max of four integer columns (x, g, x, g).
  Routes, 10 calls of cryo_codec_group_blocks each, the first checked against the plain call's rows, records and cells:
    plain (k_group_block<false>), a truth table (<true>), a float4 key every row passes (k_groupf_block), CRYO_GROUP_BUCKETS with
    CRYO_BUCKET_NONE (k_groupb_block<false>) and with the float key (<true>), CRYO_GROUP_TEXT with t as second group column
    (k_groupt_block<false>) and with the float key (<true>)

usage: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/group_routes_prof.py --card 1|16|290
       (a run of its own, no counters alongside; the k_group* rows of DIR's kernel_stats.csv; CRYO_CODEC_LIB names another library)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

CARD = int(sys.argv[sys.argv.index("--card") + 1])
CALLS = 10
N, B, ROWS = 256, 1 << 20, 290
ATTS = [(4, 4), (4, 4), (8, 8), (-1, 4)]
G, F, X, T = (1, cc.KEY_INT4), (2, cc.KEY_FLOAT4), (3, cc.KEY_INT8), (4, cc.KEY_BYTES)
TUPLE = np.dtype([("hdr", "u1", (24,)), ("g", "<i4"), ("f", "<f4"), ("x", "<i8"), ("vl", "u1"), ("code", "u1", (2,)), ("pad", "u1", (5,))])
assert TUPLE.itemsize == 48
EVERY = (1, cc.KEY_INT4, cc.OP_GE, -(1 << 31))
FLOAT = (2, cc.KEY_FLOAT4, cc.OP_GE, 0.0)
NONE = [(cc.BUCKET_NONE, 0, 0, 0)]
COLS = [X, G, X, G]


def raw_blocks(cnt, rng):
    out = np.zeros((cnt, B), np.uint8)
    upper = B - ROWS * TUPLE.itemsize
    hdr = np.zeros(24, np.uint8)
    hdr[18:20] = np.frombuffer(np.uint16(4).tobytes(), np.uint8)
    hdr[20:22] = np.frombuffer(np.uint16(0x0802).tobytes(), np.uint8)
    hdr[22] = 24
    items = np.zeros((ROWS, 2), "<u4")
    items[:, 0] = upper + TUPLE.itemsize * np.arange(ROWS)
    items[:, 1] = 43
    for i in range(cnt):
        blk = out[i]
        blk[:8].view("<u4")[:] = (8 + 8 * ROWS, upper)
        blk[8:8 + 8 * ROWS] = items.view(np.uint8).reshape(-1)
        t = blk[upper:].view(TUPLE)
        t["hdr"] = hdr
        t["g"] = rng.permutation(ROWS) if CARD == ROWS else rng.integers(0, CARD, ROWS)
        t["f"] = 1.0
        t["vl"] = (3 << 1) | 1
        t["code"] = (107, 107)
        t["x"] = rng.integers(-(1 << 40), 1 << 40, ROWS)
    return out.reshape(-1)


def main():
    with Codec(0) as c:
        rng = np.random.default_rng(7)
        cap = cc.bound(METHOD_LZ4, B)
        step = 128
        d_raw, d_dst, d_sz, d_st = c.alloc(step * B), c.alloc(step * cap), c.alloc(4 * step), c.alloc(4 * step)
        comps = []
        for _ in range(0, N, step):
            d_raw.upload(raw_blocks(step, rng))
            c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, step, d_dst, cap, d_sz, d_st)
            c.sync()
            assert (d_st.download(dtype=np.int32) == 0).all()
            sz = d_sz.download(dtype=np.uint32)
            raw = d_dst.download()
            comps += [raw[i * cap:i * cap + int(sz[i])].copy() for i in range(step)]
        for b in (d_raw, d_dst, d_sz, d_st):
            b.free()

        def call(keys, by, truth=None, buckets=None, text=False):
            return c.group_blocks(METHOD_LZ4, comps, B, cc.filter_desc(ATTS, keys, 0, truth), cc.group_desc(by, buckets, text), cc.agg_desc(COLS))

        routes = [("plain", lambda: call([], [G])), ("truth", lambda: call([EVERY], [G], truth=cc.truth_dnf([1], 1))),
                  ("float", lambda: call([FLOAT], [G])), ("buckets", lambda: call([], [G], buckets=NONE)),
                  ("buckets, float", lambda: call([FLOAT], [G], buckets=NONE)), ("text", lambda: call([], [G, T], text=True)),
                  ("text, float", lambda: call([FLOAT], [G, T], text=True))]
        plain = routes[0][1]()
        assert int(plain[0]["n_match"].sum()) == N * ROWS and plain[3] == (N * ROWS if CARD == ROWS else plain[3])
        for name, fn in routes:
            got = fn()
            assert got[3] == plain[3] and got[0].tobytes() == plain[0].tobytes() and got[2].tobytes() == plain[2].tobytes(), name
            assert np.array_equal(got[1]["key"][:, 0], plain[1]["key"][:, 0]) and np.array_equal(got[1]["n_rows"], plain[1]["n_rows"]), name
            for _ in range(CALLS - 1):
                fn()
        print("card %d: %d groups; every route returned the plain call's records and cells" % (CARD, plain[3]), flush=True)


main()
