#!/usr/bin/env python3
"""Cost of pattern scan keys (CRYO_OP_LIKE) through host buffers on one MI355X: 1 024 x 1 MiB `narrow` (290 tuples of 61 bytes
per block: an int4 rowid and a text of 32 hex digits under a 1-byte header), LZ4 streams of the GPU encoder (acceleration 1).

  LIKE '%..%' on the text column at two selectivities -- the patterns are picked from a few candidates by what the decoded
  blocks hold: the one nearest 1 % and the one nearest 50 % of the rows -- through filter_blocks with CRYO_FILTER_COUNT_ONLY
  and through agg_blocks (count, sum, min, max of the rowid).
  The same two calls with an = key on the same column: what is left between the two is the matcher's own cost.
  The only route before: filter_blocks without a key, which ships every tuple, and the match on the host over the tuples that
  came back (in Python here, one regular expression per tuple: the call's time and the match's are printed apart).

One warm-up call of each, then two series of ROUNDS rounds; a round runs every call once, wall ms around the synchronous call;
median / min / max per series -- the two series of one call give the spread of the measurement itself.  Beside every call the
bytes that crossed PCIe in one call, both ways (cryo_codec_get_transfer_counters).  The counts of every case are compared with
what the decoded blocks hold.

usage: python tools/like_cost.py [--rounds N] > profiles/like_host_calls.txt"""
import ctypes as C
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pg_cryogen_amd import Codec, METHOD_LZ4, codec as cc  # noqa: E402

ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
ATTS = [(4, 4), (-1, 4)]
N, B = 1024, 1 << 20
CANDIDATES = [b"%abc%", b"%7f3%", b"%00%", b"%a%b%c%", b"%a%b%", b"%e_f%", b"%a%", b"%12%", b"%a%b%c%d%", b"%0%1%2%"]


def make_streams(c):
    cap = cc.bound(METHOD_LZ4, B)
    d_raw, d_dst, d_sz, d_st = c.alloc(N * B), c.alloc(N * cap), c.alloc(4 * N), c.alloc(4 * N)
    c.synth_batch(7, 0, N, B, cc.DIST_NARROW, d_raw)
    c.compress_batch(METHOD_LZ4, 1, d_raw, B, B, N, d_dst, cap, d_sz, d_st)
    c.sync()
    assert (d_st.download(dtype=np.int32) == 0).all()
    sz = d_sz.download(dtype=np.uint32)
    comp = d_dst.download()
    raw = d_raw.download()
    out = [comp[i * cap:i * cap + int(sz[i])].copy() for i in range(N)]
    for b in (d_raw, d_dst, d_sz, d_st):
        b.free()
    return out, raw


def as_regex(pattern):
    """a LIKE pattern of '%', '_' and hex digits as a regular expression over bytes"""
    return re.compile(b"".join(b".*" if ch == 0x25 else b"." if ch == 0x5F else re.escape(bytes([ch])) for ch in pattern) + b"\\Z", re.S)


def stats(t):
    t = sorted(t)
    return t[len(t) // 2], t[0], t[-1]


def main():
    L = cc.lib()
    with Codec(0) as c:
        comps, raw = make_streams(c)
        src = (C.c_void_p * N)(*[a.ctypes.data for a in comps])
        szs = (C.c_uint32 * N)(*[a.nbytes for a in comps])
        blocks = raw.reshape(N, B)
        items = blocks[:, 8:8 + 8 * 290].copy().view("<u4").reshape(N, 290, 2)
        assert (blocks[:, :4].copy().view("<u4") == 8 + 8 * 290).all() and (items[:, :, 1] == 61).all()
        base = (np.arange(N, dtype=np.int64)[:, None] * B + items[:, :, 0]).ravel()
        assert (raw[base + 28] == ((32 + 1) << 1 | 1)).all()
        text = np.stack([raw[base + 29 + k] for k in range(32)], 1)
        texts = [bytes(t) for t in text]
        rows = N * 290
        share = {p: sum(1 for t in texts if as_regex(p).match(t)) for p in CANDIDATES}
        p1 = min(CANDIDATES, key=lambda p: abs(share[p] - rows // 100))
        p50 = min(CANDIDATES, key=lambda p: abs(share[p] - rows // 2))
        one = texts[rows // 2]
        n_eq = sum(1 for t in texts if t == one)
        print("rows %d; LIKE %r matches %d (%.2f %%), LIKE %r matches %d (%.2f %%), = one row's text matches %d"
              % (rows, p1, share[p1], 100.0 * share[p1] / rows, p50, share[p50], 100.0 * share[p50] / rows, n_eq), flush=True)
        dst, rec = np.zeros(N * B, np.uint8), np.zeros(N * 290, cc.FILTER_REC)
        table, tot = np.zeros(N, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
        arows, acells = np.zeros(N, cc.AGG_BLOCK), np.zeros((N, 1), cc.AGG_CELL)
        adesc = cc.agg_desc([(1, cc.KEY_INT4)])
        host_ms, call_ms = {}, {}

        def count_call(keys, want):
            desc = cc.filter_desc(ATTS, keys, cc.FILTER_COUNT_ONLY)

            def run():
                assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), dst.ctypes.data, dst.nbytes,
                                                  rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                assert int(table["n_match"].sum()) == want and int(table["n_bad"].sum()) == 0
            return run

        def agg_call(keys, want):
            desc = cc.filter_desc(ATTS, keys)

            def run():
                assert L.cryo_codec_agg_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), C.byref(adesc[0]),
                                               arows.ctypes.data, acells.ctypes.data) == 0
                assert int(arows["n_match"].sum()) == want == int(acells["n"].sum()) and int(arows["n_bad"].sum()) == 0
            return run

        def old_route(name, pattern, want):
            """every tuple back, then the match on the host: the inner text of '%..%' searched in each tuple's 32 text bytes"""
            desc = cc.filter_desc(ATTS, [])
            rx = as_regex(pattern)

            def run():
                w = time.perf_counter()
                assert L.cryo_codec_filter_blocks(c.h, METHOD_LZ4, src, szs, N, B, C.byref(desc[0]), dst.ctypes.data, dst.nbytes,
                                                  rec.ctypes.data, rec.size, table.ctypes.data, tot) == 0
                call_ms.setdefault(name, []).append((time.perf_counter() - w) * 1e3)
                assert tot[1] == rows and tot[0] == rows * 64
                w = time.perf_counter()
                view = dst[:rows * 64].reshape(rows, 64)[:, 29:61]
                hits = sum(1 for t in view if rx.match(t.tobytes()))
                host_ms.setdefault(name, []).append((time.perf_counter() - w) * 1e3)
                assert hits == want
            return run

        like = lambda p: [(2, cc.KEY_BYTES, cc.OP_LIKE, cc.like(p, utf8=False))]  # noqa: E731
        eq = [(2, cc.KEY_BYTES, cc.OP_EQ, one)]
        series = [("count only, LIKE ~1 %", count_call(like(p1), share[p1])),
                  ("count only, LIKE ~50 %", count_call(like(p50), share[p50])),
                  ("count only, text = 32 bytes", count_call(eq, n_eq)),
                  ("agg_blocks, LIKE ~1 %", agg_call(like(p1), share[p1])),
                  ("agg_blocks, LIKE ~50 %", agg_call(like(p50), share[p50])),
                  ("agg_blocks, text = 32 bytes", agg_call(eq, n_eq)),
                  ("old route: no key, every tuple back, ~1 %", old_route("~1 %", p1, share[p1])),
                  ("old route: no key, every tuple back, ~50 %", old_route("~50 %", p50, share[p50]))]
        xfer = {}
        for name, fn in series:                                              # the warm-up, and the bytes of one call
            t0 = c.transfer_counters()
            fn()
            t1 = c.transfer_counters()
            xfer[name] = (t1["h2d_bytes"] - t0["h2d_bytes"], t1["d2h_bytes"] - t0["d2h_bytes"])
        host_ms.clear()
        call_ms.clear()
        print("%-46s %6s %10s %10s %10s %13s %13s" % ("call (1 024 x 1 MiB narrow, LZ4, host buffers)", "series", "median ms", "min ms", "max ms",
                                                     "h2d bytes", "d2h bytes"))
        for which in ("A", "B"):
            times = {k: [] for k, _ in series}
            for _ in range(ROUNDS):
                for name, fn in series:
                    w = time.perf_counter()
                    fn()
                    times[name].append((time.perf_counter() - w) * 1e3)
            for name, _ in series:
                print("%-46s %6s %10.3f %10.3f %10.3f %13d %13d" % ((name, which) + stats(times[name]) + xfer[name]), flush=True)
        for name, t in host_ms.items():
            print("old route %s: the call alone median %.3f ms (min %.3f, max %.3f); the match on the host (Python, one regular expression per "
                  "tuple) median %.3f ms" % ((name,) + stats(call_ms[name]) + (stats(t)[0],)))


main()
