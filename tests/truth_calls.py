"""The calls of tests/scan_calls.py with a truth table (CRYO_FILTER_TRUTH): cryo_codec_filter_batch / _agg_batch / _group_batch /
_project_batch on device copies of the streams and descriptors, and their host-buffer forms, with truth=None the flag-less call.
Device, the sentinels and the comparisons are scan_calls': every output buffer is filled with a sentinel before a call, nothing
at or beyond the totals or the caps may be written, and after every device-resident call the caller's key array is read back.
Test infrastructure only."""
import numpy as np

import project_ref as pr
import scan_calls
from pg_cryogen_amd import codec as cc
from scan_calls import REC_SENTINEL, SENTINEL


# ---- device-resident calls ----
def filter_batch(codec, method, comps, B, atts, keys, flags=0, truth=None, shift=0):
    n = len(comps)
    with scan_calls.Device(codec, comps, atts, keys, shift) as d:
        dst, rec = d.alloc(n * B + 64, SENTINEL), d.alloc(8 * 290 * n + 64, SENTINEL)
        tab, tot = d.alloc(32 * n, 0xEE), d.alloc(16, 0xEE)
        codec.filter_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, flags, dst, n * B,
                           rec, 290 * n, tab, tot, truth=truth)
        codec.sync()
        d.keys_untouched()
        t = tot.download(dtype=np.uint64)
        return (tab.download(dtype=np.uint8).view(cc.FILTER_BLOCK).copy(), rec.download(dtype=np.uint8).view(cc.FILTER_REC).copy(),
                dst.download(), (int(t[0]), int(t[1])))


def agg_batch(codec, method, comps, B, atts, keys, cols, truth=None, shift=0):
    n, nc = len(comps), len(cols)
    with scan_calls.Device(codec, comps, atts, keys, shift) as d:
        g = d.put(cc.agg_desc(cols)[1])
        rows, cells = d.alloc(16 * n + 64, SENTINEL), d.alloc(40 * n * nc + 64, SENTINEL)
        codec.agg_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, nc, g, rows, cells,
                        truth=truth)
        codec.sync()
        d.keys_untouched()
        r, c = rows.download(), cells.download()
        assert (r[16 * n:] == SENTINEL).all() and (c[40 * n * nc:] == SENTINEL).all(), "a byte beyond the call's output was written"
        return r[:16 * n].view(cc.AGG_BLOCK).copy(), c[:40 * n * nc].view(cc.AGG_CELL).reshape(n, nc).copy()


def group_batch(codec, method, comps, B, atts, keys, by, cols, truth=None, shift=0):
    n, nc, cap = len(comps), len(cols), 290 * len(comps)
    with scan_calls.Device(codec, comps, atts, keys, shift) as d:
        b, g = d.put(cc.group_desc(by)[1]), d.put(cc.agg_desc(cols)[1])
        rows, recs, cells, total = (d.alloc(32 * n + 64, SENTINEL), d.alloc(24 * cap + 64, SENTINEL),
                                    d.alloc(40 * cap * nc + 64, SENTINEL), d.alloc(8, SENTINEL))
        codec.group_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, len(by), b, nc,
                          g if nc else None, rows, recs, cap, cells if nc else None, total, truth=truth)
        codec.sync()
        d.keys_untouched()
        r, q, c = rows.download(), recs.download(), cells.download()
        tot = int(total.download().view("<u8")[0])
        assert tot <= cap and (r[32 * n:] == SENTINEL).all() and (q[24 * tot:] == SENTINEL).all() and (c[40 * tot * nc:] == SENTINEL).all()
        return (r[:32 * n].view(cc.GROUP_BLOCK).copy(), q[:24 * tot].view(cc.GROUP_REC).copy(),
                c[:40 * tot * nc].view(cc.AGG_CELL).reshape(tot, nc).copy(), tot)


def project_batch(codec, method, comps, B, atts, keys, cols, truth=None, shift=0):
    """(table, records, rows of shape (rows written, row_bytes), (total rows, total records)), the caps at their worst case"""
    n = len(comps)
    _, rb = pr.row_layout(atts, cols)
    cap = 290 * n
    with scan_calls.Device(codec, comps, atts, keys, shift) as d:
        p = d.put(cc.project_desc(cols)[1])
        table, rec, rows, total = (d.alloc(32 * n + 64, SENTINEL), d.alloc(8 * cap + 64, SENTINEL), d.alloc(rb * cap + 64, SENTINEL),
                                   d.alloc(16, SENTINEL))
        codec.project_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, len(cols), p, rows, cap,
                            rec, cap, table, total, truth=truth)
        codec.sync()
        d.keys_untouched()
        t, q, w = table.download(), rec.download(), rows.download()
        tw, tr = (int(v) for v in total.download()[:16].view("<u8"))
        assert tw <= cap and tr <= cap and (t[32 * n:] == SENTINEL).all(), "a byte beyond the block table was written"
        assert (q[8 * tr:] == SENTINEL).all() and (w[rb * tw:] == SENTINEL).all(), "a byte at or beyond the totals was written"
        return (t[:32 * n].view(cc.PROJECT_BLOCK).copy(), q[:8 * tr].view(cc.PROJECT_REC).copy(), w[:rb * tw].reshape(tw, rb).copy(),
                (tw, tr))


# ---- host-buffer calls ----
def filter_host(codec, method, comps, B, atts, keys, flags=0, truth=None):
    n = max(len(comps), 1)
    return codec.filter_blocks(method, comps, B, cc.filter_desc(atts, keys, flags, truth), dst=np.full(n * B, SENTINEL, np.uint8),
                               rec=np.full(n * 290, REC_SENTINEL, cc.FILTER_REC))


def agg_host(codec, method, comps, B, atts, keys, cols, truth=None):
    return codec.agg_blocks(method, comps, B, cc.filter_desc(atts, keys, 0, truth), cc.agg_desc(cols))


def group_host(codec, method, comps, B, atts, keys, by, cols, truth=None):
    return codec.group_blocks(method, comps, B, cc.filter_desc(atts, keys, 0, truth), cc.group_desc(by), cc.agg_desc(cols) if cols else None)


def project_host(codec, method, comps, B, atts, keys, cols, truth=None):
    n = len(comps)
    _, rb = pr.row_layout(atts, cols)
    rows = np.full((max(n, 1) * 290, rb), SENTINEL, np.uint8)
    rec = np.full(8 * max(n, 1) * 290, SENTINEL, np.uint8).view(cc.PROJECT_REC)
    table, rec, rows, (tw, tr) = codec.project_blocks(method, comps, B, cc.filter_desc(atts, keys, 0, truth), cc.project_desc(cols), rb, rows, rec)
    assert (rows[tw:] == SENTINEL).all() and (rec[tr:].view(np.uint8) == SENTINEL).all(), "a byte beyond the totals was written"
    return table, rec[:tr].copy(), rows[:tw].copy(), (tw, tr)
