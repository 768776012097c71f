"""The calls the GPU tests of the scans share: cryo_codec_filter_batch / _agg_batch / _group_batch / _project_batch on device
copies of the streams and descriptors (the constants of byte-string keys included), their host-buffer forms, a cryo_multi_*
handle, and the comparisons with a reference's result.  Every output buffer is filled with a sentinel before a call: nothing at or
beyond the totals or the caps may be written, and after every device-resident call of Device the caller's key array is read back.
Test infrastructure only."""
import ctypes as C

import numpy as np

import project_ref as pr
from pg_cryogen_amd import METHOD_LZ4, codec as cc

SENTINEL = 0xA5
REC_SENTINEL = np.frombuffer(bytes([SENTINEL] * 8), cc.FILTER_REC)[0]


class Encoder:
    """the oracle's stream of a block, encoded once per method"""

    def __init__(self, oracle):
        self.oracle, self.seen = oracle, {}

    def __call__(self, method, block):
        key = (method, block.tobytes())
        if key not in self.seen:
            self.seen[key] = self.oracle.lz4_compress(block, 1) if method == METHOD_LZ4 else self.oracle.zstd_compress(block, 1)
        return self.seen[key]


# ---- device-resident calls ----
class Device:
    """the device buffers of one call: streams, descriptor, constants; freed on exit"""

    def __init__(self, codec, comps, atts, keys, shift=0):
        self.codec, self.bufs, self.n = codec, [], len(comps)
        sizes = np.array([len(c) for c in comps], np.uint32)
        offs = np.zeros(self.n, np.uint64)
        at = 0
        for i, c in enumerate(comps):
            offs[i] = at
            at += (len(c) + 15) & ~15
        packed = np.zeros(max(at, 16), np.uint8)
        for i, c in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + len(c)] = np.asarray(c, np.uint8)
        a, self.k, consts, rebase = cc.filter_desc_device(atts, keys)
        self.src, self.off, self.sz = self.put(packed), self.put(offs), self.put(sizes)
        self.atts = self.put(a)
        self.consts = self.alloc(consts.nbytes + 8)
        self.consts.upload(consts, shift)                              # the constants back to back from ptr + shift on
        rebase(self.consts.ptr + shift)
        self.natts, self.nkeys = len(atts), len(keys)
        self.keys = self.put(self.k)

    def alloc(self, nbytes, fill=None):
        b = self.codec.alloc(max(int(nbytes), 8))
        self.bufs.append(b)
        if fill is not None:
            b.memset(fill)
        return b

    def put(self, arr):
        b = self.alloc(arr.nbytes)
        b.upload(arr)
        return b

    def keys_untouched(self):
        assert np.array_equal(self.keys.download(self.k.nbytes).view(cc.FILTER_KEY), self.k), "the caller's key array was written"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def filter_batch(codec, method, comps, B, atts, keys, flags=0, shift=0):
    n = len(comps)
    with Device(codec, comps, atts, keys, shift) as d:
        dst, rec = d.alloc(n * B + 64, SENTINEL), d.alloc(8 * 290 * n + 64, SENTINEL)
        tab, tot = d.alloc(32 * n, 0xEE), d.alloc(16, 0xEE)
        codec.filter_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, flags, dst, n * B,
                           rec, 290 * n, tab, tot)
        codec.sync()
        d.keys_untouched()
        t = tot.download(dtype=np.uint64)
        return (tab.download(dtype=np.uint8).view(cc.FILTER_BLOCK).copy(), rec.download(dtype=np.uint8).view(cc.FILTER_REC).copy(),
                dst.download(), (int(t[0]), int(t[1])))


def agg_batch(codec, method, comps, B, atts, keys, cols, shift=0):
    n, nc = len(comps), len(cols)
    with Device(codec, comps, atts, keys, shift) as d:
        g = d.put(cc.agg_desc(cols)[1])
        rows, cells = d.alloc(16 * n + 64, SENTINEL), d.alloc(40 * n * nc + 64, SENTINEL)
        codec.agg_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, nc, g, rows, cells)
        codec.sync()
        d.keys_untouched()
        r, c = rows.download(), cells.download()
        assert (r[16 * n:] == SENTINEL).all() and (c[40 * n * nc:] == SENTINEL).all(), "a byte beyond the call's output was written"
        return r[:16 * n].view(cc.AGG_BLOCK).copy(), c[:40 * n * nc].view(cc.AGG_CELL).reshape(n, nc).copy()


def group_batch(codec, method, comps, B, atts, keys, by, cols, shift=0):
    n, nc, cap = len(comps), len(cols), 290 * len(comps)
    with Device(codec, comps, atts, keys, shift) as d:
        b, g = d.put(cc.group_desc(by)[1]), d.put(cc.agg_desc(cols)[1])
        rows, recs, cells, total = (d.alloc(32 * n + 64, SENTINEL), d.alloc(24 * cap + 64, SENTINEL),
                                    d.alloc(40 * cap * nc + 64, SENTINEL), d.alloc(8, SENTINEL))
        codec.group_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, len(by), b, nc,
                          g if nc else None, rows, recs, cap, cells if nc else None, total)
        codec.sync()
        d.keys_untouched()
        r, q, c = rows.download(), recs.download(), cells.download()
        tot = int(total.download().view("<u8")[0])
        assert tot <= cap and (r[32 * n:] == SENTINEL).all() and (q[24 * tot:] == SENTINEL).all() and (c[40 * tot * nc:] == SENTINEL).all()
        return (r[:32 * n].view(cc.GROUP_BLOCK).copy(), q[:24 * tot].view(cc.GROUP_REC).copy(),
                c[:40 * tot * nc].view(cc.AGG_CELL).reshape(tot, nc).copy(), tot)


# ---- host-buffer calls ----
def filter_host(codec, method, comps, B, atts, keys, flags=0):
    n = max(len(comps), 1)
    return codec.filter_blocks(method, comps, B, cc.filter_desc(atts, keys, flags), dst=np.full(n * B, SENTINEL, np.uint8),
                               rec=np.full(n * 290, REC_SENTINEL, cc.FILTER_REC))


def agg_host(codec, method, comps, B, atts, keys, cols):
    return codec.agg_blocks(method, comps, B, cc.filter_desc(atts, keys), cc.agg_desc(cols))


def group_host(codec, method, comps, B, atts, keys, by, cols):
    return codec.group_blocks(method, comps, B, cc.filter_desc(atts, keys), cc.group_desc(by), cc.agg_desc(cols) if cols else None)


# ---- comparing ----
def same_fields(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, (what, f, [(tuple(int(x) for x in i), got[tuple(i)], want[tuple(i)]) for i in bad[:5]])


def same_filter(got, want, what=""):
    table, recs, dst, total = got
    etable, erecs, packed, etotal = want
    same_fields(table, etable, what)
    assert tuple(total) == tuple(etotal), (what, total, etotal)
    same_fields(recs[:erecs.size], erecs, what)
    assert (recs[erecs.size:].view(np.uint8) == SENTINEL).all(), (what, "a record at or beyond the total was written")
    diff = np.flatnonzero(dst[:packed.size] != packed)
    assert diff.size == 0, (what, "first differing byte", int(diff[0]))
    assert (dst[packed.size:] == SENTINEL).all(), (what, "a byte at or beyond the total was written")


def same_agg(got, want, what=""):
    same_fields(got[0], want[0], what)
    same_fields(got[1], want[1], what)


def same_group(got, want, what=""):
    assert got[3] == want[3], (what, got[3], want[3])
    for g, w in zip(got[:3], want[:3]):
        same_fields(g, w, what)


# ---- several handles ----
def multi_call(devices, fn):
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    try:
        def chk(rc, what):
            assert rc == 0, (what, rc, L.cryo_multi_last_error(h))
        return fn(L, h, chk)
    finally:
        L.cryo_multi_close(h)


# ---- the projection ----
def pack_streams(comps):
    n = len(comps)
    sizes = np.array([len(c) for c in comps], np.uint32)
    offs = np.zeros(n, np.uint64)
    at = 0
    for i, c in enumerate(comps):
        offs[i] = at
        at += (len(c) + 15) & ~15
    packed = np.zeros(max(at, 16), np.uint8)
    for i, c in enumerate(comps):
        packed[int(offs[i]):int(offs[i]) + len(c)] = np.asarray(c, np.uint8)
    return packed, offs, sizes


def project_batch(codec, method, comps, B, atts, keys, cols, row_cap=None, rec_cap=None):
    """cryo_codec_project_batch on device copies of the streams and of the descriptors (the constants of byte-string keys
    included): (table, records, rows of shape (rows written, row_bytes), (total rows, total records)).  Table, records and rows are
    filled with SENTINEL before the call; the 64 bytes behind the table and everything at or beyond min(total, cap) of records and
    rows must still hold it afterwards, and the caller's key array what was uploaded"""
    n = len(comps)
    _, rb = pr.row_layout(atts, cols)
    wcap = 290 * n if row_cap is None else row_cap
    rcap = 290 * n if rec_cap is None else rec_cap
    packed, offs, sizes = pack_streams(comps)
    a, k, consts, rebase = cc.filter_desc_device(atts, keys)
    _, p = cc.project_desc(cols)
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(a.nbytes), codec.alloc(k.nbytes),
            codec.alloc(consts.nbytes + 16), codec.alloc(p.nbytes), codec.alloc(32 * n + 64), codec.alloc(8 * rcap + 64),
            codec.alloc(rb * wcap + 64), codec.alloc(16)]
    d_src, d_off, d_sz, d_atts, d_keys, d_consts, d_cols, d_table, d_rec, d_rows, d_total = bufs
    try:
        for d, h in ((d_src, packed), (d_off, offs), (d_sz, sizes), (d_atts, a), (d_consts, consts), (d_cols, p)):
            d.upload(h)
        d_keys.upload(rebase(d_consts.ptr))
        for d in (d_table, d_rec, d_rows, d_total):
            d.memset(SENTINEL)
        codec.project_batch(method, d_src, d_off, d_sz, B, n, len(atts), d_atts, len(keys), d_keys if keys else None, len(cols), d_cols,
                            d_rows, wcap, d_rec, rcap, d_table, d_total)
        codec.sync()
        assert np.array_equal(d_keys.download(k.nbytes).view(cc.FILTER_KEY), k), "the caller's key array was written"
        table, rec, rows = d_table.download(), d_rec.download(), d_rows.download()
        tw, tr = (int(v) for v in d_total.download()[:16].view("<u8"))
        ww, wr = min(tw, wcap), min(tr, rcap)
        assert (table[32 * n:] == SENTINEL).all(), "a byte beyond the block table was written"
        assert (rec[8 * wr:] == SENTINEL).all(), "a byte at or beyond the records' total or cap was written"
        assert (rows[rb * ww:] == SENTINEL).all(), "a byte at or beyond the rows' total or cap was written"
        return (table[:32 * n].view(cc.PROJECT_BLOCK).copy(), rec[:8 * wr].view(cc.PROJECT_REC).copy(),
                rows[:rb * ww].reshape(ww, rb).copy(), (tw, tr))
    finally:
        for x in bufs:
            x.free()


def project_host(codec, method, comps, B, atts, keys, cols, row_cap=None, rec_cap=None):
    """cryo_codec_project_blocks with sentinel-filled buffers of the given capacities; the same tuple as project_batch"""
    n = len(comps)
    _, rb = pr.row_layout(atts, cols)
    rows = np.full((max(n, 1) * 290 if row_cap is None else row_cap, rb), SENTINEL, np.uint8)
    rec = np.full(8 * (max(n, 1) * 290 if rec_cap is None else rec_cap), SENTINEL, np.uint8).view(cc.PROJECT_REC)
    table, rec, rows, (tw, tr) = codec.project_blocks(method, comps, B, cc.filter_desc(atts, keys), cc.project_desc(cols), rb, rows, rec)
    assert (rows[tw:] == SENTINEL).all() and (rec[tr:].view(np.uint8) == SENTINEL).all(), "a byte beyond the totals was written"
    return table, rec[:tr].copy(), rows[:tw].copy(), (tw, tr)


def same_project(got, want, what=""):
    table, rec, rows, total = got
    etable, erec, erows, etotal = want
    assert tuple(total) == tuple(etotal), (what, total, etotal)
    assert table.shape == etable.shape and rec.shape == erec.shape and rows.shape == erows.shape, \
        (what, table.shape, etable.shape, rec.shape, erec.shape, rows.shape, erows.shape)
    for f in etable.dtype.names:
        bad = np.flatnonzero(table[f] != etable[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(table[i]), tuple(etable[i])) for i in bad[:5]])
    for f in erec.dtype.names:
        bad = np.flatnonzero(rec[f] != erec[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(rec[i]), tuple(erec[i])) for i in bad[:5]])
    bad = np.flatnonzero((rows != erows).any(axis=1)) if rows.size else np.zeros(0, int)
    assert bad.size == 0, (what, "rows", [(int(i), bytes(rows[i]).hex(), bytes(erows[i]).hex()) for i in bad[:5]])
