"""The calls the GPU tests of the ordered scan share: cryo_codec_topn_batch on device copies of the streams and descriptors,
cryo_codec_topn_blocks, cryo_multi_topn_blocks, and the comparison with tests/topn_ref.py.  Every output buffer is filled with a
sentinel before a call: nothing at or beyond the total or the cap may be written.  Test infrastructure only."""
import numpy as np

import project_ref as pr
from pg_cryogen_amd import codec as cc
from scan_calls import SENTINEL, multi_call, pack_streams


def per_block(limit):
    return min(limit, 290)


def topn_batch(codec, method, comps, B, atts, keys, by, limit, cols, row_cap=None, truth=None):
    """cryo_codec_topn_batch on device copies of the streams and of the descriptors (the constants of byte-string and set keys
    included): (table, records, rows of shape (rows written, row_bytes), total).  Table, records, rows and total are filled with
    SENTINEL before the call; the 64 bytes behind the table and everything at or beyond min(total, cap) of records and rows must
    still hold it afterwards, and the caller's key array what was uploaded"""
    n = len(comps)
    _, rb = pr.row_layout(atts, cols)
    cap = per_block(limit) * n if row_cap is None else row_cap
    packed, offs, sizes = pack_streams(comps)
    a, k, consts, rebase = cc.filter_desc_device(atts, keys)
    _, o = cc.order_desc(by, limit)
    _, p = cc.project_desc(cols)
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * max(n, 1)), codec.alloc(4 * max(n, 1)), codec.alloc(a.nbytes), codec.alloc(k.nbytes),
            codec.alloc(consts.nbytes + 16), codec.alloc(o.nbytes), codec.alloc(p.nbytes), codec.alloc(32 * n + 64),
            codec.alloc(24 * cap + 64), codec.alloc(rb * cap + 64), codec.alloc(16)]
    d_src, d_off, d_sz, d_atts, d_keys, d_consts, d_by, d_cols, d_table, d_rec, d_rows, d_total = bufs
    try:
        for d, h in ((d_src, packed), (d_off, offs), (d_sz, sizes), (d_atts, a), (d_consts, consts), (d_by, o), (d_cols, p)):
            if h.nbytes:
                d.upload(h)
        d_keys.upload(rebase(d_consts.ptr))
        for d in (d_table, d_rec, d_rows, d_total):
            d.memset(SENTINEL)
        codec.topn_batch(method, d_src, d_off, d_sz, B, n, len(atts), d_atts, len(keys), d_keys if keys else None, len(by), limit, d_by,
                         len(cols), d_cols, d_rows, d_rec, cap, d_table, d_total, truth=truth)
        codec.sync()
        assert np.array_equal(d_keys.download(k.nbytes).view(cc.FILTER_KEY), k), "the caller's key array was written"
        table, rec, rows, tot = d_table.download(), d_rec.download(), d_rows.download(), d_total.download()
        total = int(tot[:8].view("<u8")[0])
        assert (tot[8:] == SENTINEL).all(), "the total has one entry"
        w = min(total, cap)
        assert (table[32 * n:] == SENTINEL).all(), "a byte beyond the block table was written"
        assert (rec[24 * w:] == SENTINEL).all(), "a byte at or beyond the records' total or cap was written"
        assert (rows[rb * w:] == SENTINEL).all(), "a byte at or beyond the rows' total or cap was written"
        return (table[:32 * n].view(cc.TOPN_BLOCK).copy(), rec[:24 * w].view(cc.TOPN_REC).copy(), rows[:rb * w].reshape(w, rb).copy(), total)
    finally:
        for x in bufs:
            x.free()


def host_buffers(n, limit, rb, row_cap=None):
    cap = max(n, 1) * per_block(limit) if row_cap is None else row_cap
    return (np.full((cap, rb), SENTINEL, np.uint8), np.full(24 * cap, SENTINEL, np.uint8).view(cc.TOPN_REC))


def topn_host(codec, method, comps, B, atts, keys, by, limit, cols, row_cap=None, truth=None):
    """cryo_codec_topn_blocks with sentinel-filled buffers of the given capacity; the same tuple as topn_batch"""
    _, rb = pr.row_layout(atts, cols)
    rows, rec = host_buffers(len(comps), limit, rb, row_cap)
    table, rec, rows, total = codec.topn_blocks(method, comps, B, cc.filter_desc(atts, keys, truth=truth), cc.order_desc(by, limit),
                                                cc.project_desc(cols), rb, rows, rec)
    assert (rows[total:] == SENTINEL).all() and (rec[total:].view(np.uint8) == SENTINEL).all(), "a byte beyond the total was written"
    return table, rec[:total].copy(), rows[:total].copy(), total


def topn_multi(G, method, comps, B, atts, keys, by, limit, cols, truth=None):
    """cryo_multi_topn_blocks with G handles on device 0 and sentinel-filled buffers: (table, the whole record buffer, the whole row
    buffer, total)"""
    _, rb = pr.row_layout(atts, cols)
    rows, rec = host_buffers(len(comps), limit, rb)
    desc, odesc, pdesc = cc.filter_desc(atts, keys, truth=truth), cc.order_desc(by, limit), cc.project_desc(cols)
    return multi_call([0] * G, lambda L, h, chk: cc.topn_blocks_call(L.cryo_multi_topn_blocks, h, chk, method, comps, B, desc, odesc,
                                                                     pdesc, rb, rows, rec))


def same_topn(got, want, what=""):
    table, rec, rows, total = got
    etable, erec, erows, etotal = want
    assert total == etotal, (what, total, etotal)
    assert table.shape == etable.shape and rec.shape == erec.shape and rows.shape == erows.shape, \
        (what, table.shape, etable.shape, rec.shape, erec.shape, rows.shape, erows.shape)
    for f in etable.dtype.names:
        bad = np.flatnonzero(table[f] != etable[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(table[i]), tuple(etable[i])) for i in bad[:5]])
    bad = [i for i in range(len(rec)) if rec[i].tobytes() != erec[i].tobytes()]  # 24 bytes without a pad: byte for byte
    assert not bad, (what, "records", [(i, rec[i], erec[i]) for i in bad[:5]])
    bad = np.flatnonzero((rows != erows).any(axis=1)) if rows.size else np.zeros(0, int)
    assert bad.size == 0, (what, "rows", [(int(i), bytes(rows[i]).hex(), bytes(erows[i]).hex()) for i in bad[:5]])


def same_multi(got, want, limit, what=""):
    """topn_multi's result against topn_ref.multi_call's: the table, every handle's region, the sentinel everywhere else"""
    table, rec, rows, total = got
    etable, regions, eend = want
    assert total == eend, (what, total, eend)
    for f in etable.dtype.names:
        assert (table[f] == etable[f]).all(), (what, f, table[f].tolist(), etable[f].tolist())
    used = np.zeros(len(rec), bool)
    for first, erows, erecs in regions:
        k = len(erecs)
        assert rec[first:first + k].tobytes() == erecs.tobytes(), (what, "records of the region at", first)
        assert np.array_equal(rows[first:first + k], erows), (what, "rows of the region at", first)
        used[first:first + k] = True
    assert (rec[~used].view(np.uint8) == SENTINEL).all() and (rows[~used] == SENTINEL).all(), (what, "an entry outside the regions' used parts was written")
