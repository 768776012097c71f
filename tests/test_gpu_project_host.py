"""GPU tests of the projecting scan's host side: cryo_project_scan (host/project.h) through the SHIPPED host library -- the real HIP
codec behind the walk, no test double, no test hook --, cryo_multi_project_blocks against tests/project_ref.py, and the transfer
counters of cryo_codec_project_blocks, which must grow by exactly what include/cryo_codec.h states."""
import ctypes as C
import struct

import numpy as np
import pytest

import filter_ref as fr
import fetch_walk
import project_ref as pr
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc, host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4), (2, 2), (8, 8), (1, 1)]          # (rowid int4, text, g int2, x float8 bits, flag bool)
COLS = [4, 5, 3, 1]                                       # widths 8, 1, 2, 4: offsets 0, 8, 10, 12; 16 bytes
PER = 200
SENTINEL = 0xA5


def make_blocks(B, n):
    raws = []
    for k in range(n):
        ids = range(PER * k, PER * (k + 1))
        raws.append(tc.build_block(B, [tc.form_tuple(ATTS, [r, b"w" * (r % 90), None if r % 11 == 0 else r % 7 - 3,
                                                            struct.unpack("<q", struct.pack("<d", 0.5 * r))[0], r & 1]) for r in ids]))
    return raws


@pytest.fixture()
def HP():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_project_ops")
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(131072)
    L.cryo_define_compression_gucs()
    L.cryo_cache_configure(16)
    yield L, errors
    L.cryo_cache_shutdown()
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)
    host.use(production=None)


def want_rows(first, xid, raw, keys):
    _, _, recs = pr.project_block(raw, ATTS, keys, COLS)
    return [("row", first, pos, xid, nulls, row) for pos, st, nulls, row in recs if st == 0]


def test_project_scan_production_library(HP, oracle):
    L, errors = HP
    B, n = 131072, 16
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4343, C.byref(rel))
    raws, firsts = make_blocks(B, n), []
    for k in range(n):
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    lo, hi = 5 * PER + 150, 7 * PER + 30                                  # blocks 5 and 7 in part, block 6 whole
    keys = [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)]
    before_cache = (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls())
    pool = host.transfer_counters()
    events, t = host.project_scan(rel, ATTS, keys, COLS)
    after = host.transfer_counters()
    assert (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls()) == before_cache   # the cache is not touched
    assert after[2:] == pool[2:]                                          # the device pool is neither read nor filled
    want = []
    for k in range(n):
        want += want_rows(firsts[k], 500 + k, raws[k], keys)
    assert events == want and len(events) == hi - lo
    assert events[0][1:5] == (firsts[5], 151, 505, 0) and events[0][5] == struct.pack("<dBxhi", 0.5 * lo, lo & 1, lo % 7 - 3, lo)
    nulls = [e for e in events if e[4]]
    assert len(nulls) == len([r for r in range(lo, hi) if r % 11 == 0]) and all(e[4] == 0b100 for e in nulls)
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"]) == (n, n * PER, hi - lo, 0, 0, 2)
    assert t["bytes_back"] == n * 32 + (hi - lo) * (8 + 16) == after[1] - pool[1]                     # nothing else came back
    # a damaged stream in the middle is reported in place and the scan goes on
    C.memset(L.cryo_memrel_page(mem, firsts[6]) + 48, 0xFF, 64)
    events, t = host.project_scan(rel, ATTS, keys, COLS)
    assert events == want_rows(firsts[5], 505, raws[5], keys) + [("report", firsts[6], fr.STREAM, 0)] + want_rows(firsts[7], 507, raws[7], keys)
    assert t["reports"] == 1 and t["matches"] == 50 + 30
    assert not errors
    L.cryo_memrel_destroy(mem)


def oracle_encode(oracle, method, raw):
    return oracle.lz4_compress(raw, 1) if method == METHOD_LZ4 else oracle.zstd_compress(raw, 1)


def multi_project(method, comps, B, atts, keys, cols, devices, row_cap=None, rec_cap=None):
    """cryo_multi_project_blocks into sentinel-filled buffers: (table, the whole record buffer, the whole row buffer, totals)"""
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    n = max(len(comps), 1)
    _, rb = pr.row_layout(atts, cols)
    rows = np.full((290 * n if row_cap is None else row_cap, rb), SENTINEL, np.uint8)
    rec = np.full(8 * (290 * n if rec_cap is None else rec_cap), SENTINEL, np.uint8).view(cc.PROJECT_REC)
    try:
        def chk(rc, what):
            if rc != 0:
                raise CryoError(rc, what, L.cryo_multi_last_error(h).decode())
        return cc.project_blocks_call(L.cryo_multi_project_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys),
                                      cc.project_desc(cols), rb, rows, rec)
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("devices", [(0,), (0, 0), (0, 1), None])
def test_multi_project_blocks(codec, oracle, devices):
    """one handle: cryo_codec_project_blocks byte for byte; two handles on one device, two devices, every visible device: the
    regions and the table of project_ref.multi_call, and nothing written outside the regions' used parts"""
    if devices is None:
        devices = tuple(range(cc.device_count()))
    if max(devices) >= cc.device_count():
        pytest.skip("one device visible")
    B, n = 131072, 11
    raws = make_blocks(B, n)
    keys = [(1, fr.INT4, fr.GE, 130), (1, fr.INT4, fr.LT, 1900)]
    G = len(devices)
    rb = pr.row_layout(ATTS, COLS)[1]
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, r) for r in raws]
        comps[2] = comps[2][:40]
        blocks = [None if i == 2 else r for i, r in enumerate(raws)]
        table, rec, rows, total = multi_project(method, comps, B, ATTS, keys, COLS, devices)
        etable, regions, etotal = pr.multi_call(blocks, ATTS, keys, COLS, G)
        assert total == etotal and table.tobytes() == etable.tobytes(), (method, devices)
        used_w, used_r = np.zeros(rows.shape[0], bool), np.zeros(rec.size, bool)
        for first, erows, erecs in regions:
            assert rows[first:first + erows.shape[0]].tobytes() == erows.tobytes(), (method, devices, first)
            assert rec[first:first + erecs.size].tobytes() == erecs.tobytes(), (method, devices, first)
            used_w[first:first + erows.shape[0]] = True
            used_r[first:first + erecs.size] = True
        assert (rows[~used_w] == SENTINEL).all() and (rec[~used_r].view(np.uint8) == SENTINEL).all()
        # every block's rows are found through the table alone, whatever the handle
        single = pr.project_call(blocks, ATTS, keys, COLS)
        for i in range(n):
            assert pr.rows_of(table, rec, rows, i) == pr.rows_of(*single[:3], i), (method, devices, i)
        if G == 1:
            one = codec.project_blocks(method, comps, B, cc.filter_desc(ATTS, keys), cc.project_desc(COLS), rb,
                                       np.full((290 * n, rb), SENTINEL, np.uint8),
                                       np.full(8 * 290 * n, SENTINEL, np.uint8).view(cc.PROJECT_REC))
            assert total == one[3] and all(a.tobytes() == b.tobytes() for a, b in zip((table, rec, rows), one[:3]))
            with pytest.raises(CryoError) as e:
                multi_project(method, comps, B, ATTS, keys, COLS, devices, etotal[0] - 1, 290 * n)
            assert e.value.code == cc.E_DSTSIZE
    table, rec, rows, total = multi_project(METHOD_LZ4, [], B, ATTS, keys, COLS, devices)
    assert table.size == 0 and total == (0, 0)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_transfer_and_codec_counters(codec, oracle, method):
    """d2h_bytes grows by exactly 32 * n_blocks + 8 * total[1] + row_bytes * total[0] -- per match 8 + row_bytes, where the filter
    brings 8 + MAXALIGN(len) -- and h2d_bytes by the staged streams plus align16(4 * natts) + 16 * nkeys + align16(8 * ncols); the
    pool and the codec counters stand still; under a small budget (several chunks) the same exact figures"""
    B, n = 131072, 12
    raws = make_blocks(B, n)
    raws[3] = raws[3].copy()
    raws[3][8 + 4:8 + 8] = 0                                              # a bad item: a record without a row
    comps = [oracle_encode(oracle, method, r) for r in raws]
    keys = [(1, fr.INT4, fr.GE, 450), (1, fr.INT4, fr.LT, 1500)]
    t0 = codec.transfer_counters()
    codec.check_blocks(method, comps, B)
    check_up = codec.transfer_counters()["h2d_bytes"] - t0["h2d_bytes"]
    codec.set_option(cc.OPT_POOL_BYTES, 8 * B)
    try:
        for budget in (0, 2 << 20):
            codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
            for cols in (COLS, [5], [4] * 8):
                want = pr.project_call(raws, ATTS, keys, cols)
                rb = pr.row_layout(ATTS, cols)[1]
                desc, pdesc = cc.filter_desc(ATTS, keys), cc.project_desc(cols)
                before_t, before_c = codec.transfer_counters(), codec.counters()
                table, rec, rows, total = codec.project_blocks(method, comps, B, desc, pdesc, rb)
                after_t, after_c = codec.transfer_counters(), codec.counters()
                assert total == want[3] == (1049, 1050)                   # rowids 450 .. 1499, one of them behind the bad item
                assert table.tobytes() == want[0].tobytes() and rec[:total[1]].tobytes() == want[1].tobytes()
                assert rows[:total[0]].tobytes() == want[2].tobytes()
                assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 32 * n + 8 * total[1] + rb * total[0]
                assert after_t["h2d_bytes"] - before_t["h2d_bytes"] == check_up + ((4 * len(ATTS) + 15) & ~15) + 16 * len(keys) + \
                    ((8 * len(cols) + 15) & ~15)
                for k in ("pool_hits", "pool_misses", "pool_blocks"):
                    assert after_t[k] == before_t[k], k
                assert after_c == before_c
            # the filter's route on the same keys: 8 + MAXALIGN(len) per match
            before_t = codec.transfer_counters()
            ftable, frec, fdst, (fb, frn) = codec.filter_blocks(method, comps, B, cc.filter_desc(ATTS, keys))
            after_t = codec.transfer_counters()
            assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 32 * n + 8 * frn + fb
            assert frn == want[3][1] and fb == sum(fr.maxalign(int(r["len"])) for r in frec[:frn] if r["status"] == 0) > 16 * want[3][0]
    finally:
        codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
        codec.set_option(cc.OPT_POOL_BYTES, 0)
