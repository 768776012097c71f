"""GPU tests of the ordered scan's host side: cryo_topn_scan and the merge (host/topn.h) through the SHIPPED host library -- the real
HIP codec behind the walk, no test double, no test hook -- against tests/topn_ref.py on the oracle's decode, and the transfer
counters of cryo_codec_topn_blocks, which must grow by exactly what include/cryo_codec.h states."""
import ctypes as C

import numpy as np
import pytest

import fetch_walk
import filter_ref as fr
import project_ref as pr
import topn_ref as tr
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc, host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4), (2, 2), (8, 8), (4, 4)]          # (rowid int4, text, g int2, ts int8, app int4)
COLS = [1, 4, 3]                                          # widths 4, 8, 2: offsets 0, 8, 16; 24 bytes
BY = [(4, fr.INT8, tr.DESC | tr.NULLS_FIRST), (3, fr.INT2, 0)]   # ORDER BY ts DESC (PostgreSQL's default: NULLS FIRST), g
PER = 200


def make_blocks(B, n):
    """timestamps repeat within and across blocks and every 13th is NULL; g is NULL for every 11th row"""
    raws = []
    for k in range(n):
        ids = range(PER * k, PER * (k + 1))
        raws.append(tc.build_block(B, [tc.form_tuple(ATTS, [r, b"w" * (r % 90), None if r % 11 == 0 else r % 7 - 3,
                                                            None if r % 13 == 0 else (r * 7919) % 500 - 250, r % 20]) for r in ids]))
    return raws


@pytest.fixture()
def HT():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_topn_ops")
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


def test_topn_scan_and_merge_production_library(HT, oracle):
    L, errors = HT
    B, n, limit = 131072, 12, 100
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4343, C.byref(rel))
    raws, firsts = make_blocks(B, n), []
    for k in range(n):
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    keys = [(5, fr.INT4, cc.OP_IN, [3, 17]), (1, fr.INT4, fr.GE, 150)]   # app_id IN (3, 17) AND rowid >= 150
    before_cache = (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls())
    pool = host.transfer_counters()
    events, t = host.topn_scan(rel, ATTS, keys, BY, limit, COLS)
    after = host.transfer_counters()
    assert (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls()) == before_cache   # the cache is not touched
    assert after[2:] == pool[2:]                                          # the device pool is neither read nor filled
    want = [tr.topn_call([raws[k]], ATTS, keys, BY, limit, COLS) for k in range(n)]
    assert [e[0] for e in events] == ["block"] * n and [e[1:3] for e in events] == [(firsts[k], 500 + k) for k in range(n)]
    for e, (tab, recs, rows, tot) in zip(events, want):
        assert e[3] == (int(tab["n_items"][0]), int(tab["n_match"][0]), int(tab["n_bad"][0])) and e[4].tobytes() == recs.tobytes()
        assert e[5].tobytes() == rows.tobytes()
    kept = sum(w[3] for w in want)
    assert kept == sum(min(limit, int(w[0]["n_match"][0])) for w in want) > 0 and events[0][3] == (PER, 5, 0)
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"], t["rows"]) == \
        (n, n * PER, sum(int(w[0]["n_match"][0]) for w in want), 0, 0, 2, kept)
    assert t["bytes_back"] == n * 32 + kept * (24 + 24) == after[1] - pool[1]                         # nothing else came back
    # the merge of the blocks a snapshot sees -- every block but the third and the eighth -- is the plain sort of all their matches
    seen = [k for k in range(n) if k not in (2, 7)]
    every = [tr.topn_call([raws[k]], ATTS, keys, BY, 290, COLS) for k in seen]
    flat = sorted(((tr.sort_key(BY, [int(x) for x in r["key"]], int(r["key_nulls"])), b, i), bytes(w))
                  for b, (_, recs, rows, _) in enumerate(every) for i, (r, w) in enumerate(zip(recs, rows)))
    for lim in (10, 25):
        ev, _ = host.topn_scan(rel, ATTS, keys, BY, lim, COLS)
        for merge in (host.topn_merge, cc.topn_merge, tr.merge):
            recs, rows = merge(BY, lim, [(ev[k][4], ev[k][5]) for k in seen])
            assert [bytes(w) for w in rows] == [w for _, w in flat[:lim]] and len(rows) == lim
    # a damaged stream in the middle is reported in place and the scan goes on
    C.memset(L.cryo_memrel_page(mem, firsts[6]) + 48, 0xFF, 64)
    events, t = host.topn_scan(rel, ATTS, keys, BY, limit, COLS)
    assert [e[0] for e in events] == ["block"] * 6 + ["report"] + ["block"] * 5 and events[6] == ("report", firsts[6], fr.STREAM, 0)
    assert t["reports"] == 1 and t["rows"] == kept - want[6][3]
    assert not errors
    L.cryo_memrel_destroy(mem)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_transfer_and_codec_counters(codec, oracle, method):
    """d2h_bytes grows by exactly 32 * n_blocks + (24 + row_bytes) * total and h2d_bytes by the staged streams plus
    align16(4 * natts) + 16 * nkeys + 80; the pool and the codec counters stand still; under a small budget (several chunks) the
    same exact figures"""
    B, n = 131072, 12
    raws = make_blocks(B, n)
    comps = [oracle.lz4_compress(r, 1) if method == METHOD_LZ4 else oracle.zstd_compress(r, 1) for r in raws]
    keys = [(1, fr.INT4, fr.GE, 450), (1, fr.INT4, fr.LT, 1500)]
    t0 = codec.transfer_counters()
    codec.check_blocks(method, comps, B)
    check_up = codec.transfer_counters()["h2d_bytes"] - t0["h2d_bytes"]
    codec.set_option(cc.OPT_POOL_BYTES, 8 * B)
    rb = pr.row_layout(ATTS, COLS)[1]
    try:
        for budget in (0, 2 << 20):
            codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
            for limit in (10, 1000):
                want = tr.topn_call(raws, ATTS, keys, BY, limit, COLS)
                desc, odesc, pdesc = cc.filter_desc(ATTS, keys), cc.order_desc(BY, limit), cc.project_desc(COLS)
                before_t, before_c = codec.transfer_counters(), codec.counters()
                table, rec, rows, total = codec.topn_blocks(method, comps, B, desc, odesc, pdesc, rb)
                after_t, after_c = codec.transfer_counters(), codec.counters()
                assert total == want[3] == (60 if limit == 10 else 1050)
                assert table.tobytes() == want[0].tobytes() and rec[:total].tobytes() == want[1].tobytes()
                assert rows[:total].tobytes() == want[2].tobytes()
                assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 32 * n + (24 + rb) * total
                assert after_t["h2d_bytes"] - before_t["h2d_bytes"] == check_up + ((4 * len(ATTS) + 15) & ~15) + 16 * len(keys) + 80
                for k in ("pool_hits", "pool_misses", "pool_blocks"):
                    assert after_t[k] == before_t[k], k
                assert after_c == before_c
    finally:
        codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
        codec.set_option(cc.OPT_POOL_BYTES, 0)
