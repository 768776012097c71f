"""GPU test of cryo_group_scan (host/group.h) through the SHIPPED host library: the real HIP codec behind the walk, no test
double, no test hook.  A mini-AM relation of 16 crafted blocks of 128 KiB, half LZ4 and half zstd, grouped by an int2 column with
NULLs over a range of the int4 column that cuts through two blocks; every block's groups are compared with tests/group_ref.py."""
import ctypes as C

import pytest

import fetch_walk
import filter_ref as fr
import group_ref as gr
import tuple_craft as tc
from pg_cryogen_amd import host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (2, 2), (8, 8)]                         # (rowid int4, g int2, x int8)
BY, COLS = [(2, fr.INT2)], [(3, fr.INT8), (1, fr.INT4)]
PER = 200


@pytest.fixture()
def HG():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_group_ops")
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


def want_block(first, xid, raw, keys, cols=COLS):
    row, gs = gr.group_block(raw, ATTS, keys, BY, cols or [])
    return ("block", first, xid, row[1], row[2], row[3], [(k, n, [(c[0], c[1], c[2], (c[4] << 64) + c[3]) for c in cs]) for k, n, cs in gs])


def test_group_scan_production_library(HG, oracle):
    L, errors = HG
    B, n = 131072, 16
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws, firsts = [], []
    for k in range(n):
        ids = range(PER * k, PER * (k + 1))
        raws.append(tc.build_block(B, [tc.form_tuple(ATTS, [r, None if r % 11 == 0 else r % 7 - 3, (1 << 40) * r]) for r in ids]))
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    lo, hi = 5 * PER + 150, 7 * PER + 30                                  # blocks 5 and 7 in part, block 6 whole
    keys = [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)]
    before_cache = (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls())
    pool = host.transfer_counters()
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS)
    after = host.transfer_counters()
    assert (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls()) == before_cache   # the cache is not touched
    assert after[2:] == pool[2:]                                          # the device pool is neither read nor filled
    assert events == [want_block(firsts[k], 500 + k, raws[k], keys) for k in range(n)]
    assert [e[4] for e in events][4:9] == [0, 50, 200, 30, 0] and [len(e[6]) for e in events][4:9] == [0, 8, 8, 8, 0]
    assert [g[0] for g in events[6][6]] == [(v,) for v in range(-3, 4)] + [(None,)]                   # ascending, NULLS LAST
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"], t["groups"]) == \
        (n, n * PER, hi - lo, 0, 0, 2, 24)
    assert t["bytes_back"] == n * 32 + 24 * (24 + 2 * 40) == after[1] - pool[1]       # nothing else came back
    assert sum(c[1][3] for e in events for _, _, c in e[6]) == sum(range(lo, hi))    # the groups' sums of the rowid column
    # no aggregate column: records only
    events, t = host.group_scan(rel, ATTS, keys, BY, None)
    assert events == [want_block(firsts[k], 500 + k, raws[k], keys, None) for k in range(n)] and t["bytes_back"] == n * 32 + 24 * 24
    # a damaged stream in the middle is reported in place and the scan goes on
    C.memset(L.cryo_memrel_page(mem, firsts[6]) + 48, 0xFF, 64)
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS)
    assert events[6] == ("report", firsts[6], fr.STREAM, 0) and t["reports"] == 1 and t["groups"] == 16
    assert [e for e in events if e[0] == "block"] == [want_block(firsts[k], 500 + k, raws[k], keys) for k in range(n) if k != 6]
    assert not errors
    L.cryo_memrel_destroy(mem)
