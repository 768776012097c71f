"""GPU test of cryo_aggregate_scan (host/aggregate.h) through the SHIPPED host library: the real HIP codec behind the walk, no
test double, no test hook.  A mini-AM relation of 16 `narrow` blocks of the generator, half LZ4 and half zstd, aggregated over a
range of the int4 column that cuts through two blocks; every block's partial is compared with tests/agg_ref.py."""
import ctypes as C

import pytest

import agg_ref as ar
import fetch_walk
import filter_ref as fr
from pg_cryogen_amd import host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4)]
COLS = [(1, fr.INT4), (1, fr.INT4)]


@pytest.fixture()
def HG():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_agg_ops")
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


def want_block(first, xid, raw, keys):
    row, cs = ar.agg_block(raw, ATTS, keys, COLS)
    return ("block", first, xid, row[1], row[2], row[3], [(c[0], c[1], c[2], (c[4] << 64) + c[3]) for c in cs])


def test_aggregate_scan_production_library(HG, oracle):
    L, errors = HG
    B, n = 131072, 16
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws = [oracle.synth(9, k, B, 1) for k in range(n)]
    firsts = []
    for k, raw in enumerate(raws):
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    lo, hi = 5 * 290 + 200, 7 * 290 + 30                                  # blocks 5 and 7 in part, block 6 whole
    keys = [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)]
    before_cache = (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls())
    pool = host.transfer_counters()
    events, t = host.aggregate_scan(rel, ATTS, keys, COLS)
    after = host.transfer_counters()
    assert (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls()) == before_cache   # the cache is not touched
    assert after[2:] == pool[2:]                                          # the device pool is neither read nor filled
    assert events == [want_block(firsts[k], 500 + k, raws[k], keys) for k in range(n)]
    assert [e[4] for e in events][4:9] == [0, 91, 290, 29, 0]
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"]) == (n, n * 290, hi - lo, 0, 0, 2)
    assert t["bytes_back"] == n * (16 + 2 * 40) == after[1] - pool[1]     # nothing else came back
    assert t["cells"] == [(hi - lo, lo, hi - 1, sum(range(lo, hi)))] * 2
    # a damaged stream in the middle is reported in place and the scan goes on
    C.memset(L.cryo_memrel_page(mem, firsts[6]) + 48, 0xFF, 64)
    events, t = host.aggregate_scan(rel, ATTS, keys, COLS)
    assert events[6] == ("report", firsts[6], fr.STREAM, 0) and t["reports"] == 1
    assert [e for e in events if e[0] == "block"] == [want_block(firsts[k], 500 + k, raws[k], keys) for k in range(n) if k != 6]
    assert t["cells"][0][0] == hi - lo - 290 and t["cells"][0][1:3] == (lo, hi - 1)
    assert not errors
    L.cryo_memrel_destroy(mem)
