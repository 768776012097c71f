"""GPU test of cryo_filter_scan (host/filter.h) through the SHIPPED host library: the real HIP codec behind the walk, no test
double, no test hook.  A mini-AM relation of 64 `narrow` blocks of the generator, half LZ4 and half zstd, scanned with a range of
about 1 % on the int4 column and counted with CRYO_FILTER_COUNT_ONLY; the tuples are compared with the generator's own bytes."""
import ctypes as C

import pytest

import fetch_ref
import fetch_walk
import filter_ref as fr
from pg_cryogen_amd import host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4)]


@pytest.fixture()
def HG():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_filter_ops")
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


def test_filter_scan_production_library(HG, oracle):
    L, errors = HG
    B = 131072
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws = [oracle.synth(9, k, B, 1) for k in range(64)]
    firsts = []
    for k, raw in enumerate(raws):
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    lo, hi = 5 * 290 + 200, 5 * 290 + 200 + 186                           # 186 of 18 560 rows: 1 %, across blocks 5 and 6
    keys = [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)]
    before_cache = (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls())
    pool = host.transfer_counters()
    events, t = host.filter_scan(rel, ATTS, keys)
    after = host.transfer_counters()
    assert (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls()) == before_cache   # the cache is not touched
    assert after[2:] == pool[2:]                                          # the device pool is neither read nor filled
    want = []
    for rowid in range(lo, hi):
        k, pos = (rowid - 1) // 290, (rowid - 1) % 290 + 1
        row = fetch_ref.slice_by_items(raws[k])[pos - 1].tobytes()
        want.append(("tuple", firsts[k], pos, 500 + k, row + bytes(-len(row) % 8), len(row)))
    assert events == want
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"]) == (64, 64 * 290, 186, 0, 0, 2)
    assert t["bytes_back"] == 32 * 64 + 8 * 186 + 64 * 186 == after[1] - pool[1]                      # nothing else came back
    assert t["bytes_back"] < 64 * B // 400
    # count(*): the block table only
    pool = host.transfer_counters()
    events, c = host.filter_scan(rel, ATTS, keys, fr.COUNT_ONLY)
    assert events == [] and (c["items"], c["matches"], c["bad"]) == (64 * 290, 186, 0)
    assert c["bytes_back"] == 32 * 64 == host.transfer_counters()[1] - pool[1]
    # a damaged stream in the middle is reported and the scan goes on
    C.memset(L.cryo_memrel_page(mem, firsts[5]) + 48, 0xFF, 64)
    events, t = host.filter_scan(rel, ATTS, keys)
    assert events == [("report", firsts[5], fr.STREAM, 0)] + [e for e in want if e[1] != firsts[5]] and t["reports"] == 1
    assert not errors
    L.cryo_memrel_destroy(mem)
