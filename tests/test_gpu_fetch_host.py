"""GPU test of cryo_fetch_tuples (host/fetch.h) through the SHIPPED host library: the real HIP codec behind the walk, no test
double, no test hook.  The scenario and its assertions are those of the CPU walk test (tests/fetch_walk.py): the tuples are
compared with what cryo_read_data + cryo_storage_fetch hand out for the same TIDs."""
import ctypes as C
import struct

import pytest

import fetch_walk
from mini_am import load_relation
from pg_cryogen_amd import host

pytestmark = pytest.mark.gpu


@pytest.fixture()
def HG():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_fetch_ops")
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


def test_fetch_tuples_production_library(HG, oracle):
    L, errors = HG
    rows = [struct.pack("<i", i) for i in range(1, 10001)]
    mem, rel, blocks, firsts = load_relation(L, rows, 1, host.COMP_LZ4, batch=16, xid=777)
    assert len(blocks) == 35
    pages, events, totals = fetch_walk.build(L, oracle, mem, rel, blocks, firsts, 777)
    pool = host.transfer_counters()
    t = fetch_walk.check(L, rel, pages, events, totals, calls=2)
    after = host.transfer_counters()
    assert after[2:] == pool[2:]                                          # the device pool is neither read nor filled
    assert after[1] - pool[1] == t["bytes_back"]                          # nothing else came back
    assert t["bytes_back"] < t["blocks"] * host.get_block_size() // 8     # far below the decoded blocks
    # every block of the table, lossy: all 10 000 rows in order, one codec call
    got, t = host.fetch_tuples(rel, [(f, None) for f in firsts])
    assert [struct.unpack_from("<i", e[4], 24)[0] for e in got] == list(range(1, 10001))
    assert all(e[0] == "tuple" and e[3] == 777 for e in got)
    assert t["codec_calls"] == 1 and t["blocks"] == 35 and t["bad"] == 0 and t["tuples"] == 10000
    assert t["bytes_back"] == 10000 * 32 + 16 * 290 * 35 and t["bytes_back"] < 35 * 131072 // 4
    assert not errors
    L.cryo_memrel_destroy(mem)
