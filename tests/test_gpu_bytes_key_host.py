"""GPU test of the three host walks (host/filter.h, host/aggregate.h, host/group.h) with a byte-string key, through the SHIPPED
host library: the real HIP codec behind the walks, no test double, no test hook.  A mini-AM relation of 12 chains, half LZ4 and
half zstd, whose text column holds 'k0' / 'k1' / 'k2', a NULL or an external pointer: reason 9 comes through as a report, the
totals count the undecided tuples as bad, and tuples, cells and groups are what tests/bytes_key_ref.py says."""
import ctypes as C

import pytest

import bytes_key_ref as br
import fetch_walk
import tuple_craft as tc
from pg_cryogen_amd import host
from tuple_craft import Toast

pytestmark = pytest.mark.gpu

B = 131072
ATTS = [(4, 4), (-1, 4), (8, 8)]                        # (rowid int4, tag text, x int8)
KEYS = [(2, br.BYTES, br.EQ, b"k1"), (1, br.INT4, br.GT, 10)]
ROWS = 12 * 40


@pytest.fixture()
def HP():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_filter_ops")
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B)
    L.cryo_define_compression_gucs()
    L.cryo_cache_configure(16)
    yield L, errors
    L.cryo_cache_shutdown()
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)
    host.use(production=None)


def _tag(r):
    return Toast() if r % 7 == 0 else None if r % 5 == 0 else b"k" + bytes([48 + r % 3])


def _relation(L, oracle):
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws, firsts = [], []
    for k in range(12):
        raw = tc.build_block(B, [tc.form_tuple(ATTS, [r, _tag(r), -3 * r]) for r in range(40 * k + 1, 40 * k + 41)])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def test_scans_with_a_byte_string_key_production_library(HP, oracle):
    L, errors = HP
    mem, rel, raws, firsts = _relation(L, oracle)
    rows = [r for r in range(11, ROWS + 1) if r % 3 == 1 and r % 7 and r % 5]
    und = [r for r in range(11, ROWS + 1) if r % 7 == 0]
    # the filter: tuples in block and position order, reason 9 between them
    events, t = host.filter_scan(rel, ATTS, KEYS)
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == rows
    assert [e for e in events if e[0] == "report"] == [("report", firsts[(r - 1) // 40], br.UNDECIDED, (r - 1) % 40 + 1) for r in und]
    want = br.filter_call(raws, ATTS, KEYS)
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"]) == (12, ROWS, len(rows), len(und), len(und))
    assert t["matches"] == int(want[0]["n_match"].sum()) and t["bad"] == int(want[0]["n_bad"].sum())
    assert t["bytes_back"] == 32 * 12 + 8 * (len(rows) + len(und)) + want[3][0]
    events, c = host.filter_scan(rel, ATTS, KEYS, br.COUNT_ONLY)
    assert events == [] and (c["matches"], c["bad"], c["reports"]) == (len(rows), len(und), 0)
    # the aggregate: an undecided tuple is in no cell
    events, t = host.aggregate_scan(rel, ATTS, KEYS, [(3, br.INT8)])
    blocks = [e for e in events if e[0] == "block"]
    awant = br.agg_call(raws, ATTS, KEYS, [(3, br.INT8)])
    assert [(e[3], e[4], e[5]) for e in blocks] == [(40, int(r["n_match"]), int(r["n_bad"])) for r in awant[0]]
    assert t["cells"][0] == (len(rows), -3 * rows[-1], -3 * rows[0], -3 * sum(rows)) and (t["matches"], t["bad"]) == (len(rows), len(und))
    # the grouped scan: an undecided tuple is in no group
    events, t = host.group_scan(rel, ATTS, KEYS, [(1, br.INT4)], [(3, br.INT8)])
    blocks = [e for e in events if e[0] == "block"]
    assert [g[0][0] for e in blocks for g in e[6]] == rows
    assert (t["matches"], t["groups"], t["bad"]) == (len(rows), len(rows), len(und))
    assert not errors
    L.cryo_memrel_destroy(mem)
