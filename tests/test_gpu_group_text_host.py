"""GPU test of cryo_group_scan (host/group.h) with a text group column through the SHIPPED host library: the real HIP codec
behind the walk, no test double, no test hook.  A mini-AM relation of 8 crafted blocks of 128 KiB, half LZ4 and half zstd, grouped
by a country column of short values -- among them the empty string, NULLs and, in two blocks, values that are no key --; every
block's groups, cells and key bytes are compared with tests/group_text_ref.py, and a block with n_bad > 0 is delivered with its
counts."""
import ctypes as C

import pytest

import fetch_walk
import filter_ref as fr
import group_text_ref as gt
import tuple_craft as tc
from pg_cryogen_amd import host
from tuple_craft import Long, Toast

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4), (8, 8), (4, 4)]                # (rowid int4, country text, revenue int8, app int4)
COUNTRIES = [b"de", b"fr", b"", b"us", b"de\x00", b"a-long-name-of-a-country-32bytes", b"\xc3\xa9", b"\xff"]
BY, COLS = [(2, gt.BYTES)], [(3, fr.INT8), (1, fr.INT4)]
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


def country(k, r):
    """blocks 2 and 5 hold values that are no key: a pointer, and 33 bytes in line"""
    if r % 13 == 0:
        return None
    if k == 2 and r % 50 == 7:
        return Toast()
    if k == 5 and r % 40 == 9:
        return Long(b"x" * 33)
    v = COUNTRIES[(r * 7 + k) % len(COUNTRIES)]
    return Long(v) if r % 3 == 0 else v


def want_events(firsts, raws, keys, by, cols):
    res = gt.group_call(raws, ATTS, keys, by, cols)
    rows, recs, cells = res[:3]
    out = []
    for k, row in enumerate(rows):
        gs = []
        for g, (key, n_rows) in enumerate(gt.groups_of(res, by, k), int(row["first_group"])):
            gs.append((key, n_rows, [(int(c["n"]), int(c["min"]), int(c["max"]), (int(c["sum_hi"]) << 64) + int(c["sum_lo"])) for c in cells[g]]))
        out.append(("block", firsts[k], 500 + k, int(row["n_items"]), int(row["n_match"]), int(row["n_bad"]), gs))
    return out


def test_text_group_scan_production_library(HG, oracle):
    L, errors = HG
    B, n = 131072, 8
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4245, C.byref(rel))
    raws, firsts = [], []
    for k in range(n):
        ids = range(PER * k, PER * (k + 1))
        raws.append(tc.build_block(B, [tc.form_tuple(ATTS, [r, country(k, r), 3 * r - 500, r % 4]) for r in ids]))
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    keys = [(1, fr.INT4, fr.GE, PER + 50), (1, fr.INT4, fr.LT, 7 * PER + 120)]     # blocks 1 and 7 in part, block 0 not at all
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS, text=True)
    want = want_events(firsts, raws, keys, BY, COLS)
    assert events == want
    assert [e[4] for e in want][0] == 0 and all(e[4] > 0 and e[6] for e in want[1:])
    assert [e[5] > 0 for e in want] == [False, False, True, False, False, True, False, False]   # delivered with their counts
    assert t["bad"] == sum(e[5] for e in want) and t["matches"] == sum(e[4] for e in want) == sum(g[1] for e in want for g in e[6])
    assert {g[0][0] for e in events for g in e[6]} == set(COUNTRIES) | {None} and t["codec_calls"] == 2
    assert t["bytes_back"] == n * 32 + t["groups"] * (24 + 40 * 3)
    # country and app, no aggregate column
    by = [(2, gt.BYTES), (4, fr.INT4)]
    events, t = host.group_scan(rel, ATTS, keys, by, None, text=True)
    assert events == want_events(firsts, raws, keys, by, []) and t["bytes_back"] == n * 32 + t["groups"] * (24 + 40)
    assert not errors
    # without the flag a text group column is refused, and integer columns under the flag are the plain call
    with pytest.raises(host.GroupScanError) as e:
        host.group_scan(rel, ATTS, keys, BY, COLS)
    assert e.value.code == -1
    assert host.group_scan(rel, ATTS, keys, [(4, fr.INT4)], COLS, text=True) == host.group_scan(rel, ATTS, keys, [(4, fr.INT4)], COLS)
