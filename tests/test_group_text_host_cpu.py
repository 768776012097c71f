"""CPU test of the grouped scan's host walk (host/group.c) under CRYO_GROUP_TEXT, through a codec double
(tests/group_text_double.py) whose group_blocks decodes with the oracle and answers from tests/group_text_ref.py: a relation with a
text group column and two aggregate columns.  The walk sizes the cells array and finds every block's cells by the cells of a
group -- the aggregate cells and the key cell --, so every callback's records, cells and key bytes are the reference's and
bytes_back counts the key cells."""
import ctypes as C

import pytest

import fetch_walk
import filter_ref as fr
import group_text_ref as gt
import tuple_craft as tc
from pg_cryogen_amd import host
from tuple_craft import Toast

B128 = 131072
ATTS = [(4, 4), (-1, 4), (8, 8), (4, 4)]                # (rowid int4, country text, revenue int8, app int4)
COUNTRIES = [b"de", b"fr", b"", b"us", b"de\x00", b"a-long-name-of-a-country-32bytes"]
BY, COLS = [(2, gt.BYTES)], [(3, fr.INT8), (1, fr.INT4)]


@pytest.fixture()
def HG():
    import group_text_double
    L = host.lib()
    dbl = group_text_double.TextGroupingDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_group_ops(C.byref(dbl.group_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_group_set_window(0, 0)
    L.cryo_cache_shutdown()
    L.cryo_host_set_group_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


def country(r):
    return None if r % 11 == 0 else Toast() if r % 53 == 0 else COUNTRIES[r % len(COUNTRIES)]


def relation(L, oracle, nblocks=7):
    """nblocks chains of 40 + k tuples (rowid, country -- NULL, a pointer or one of six values, one of them 32 bytes --, revenue
    = 7 rowid - 1000, app = rowid % 3): even ones LZ4, odd ones zstd, xid 500 + k"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4244, C.byref(rel))
    raws, firsts, at = [], [], 1
    for k in range(nblocks):
        ids = range(at, at + 40 + k)
        at += 40 + k
        raw = tc.build_block(B128, [tc.form_tuple(ATTS, [r, country(r), 7 * r - 1000, r % 3]) for r in ids])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def want_events(firsts, raws, keys, by, cols):
    """what host.group_scan delivers, from the reference alone: a text column's place in a key holds its bytes"""
    res = gt.group_call(raws, ATTS, keys, by, cols or [])
    rows, recs, cells = res[:3]
    out = []
    for k, row in enumerate(rows):
        gs, first = [], int(row["first_group"])
        for g, (key, n_rows) in enumerate(gt.groups_of(res, by, k), first):
            gs.append((key, n_rows, [(int(c["n"]), int(c["min"]), int(c["max"]), (int(c["sum_hi"]) << 64) + int(c["sum_lo"])) for c in cells[g]]))
        out.append(("block", firsts[k], 500 + k, int(row["n_items"]), int(row["n_match"]), int(row["n_bad"]), gs))
    return out


def test_group_scan_with_a_text_column_through_a_double(HG, oracle):
    L, dbl, errors = HG
    mem, rel, raws, firsts = relation(L, oracle)
    keys = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 280)]
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS, text=True)
    want = want_events(firsts, raws, keys, BY, COLS)
    assert events == want                                                 # records, cells and key bytes of every callback
    keys_seen = {g[0][0] for e in events for g in e[6]}
    assert keys_seen == set(COUNTRIES) | {None} and sum(e[5] for e in events) == len([r for r in range(30, 280) if r % 53 == 0 and r % 11]) > 0
    assert dbl.calls == [(host.COMP_LZ4, 4), (host.COMP_ZSTD, 3)]
    ngroups = sum(len(e[6]) for e in events)
    assert t["groups"] == ngroups and t["matches"] == sum(n for e in events for _, n, _ in e[6]) and t["bad"] == sum(e[5] for e in events)
    assert t["bytes_back"] == 7 * 32 + ngroups * (24 + 40 * (2 + 1))      # a key cell beside the two aggregate cells
    # text and int, no aggregate column: the cells array holds key cells alone
    for cols in (None, []):
        by = [(4, fr.INT4), (2, gt.BYTES)]
        events, t2 = host.group_scan(rel, ATTS, keys, by, cols, text=True)
        assert events == want_events(firsts, raws, keys, by, cols)
        assert t2["bytes_back"] == 7 * 32 + t2["groups"] * (24 + 40) and t2["groups"] > ngroups
    # two text columns: the same column twice gives two key cells
    by = [(2, gt.BYTES), (2, gt.BYTES)]
    events, t3 = host.group_scan(rel, ATTS, keys, by, COLS, text=True)
    assert events == want_events(firsts, raws, keys, by, COLS) and t3["bytes_back"] == 7 * 32 + ngroups * (24 + 40 * 4)
    # integer columns under the flag: what the plain call delivers
    plain, t4 = host.group_scan(rel, ATTS, keys, [(4, fr.INT4)], COLS)
    flagged, t5 = host.group_scan(rel, ATTS, keys, [(4, fr.INT4)], COLS, text=True)
    assert flagged == plain and t5 == t4
    # the walk in windows: the same delivery
    L.cryo_group_set_window(3, 0)
    again, t6 = host.group_scan(rel, ATTS, keys, BY, COLS, text=True)
    assert again == want and t6["codec_calls"] > t["codec_calls"] and t6["bytes_back"] == t["bytes_back"]
    L.cryo_group_set_window(0, 0)
    # a text column without the flag, and a text aggregate column, are refused by the codec
    with pytest.raises(host.GroupScanError) as e:
        host.group_scan(rel, ATTS, keys, BY, COLS)
    assert e.value.code == -1 and e.value.events == []
    with pytest.raises(host.GroupScanError) as e:
        host.group_scan(rel, ATTS, keys, BY, [(2, gt.BYTES)], text=True)
    assert e.value.code == -1 and e.value.events == []
    assert not errors
    L.cryo_memrel_destroy(mem)
