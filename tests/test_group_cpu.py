"""CPU tests of the grouped scan: the rules (tests/group_ref.py) on hand-made vectors (tests/group_cases.py, tests/agg_cases.py)
with the expected values written out here, the invariants that tie a block's groups to the aggregate's cell of the same block,
the descriptor rules, and cryo_group_scan (host/group.c) walking a mini-AM relation through the test build, with a codec double
(tests/group_double.py) whose group_blocks decodes with the oracle and answers by the rules."""
import ctypes as C
import struct

import numpy as np
import pytest

import agg_cases as ac
import agg_ref as ar
import fetch_walk
import filter_cases as fc
import filter_ref as fr
import group_cases as gc
import group_ref as gr
import tuple_craft as tc
from pg_cryogen_amd import codec, host

B128 = 131072
E_UNSUPPORTED, E_ARG = -6, -1
I64_MIN, I64_MAX = ac.I64_MIN, ac.I64_MAX


def groups(block, keys, by, cols, atts=ac.ATTS):
    return gr.group_block(block, atts, keys, by, cols)


# ---- the reference on hand-made vectors ----
def test_range_block():
    # i = 5 .. 11 of 30 match; grouped by column 1 = i every match is its own group, in ascending order
    row, gs = groups(ac.range_block(), ac.RANGE_KEYS, [(1, fr.INT2)], [(2, fr.INT8), (6, fr.INT8)])
    assert row == (0, 30, 7, 0)
    assert gs == [((i,), 1, [(1, 1000 + i, 1000 + i, 1000 + i, 0), (1, -i, -i, (1 << 64) - i, -1)]) for i in range(5, 12)]
    # grouped by column 6 = -i the order turns round
    row, gs = groups(ac.range_block(), ac.RANGE_KEYS, [(6, fr.INT8)], [])
    assert [g[0] for g in gs] == [(-i,) for i in range(11, 4, -1)] and all(g[1:] == (1, []) for g in gs)
    # nothing matches: no group
    assert groups(ac.range_block(), [(4, fr.INT4, fr.GT, 1000)], [(1, fr.INT2)], [(2, fr.INT8)]) == ((0, 30, 0, 0), [])


def test_order_block_by_hand():
    # int8 keys: the five values six times each, whatever the position order; x = the position, so the cells differ per group
    row, gs = groups(gc.order_block(), [], [(1, fr.INT8)], [(4, fr.INT8)], gc.ORDER_ATTS)
    assert row == (0, 30, 30, 0) and [g[0][0] for g in gs] == [I64_MIN, -1, 0, 1, I64_MAX] and [g[1] for g in gs] == [6] * 5
    assert sum(g[2][0][3] for g in gs) == 30 * 31 // 2 and all(g[2][0][0] == 6 for g in gs)
    # int4 then int2: (b, c) = (b[p % 3], c[p % 4]): twelve pairs, b ascending first, then c -- signed after sign extension
    row, gs = groups(gc.order_block(), [], [(2, fr.INT4), (3, fr.INT2)], [], gc.ORDER_ATTS)
    b, c = [-(1 << 31), 0, (1 << 31) - 1], [-(1 << 15), -1, 0, (1 << 15) - 1]
    assert [g[0] for g in gs] == [(x, y) for x in b for y in c]
    assert sorted(g[1] for g in gs) == [2] * 6 + [3] * 6


def test_second_column_decides():
    row, gs = groups(gc.second_differs_block(), [], [(1, fr.INT8), (3, fr.INT2)], [(4, fr.INT8)], gc.ORDER_ATTS)
    assert row == (0, 12, 12, 0)
    # c = 3, -3, 0, 32767, -32768, 3 twice over; x = 10 (p + 1)
    assert gs == [((I64_MAX, -32768), 2, [(2, 50, 110, 160, 0)]), ((I64_MAX, -3), 2, [(2, 20, 80, 100, 0)]),
                  ((I64_MAX, 0), 2, [(2, 30, 90, 120, 0)]), ((I64_MAX, 3), 4, [(4, 10, 120, 260, 0)]),
                  ((I64_MAX, 32767), 2, [(2, 40, 100, 140, 0)])]


def test_nulls_form_groups_and_sort_last():
    row, gs = groups(gc.nulls_block(), [], gc.NULL_BY2, [(3, fr.INT8)], gc.NULL_ATTS)
    assert row == (0, 10, 10, 0)
    assert gs == [((4, 9), 1, [(1, 90, 90, 90, 0)]), ((5, 5), 2, [(1, 40, 40, 40, 0)]), ((5, None), 3, [(1, 10, 10, 10, 0)]),
                  ((None, 5), 2, [(2, 20, 70, 90, 0)]), ((None, None), 2, [(0, 0, 0, 0, 0)])]
    # one column: the NULL group (bitmap and short natts together) comes last
    row, gs = groups(gc.nulls_block(), [], [(2, fr.INT4)], [(3, fr.INT8)], gc.NULL_ATTS)
    assert gs == [((5,), 4, [(3, 20, 70, 130, 0)]), ((9,), 1, [(1, 90, 90, 90, 0)]), ((None,), 5, [(1, 10, 10, 10, 0)])]
    # the records of a call: key 0 and the null bit for a NULL, key[1] = 0 without a second column
    rows, recs, cells, total = gr.group_call([gc.nulls_block()], gc.NULL_ATTS, [], gc.NULL_BY2, [(3, fr.INT8)])
    assert total == 5 and recs["key"].tolist() == [[4, 9], [5, 5], [5, 0], [0, 5], [0, 0]] and recs["nulls"].tolist() == [0, 0, 2, 1, 3]
    rows, recs, cells, total = gr.group_call([gc.nulls_block()], gc.NULL_ATTS, [], [(2, fr.INT4)], [])
    assert recs["key"].tolist() == [[5, 0], [9, 0], [0, 0]] and recs["nulls"].tolist() == [0, 0, 1] and cells.shape == (3, 0)


def test_extremes_need_128_bits():
    got = {name: groups(blk, [], [(2, fr.INT4)], [(1, fr.INT8)], ac.EXT_ATTS) for name, blk in ac.extremes_blocks()}
    assert got["min"] == ((0, 290, 290, 0), [((-(1 << 31),), 290, [(290, I64_MIN, I64_MIN, 0, -145)])])
    assert got["max"] == ((0, 290, 290, 0), [(((1 << 31) - 1,), 290, [(290, I64_MAX, I64_MAX, (1 << 64) - 290, 144)])])
    # the mix splits by key: 145 x INT64_MIN = -72.5 x 2^64, 145 x INT64_MAX = 72.5 x 2^64 - 145
    assert got["mix"][1] == [((-(1 << 31),), 145, [(145, I64_MIN, I64_MIN, 1 << 63, -73)]),
                             (((1 << 31) - 1,), 145, [(145, I64_MAX, I64_MAX, (1 << 63) - 145, 72)])]


def test_turn_blocks():
    for m in gc.TURN_SIZES:
        row, gs = groups(gc.turn_block("one", m), gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, gc.GX_ATTS)
        assert row == (0, m, m, 0) and gs == ([((7,), m, [(m, 0, m - 1, m * (m - 1) // 2, 0)])] if m else [])
        row, gs = groups(gc.turn_block("distinct", m), gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, gc.GX_ATTS)
        assert gs == [((1000 - 3 * p,), 1, [(1, p, p, p, 0)]) for p in range(m - 1, -1, -1)]      # the reverse of the position order
        row, gs = groups(gc.turn_block("alternate", m), gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, gc.GX_ATTS)
        assert [(g[0], g[1]) for g in gs] == [(k, n) for k, n in (((-5,), m // 2), ((5,), (m + 1) // 2)) if n]
        row, gs = groups(gc.turn_block("runs3", m), gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, gc.GX_ATTS)
        assert [g[1] for g in gs] == [gc.runs3(m).count(k) for k in sorted(set(gc.runs3(m)))]
    r = gc.runs3(290)
    assert all(r[b - 1] == r[b] for b in (64, 128, 192, 256)) and max(r.count(k) for k in set(r)) == 3
    # interleaved: behind every second match a tuple the key rejects, behind every seventh a damaged one
    row, gs = groups(gc.turn_block("alternate", 65, True), gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, gc.GX_ATTS)
    assert row == (0, 65 + 32 + 9, 65, 9) and [(g[0], g[1]) for g in gs] == [((-5,), 32), ((5,), 33)]


def test_walk_length_and_damage():
    blk = ac.cut_block()
    k1 = [(1, fr.INT2, fr.EQ, 5)]
    assert [r[:2] for r in fr.filter_block(blk, ac.ATTS, k1)[2]] == [(1, fr.OK), (2, fr.OK), (3, fr.OK)]     # the filter: a match
    assert groups(blk, k1, [(6, fr.INT8)], []) == ((0, 3, 2, 1), [((900,), 2, [])])       # here: TUPLE, the walk goes on to column 6
    assert groups(blk, k1, [(4, fr.INT4)], []) == ((0, 3, 3, 0), [((7,), 3, [])])
    blk, bad = ac.damaged_block()
    assert groups(blk, fc.WALK, [(4, fr.INT4)], [(6, fr.INT8)]) == ((0, 21, 11, 10), [((7,), 11, [(11, 900, 900, 9900, 0)])])
    assert groups(ac.bad_item_block(), fc.K6, [(1, fr.INT2)], [(2, fr.INT8)]) == ((0, 6, 5, 1), [((5,), 5, [(5, 100, 100, 500, 0)])])


def test_stream_and_header_blocks_have_no_groups():
    assert groups(None, [], [(1, fr.INT2)], ac.COLS4) == ((fr.STREAM, 0, 0, 0), [])
    assert groups(ac.header_block(), [], [(1, fr.INT2)], []) == ((fr.HEADER, 0, 0, 0), [])
    rows, recs, cells, total = gr.group_call([ac.range_block(), None, ac.header_block(), ac.range_block()], ac.ATTS, ac.RANGE_KEYS,
                                             [(1, fr.INT2)], [(2, fr.INT8)])
    assert rows["status"].tolist() == [0, fr.STREAM, fr.HEADER, 0] and rows["n_groups"].tolist() == [7, 0, 0, 7]
    assert rows["first_group"].tolist() == [0, 7, 7, 7] and total == 14 and not rows["rsv"].any()     # the successor's first_group
    assert recs["key"][:, 0].tolist() == list(range(5, 12)) * 2


def test_columns_in_several_roles():
    # column 4 as key, group column and aggregate column; a group column named twice
    row, gs = groups(ac.range_block(), ac.RANGE_KEYS, [(4, fr.INT4)], [(4, fr.INT4)])
    assert gs == [((10 * i,), 1, [(1, 10 * i, 10 * i, 10 * i, 0)]) for i in range(5, 12)]
    row, gs = groups(ac.nulls_block(), [], [(2, fr.INT8), (2, fr.INT8)], [])
    assert gs == [((100, 100), 6, []), ((None, None), 1, [])]


# ---- the invariants ----
def test_groups_combine_to_the_aggregates_cell():
    cases = [(ac.range_block(), ac.ATTS, ac.RANGE_KEYS, [(1, fr.INT2)], ac.COLS4),
             (ac.nulls_block(), ac.ATTS, [], [(4, fr.INT4), (2, fr.INT8)], [(6, fr.INT8), (2, fr.INT8)]),
             (ac.short_block(), ac.ATTS, [], [(4, fr.INT4)], [(6, fr.INT8), (1, fr.INT2)]),
             (ac.damaged_block()[0], ac.ATTS, fc.WALK, [(1, fr.INT2)], [(6, fr.INT8)]),
             (gc.order_block(), gc.ORDER_ATTS, [], [(2, fr.INT4), (3, fr.INT2)], [(1, fr.INT8), (4, fr.INT8)]),
             (gc.nulls_block(), gc.NULL_ATTS, [], gc.NULL_BY2, [(3, fr.INT8), (1, fr.INT4)]),
             (gc.turn_block("runs3", 290), gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS),
             (gc.turn_block("alternate", 129, True), gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS)]
    cases += [(blk, ac.EXT_ATTS, [], [(3, fr.INT2)], ac.EXT_COLS) for _, blk in ac.extremes_blocks()]
    for block, atts, keys, by, cols in cases:
        row, gs = gr.group_block(block, atts, keys, by, cols)
        # the walk of the aggregate goes as far as the group columns too when they ride as aggregate columns
        arow, acells = ar.agg_block(block, atts, keys, list(cols) + list(by))
        assert row == arow and sum(g[1] for g in gs) == row[2]
        for j in range(len(cols)):
            c = acells[j]
            assert gr.combine_block(gs, j) == (c[0], c[1], c[2], (c[4] << 64) + c[3]), (by, cols, j)
        assert [g[0] for g in gs] == sorted({g[0] for g in gs}, key=gr.order_key)


def test_descriptor_rules():
    for name, atts, keys, by, cols, flags, patch, ok in gc.descriptors():
        assert gc.ref_ok(gr, atts, keys, by, cols, flags, patch) == ok, name


# ---- the walk, through a codec double ----
@pytest.fixture()
def HG():
    import group_double
    L = host.lib()
    dbl = group_double.GroupingDouble()
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


ATTS3 = [(4, 4), (2, 2), (8, 8)]                        # (rowid int4, g int2, x int8)
BY, COLS = [(2, fr.INT2)], [(3, fr.INT8), (1, fr.INT4)]


def _relation(L, oracle, nblocks=9):
    """nblocks chains of 40 tuples (rowid, g = rowid % 3 or NULL when rowid % 10 == 0, x = -3 rowid): even ones LZ4, odd ones
    zstd, xid 500 + k.  Returns (mem, rel, decoded blocks, first pages)"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws, firsts = [], []
    for k in range(nblocks):
        ids = [40 * k + i for i in range(1, 41)]
        raw = tc.build_block(B128, [tc.form_tuple(ATTS3, [r, None if r % 10 == 0 else r % 3, -3 * r]) for r in ids])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def _want_block(first, xid, raw, keys, by=BY, cols=COLS):
    row, gs = gr.group_block(raw, ATTS3, keys, by, cols or [])
    return ("block", first, xid, row[1], row[2], row[3], [(k, n, [(c[0], c[1], c[2], (c[4] << 64) + c[3]) for c in cs]) for k, n, cs in gs])


def test_group_scan_walk_through_a_double(HG, oracle):
    L, dbl, errors = HG
    mem, rel, raws, firsts = _relation(L, oracle)
    # behind the nine good chains: a chain that cannot be read, a stream the decoders reject between good ones, a good chain
    short_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 904, oracle.lz4_compress(raws[0], 1))
    dead_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 906, oracle.lz4_compress(raws[3], 1))
    tail_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 907, oracle.zstd_compress(raws[0], 1))
    page = L.cryo_memrel_page(mem, short_first)
    csize = struct.unpack_from("<I", C.string_at(page, 64), 40)[0]
    C.memmove(page + 40, struct.pack("<I", csize + 100000), 4)
    C.memset(L.cryo_memrel_page(mem, dead_first) + 48, 0xFF, 64)

    keys = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 250)]
    events, t = host.group_scan(rel, ATTS3, keys, BY, COLS)
    want = [_want_block(firsts[k], 500 + k, raws[k], keys) for k in range(9)]
    want += [("report", short_first, fetch_walk.CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED), ("report", dead_first, fr.STREAM, 0),
             _want_block(tail_first, 907, raws[0], keys)]
    assert events == want                                                 # groups and one xid per block, reports in order
    assert [g[0] for g in want[1][6]] == [(0,), (1,), (2,), (None,)] and want[0][6][-1][0] == (None,) and want[8][6] == []
    assert dbl.calls == [(host.COMP_LZ4, 6), (host.COMP_ZSTD, 5)]         # both methods in one relation: one call each
    blocks = [e for e in events if e[0] == "block"]
    ngroups = sum(len(e[6]) for e in blocks)
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"], t["groups"]) == \
        (12, 40 * 10, sum(e[4] for e in blocks), 0, 2, 2, ngroups)
    assert t["bytes_back"] == 11 * 32 + ngroups * (24 + 40 * 2)               # a row for the rejected stream too
    assert sum(n for e in blocks for _, n, _ in e[6]) == t["matches"]
    # without aggregate columns: a null descriptor and an empty one give records only
    for cols in (None, []):
        events, t2 = host.group_scan(rel, ATTS3, keys, BY, cols)
        assert [e for e in events if e[0] == "block"][:9] == [_want_block(firsts[k], 500 + k, raws[k], keys, BY, cols) for k in range(9)]
        assert t2["bytes_back"] == 11 * 32 + ngroups * 24 and t2["groups"] == ngroups
    # a frozen block is handed over with FrozenTransactionId, as the read path does
    L.cryo_memrel_set_frozen(mem, firsts[3], True)
    events, _ = host.group_scan(rel, ATTS3, keys, BY, COLS)
    assert [e[2] for e in events if e[0] == "block"][:5] == [500, 501, 502, 2, 504]
    # descriptors the codec refuses; null arguments
    with pytest.raises(host.GroupScanError) as e:
        host.group_scan(rel, ATTS3, keys, [(2, fr.INT4)], COLS)
    assert e.value.code == E_ARG and e.value.events == []
    with pytest.raises(host.GroupScanError) as e:
        host.group_scan(rel, ATTS3, keys, [], COLS)
    assert e.value.code == E_ARG
    f, r = codec.filter_desc(ATTS3, keys), codec.group_desc(BY)
    nb, nr = host.GROUP_BLOCK_FN(0), host.FETCH_REPORT_FN(0)
    assert L.cryo_group_scan(C.byref(rel), None, C.byref(r[0]), None, nb, nr, None, None) == E_ARG
    assert L.cryo_group_scan(C.byref(rel), C.byref(f[0]), None, None, nb, nr, None, None) == E_ARG
    assert L.cryo_group_scan(None, C.byref(f[0]), C.byref(r[0]), None, nb, nr, None, None) == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_group_scan_windows(HG, oracle):
    """the window lowered to 4 chains, then to the compressed bytes of about three: several codec calls, the same delivery"""
    L, dbl, _ = HG
    mem, rel, raws, firsts = _relation(L, oracle)
    keys = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 250)]
    whole, t0 = host.group_scan(rel, ATTS3, keys, BY, COLS)
    assert dbl.calls == [(host.COMP_LZ4, 5), (host.COMP_ZSTD, 4)] and t0["codec_calls"] == 2
    dbl.calls.clear()
    L.cryo_group_set_window(4, 0)
    got, t = host.group_scan(rel, ATTS3, keys, BY, COLS)
    assert got == whole and [e[1] for e in got] == firsts
    assert dbl.calls == [(host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 1)]
    assert t["codec_calls"] == 5
    assert {k: v for k, v in t.items() if k != "codec_calls"} == {k: v for k, v in t0.items() if k != "codec_calls"}
    dbl.calls.clear()
    csize = len(oracle.lz4_compress(raws[0], 1))
    L.cryo_group_set_window(0, 3 * csize + csize // 2)
    got, t = host.group_scan(rel, ATTS3, keys, BY, COLS)
    assert got == whole and t["codec_calls"] == len(dbl.calls) >= 3 and t["groups"] == t0["groups"]
    L.cryo_memrel_destroy(mem)


def test_without_a_group_table_the_scan_is_unsupported(HG, oracle):
    L, dbl, _ = HG
    mem, rel, raws, firsts = _relation(L, oracle, nblocks=2)
    L.cryo_host_set_group_ops(None)
    with pytest.raises(host.GroupScanError) as e:
        host.group_scan(rel, ATTS3, [], BY, COLS)
    assert e.value.code == E_UNSUPPORTED and e.value.events == [] and e.value.totals["blocks"] == 0
    L.cryo_memrel_destroy(mem)
