"""CPU tests of the projecting scan: the rules (tests/project_ref.py) on hand-made vectors (tests/project_cases.py) whose expected
records and rows are written out there, the row-layout rule, the descriptor rules, and cryo_project_scan (host/project.c) walking
a mini-AM relation through the test build, with a codec double (tests/project_double.py) whose project_blocks decodes with the
oracle and answers by the rules."""
import ctypes as C
import itertools
import struct

import numpy as np
import pytest

import fetch_walk
import filter_ref as fr
import project_cases as pc
import project_ref as pr
import tuple_craft as tc
from pg_cryogen_amd import codec, host

B128 = 131072
E_UNSUPPORTED, E_ARG, E_DSTSIZE = -6, -1, -5


# ---- the reference on hand-made vectors ----
@pytest.mark.parametrize("case", pc.cases(), ids=[c[0] for c in pc.cases()])
def test_reference_reproduces_the_hand_made_cases(case):
    name, B, atts, block, keys, cols, expected = case
    assert pr.desc_ok(atts, keys, cols)
    assert pr.project_block(block, atts, keys, cols) == (0, int(block[:4].view("<u4")[0] - 8) // 8, expected)
    # the call's table, records and rows say the same through rows_of
    table, recs, rows, (tw, tr) = pr.project_call([block], atts, keys, cols)
    assert (tw, tr) == (sum(1 for e in expected if e[1] == 0), len(expected)) and rows.shape == (tw, pr.row_layout(atts, cols)[1])
    assert pr.rows_of(table, recs, rows, 0) == [(p, nulls, row) for p, st, nulls, row in expected if st == 0]
    assert [(int(r["pos"]), int(r["status"]), int(r["nulls"])) for r in recs] == [e[:3] for e in expected]


def test_the_filter_passes_what_the_projection_cuts():
    """the documented difference: the tuple cut before the timestamp matches the id key in the filter"""
    name, B, atts, block, keys, cols, expected = [c for c in pc.cases() if c[0] == "cut before a projected column"][0]
    status, n, recs = fr.filter_block(block, atts, keys)
    assert status == 0 and [r[:2] for r in recs] == [(1, 0), (2, 0), (3, 0)] and expected[1][:2] == (2, pc.TUPLE)


def test_stream_and_header_blocks_have_nothing_and_keep_the_count():
    good = [c for c in pc.cases() if c[0] == "width mix, range on id"][0]
    _, B, atts, block, keys, cols, expected = good
    table, recs, rows, tot = pr.project_call([block, None, block, pc.header_block(), block], atts, keys, cols)
    assert [int(s) for s in table["status"]] == [0, 1, 0, 2, 0] and [int(x) for x in table["n_items"]] == [5, 0, 5, 0, 5]
    assert [int(x) for x in table["row_first"]] == [0, 3, 3, 6, 6] and [int(x) for x in table["rec_first"]] == [0, 3, 3, 6, 6]
    assert tot == (9, 9) and [bytes(r) for r in rows] == [e[3] for e in expected] * 3


def test_turn_blocks():
    for n in pc.TURN_SIZES:
        blk = pc.turn_block(n)
        st, items, recs = pr.project_block(blk, pc.TURN_ATTS, pc.TURN_KEYS["all"], pc.TURN_COLS)
        assert (st, items) == (0, n)
        assert recs == [(p, 0, 0, struct.pack("<b3xi", p % 251 - 125, p)) for p in range(1, n + 1)]
        assert pr.project_block(blk, pc.TURN_ATTS, pc.TURN_KEYS["none"], pc.TURN_COLS) == (0, n, [])
        st, items, recs = pr.project_block(pc.turn_block_alternating(n), pc.TURN_ATTS, pc.ALTERNATING_KEYS, pc.TURN_COLS)
        assert recs == [(p, 0, 0, struct.pack("<b3xi", p % 100, p)) for p in range(1, n + 1, 2)]


# ---- the row layout ----
def _layout_by_hand(widths):
    """the rule once more, with integer arithmetic spelled differently from the reference's and the library's"""
    at, offsets = 0, []
    for w in widths:
        while at % w:
            at += 1
        offsets.append(at)
        at += w
    while at % 8:
        at += 1
    return offsets, at


def test_row_layout_on_all_width_triples_and_the_extremes():
    for widths in itertools.product(pr.WIDTHS, repeat=3):
        atts = [(w, w) for w in widths]
        want = _layout_by_hand(widths)
        assert pr.row_layout(atts, [1, 2, 3]) == want and codec.project_row_layout(atts, [1, 2, 3]) == want, widths
        assert 8 <= want[1] <= 24 and want[1] % 8 == 0
    assert pr.row_layout([(1, 1)], [1] * 8) == (list(range(8)), 8) == codec.project_row_layout([(1, 1)], [1] * 8)
    assert pr.row_layout([(8, 8)], [1] * 8) == (list(range(0, 64, 8)), 64) == codec.project_row_layout([(8, 8)], [1] * 8)
    assert pr.row_layout([(1, 1), (8, 8)], [1, 2, 1, 2]) == ([0, 8, 16, 24], 32)
    # a few written out
    assert pr.row_layout([(1, 1), (2, 2), (4, 4)], [1, 2, 3]) == ([0, 2, 4], 8)
    assert pr.row_layout([(4, 4), (1, 1), (8, 8)], [1, 2, 3]) == ([0, 4, 8], 16)
    assert pr.row_layout([(8, 8), (1, 1), (2, 2)], [1, 2, 3]) == ([0, 8, 10], 16)


def test_descriptor_rules():
    for name, atts, keys, cols, flags, patch, ok in pc.descriptors():
        assert pc.ref_ok(pr, atts, keys, cols, flags, patch) == ok, name


# ---- the walk, through a codec double ----
@pytest.fixture()
def HP():
    import project_double
    L = host.lib()
    dbl = project_double.ProjectingDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_project_ops(C.byref(dbl.project_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_project_set_window(0, 0)
    L.cryo_cache_shutdown()
    L.cryo_host_set_project_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


ATTS4 = [(4, 4), (-1, 4), (2, 2), (8, 8)]                 # (rowid int4, pad text, g int2, x float8 bits)
COLS = [4, 3, 1]                                          # widths 8, 2, 4: offsets 0, 8, 12; 16 bytes
KEYS = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 250)]


def _relation(L, oracle, nblocks=9):
    """nblocks chains of 40 tuples (rowid, "t" x (rowid % 7), g = rowid % 3 or NULL when rowid % 10 == 0, x = the bits of -3.0 *
    rowid): even ones LZ4, odd ones zstd, xid 500 + k.  Returns (mem, rel, decoded blocks, first pages)"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4343, C.byref(rel))
    raws, firsts = [], []
    for k in range(nblocks):
        ids = [40 * k + i for i in range(1, 41)]
        raw = tc.build_block(B128, [tc.form_tuple(ATTS4, [r, b"t" * (r % 7), None if r % 10 == 0 else r % 3,
                                                          struct.unpack("<q", struct.pack("<d", -3.0 * r))[0]]) for r in ids])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def _want_rows(first, xid, raw, keys=KEYS, cols=COLS):
    st, n, recs = pr.project_block(raw, ATTS4, keys, cols)
    return [("row", first, pos, xid, nulls, row) for pos, s, nulls, row in recs if s == 0]


def test_project_scan_walk_through_a_double(HP, oracle):
    L, dbl, errors = HP
    mem, rel, raws, firsts = _relation(L, oracle)
    # behind the nine good chains: a chain that cannot be read, a stream the decoders reject, a block with a bad item, a good chain
    short_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 904, oracle.lz4_compress(raws[0], 1))
    dead_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 906, oracle.lz4_compress(raws[3], 1))
    dented = raws[1].copy()
    dented[8 + 8 * 4 + 4:8 + 8 * 4 + 8] = 0                                 # item 5 (rowid 45): len 0
    dent_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 908, oracle.zstd_compress(dented, 1))
    tail_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 907, oracle.zstd_compress(raws[0], 1))
    page = L.cryo_memrel_page(mem, short_first)
    csize = struct.unpack_from("<I", C.string_at(page, 64), 40)[0]
    C.memmove(page + 40, struct.pack("<I", csize + 100000), 4)
    C.memset(L.cryo_memrel_page(mem, dead_first) + 48, 0xFF, 64)

    events, t = host.project_scan(rel, ATTS4, KEYS, COLS)
    want = []
    for k in range(9):
        want += _want_rows(firsts[k], 500 + k, raws[k])
    want += [("report", short_first, fetch_walk.CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED), ("report", dead_first, fr.STREAM, 0)]
    dent_rows = _want_rows(dent_first, 908, dented)
    want += [r for r in dent_rows if r[2] < 5] + [("report", dent_first, fr.ITEM, 5)] + [r for r in dent_rows if r[2] > 5]
    want += _want_rows(tail_first, 907, raws[0])
    assert events == want                                                 # rows in block, then position order; reports between
    rows = [e for e in events if e[0] == "row"]
    # rowids 30 .. 249 of the nine blocks, 41 .. 80 less 45 of the dented one, 30 .. 40 of the tail
    assert len(rows) == 220 + 39 + 11 and all(len(e[5]) == 16 for e in rows)
    assert rows[0][1:5] == (firsts[0], 30, 500, 0b010) and rows[0][5] == struct.pack("<dh2xi", -90.0, 0, 30)
    assert rows[1][4] == 0 and rows[1][5] == struct.pack("<dh2xi", -93.0, 1, 31)
    assert dbl.calls == [(host.COMP_LZ4, 6), (host.COMP_ZSTD, 6)]         # both methods in one relation: one call each
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"]) == (13, 40 * 11, len(rows), 1, 3, 2)
    assert t["bytes_back"] == 12 * 32 + (len(rows) + 1) * 8 + len(rows) * 16  # a table row for the rejected stream too
    # a frozen block is handed over with FrozenTransactionId, as the read path does
    L.cryo_memrel_set_frozen(mem, firsts[3], True)
    events, _ = host.project_scan(rel, ATTS4, KEYS, COLS)
    assert sorted({e[3] for e in events if e[0] == "row" and e[1] in firsts[:5]}) == [2, 500, 501, 502, 504]
    # descriptors the codec refuses; null arguments
    for cols in ([2], [], [5], [1] * 9):
        with pytest.raises(host.ProjectScanError) as e:
            host.project_scan(rel, ATTS4, KEYS, cols)
        assert e.value.code == E_ARG and e.value.events == [], cols
    f, p = codec.filter_desc(ATTS4, KEYS), codec.project_desc(COLS)
    nw, nr = host.PROJECT_ROW_FN(0), host.FETCH_REPORT_FN(0)
    assert L.cryo_project_scan(C.byref(rel), None, C.byref(p[0]), nw, nr, None, None) == E_ARG
    assert L.cryo_project_scan(C.byref(rel), C.byref(f[0]), None, nw, nr, None, None) == E_ARG
    assert L.cryo_project_scan(None, C.byref(f[0]), C.byref(p[0]), nw, nr, None, None) == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_project_scan_windows(HP, oracle):
    """the window lowered to 4 chains (three windows), then to the compressed bytes of about three: several codec calls, the same
    delivery; then a call the double refuses with CRYO_E_DSTSIZE stops the walk and what was delivered stands"""
    L, dbl, _ = HP
    mem, rel, raws, firsts = _relation(L, oracle)
    whole, t0 = host.project_scan(rel, ATTS4, KEYS, COLS)
    assert dbl.calls == [(host.COMP_LZ4, 5), (host.COMP_ZSTD, 4)] and t0["codec_calls"] == 2
    dbl.calls.clear()
    L.cryo_project_set_window(4, 0)
    got, t = host.project_scan(rel, ATTS4, KEYS, COLS)
    assert got == whole and sorted({e[1] for e in got}) == firsts[:7]      # rowids 30 .. 249 lie in the first seven blocks
    assert dbl.calls == [(host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 1)]
    assert t["codec_calls"] == 5 and t["matches"] == 220 == len(got)
    assert {k: v for k, v in t.items() if k != "codec_calls"} == {k: v for k, v in t0.items() if k != "codec_calls"}
    # with rowid >= 100 the first window's calls bring 21 and 40 rows, the second window's first call needs 80: refused.  The first
    # window's rows stand, the totals say how far the walk got
    dbl.calls.clear()
    dbl.row_cap_limit = 79
    late = [(1, fr.INT4, fr.GE, 100)]
    with pytest.raises(host.ProjectScanError) as e:
        host.project_scan(rel, ATTS4, late, COLS)
    assert e.value.code == E_DSTSIZE
    want = []
    for k in range(4):
        want += _want_rows(firsts[k], 500 + k, raws[k], late)
    assert e.value.events == want and len(want) == 21 + 40
    assert e.value.totals["codec_calls"] == 3 and e.value.totals["matches"] == 61 and e.value.totals["blocks"] == 8
    assert dbl.calls == [(host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 2)]     # no call after the refused one
    dbl.row_cap_limit = None
    dbl.calls.clear()
    csize = len(oracle.lz4_compress(raws[0], 1))
    L.cryo_project_set_window(0, 3 * csize + csize // 2)
    got, t = host.project_scan(rel, ATTS4, KEYS, COLS)
    assert got == whole and t["codec_calls"] == len(dbl.calls) >= 3 and t["matches"] == t0["matches"]
    L.cryo_memrel_destroy(mem)


def test_without_a_project_table_the_scan_is_unsupported(HP, oracle):
    L, dbl, _ = HP
    mem, rel, raws, firsts = _relation(L, oracle, nblocks=2)
    L.cryo_host_set_project_ops(None)
    with pytest.raises(host.ProjectScanError) as e:
        host.project_scan(rel, ATTS4, [], COLS)
    assert e.value.code == E_UNSUPPORTED and e.value.events == [] and e.value.totals["blocks"] == 0
    L.cryo_memrel_destroy(mem)
