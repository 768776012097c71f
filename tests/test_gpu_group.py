"""GPU tests of the grouped scan (cryo_codec_group_batch, cryo_codec_group_blocks, cryo_multi_group_blocks).

Every row, record and cell is compared with tests/group_ref.py, the numpy statement of the rules in include/cryo_codec.h, applied
to the ORACLE's decode of each stream.  The device buffers are filled with a sentinel before every call: nothing beyond the rows,
the records and the cells of the call may be written."""
import ctypes as C

import numpy as np
import pytest

import agg_cases as ac
import agg_ref as ar
import filter_cases as fc
import filter_ref as fr
import group_cases as gc
import group_ref as gr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SYNTH_ATTS = [(4, 4), (-1, 4)]
ROWID = [(1, fr.INT4)]
METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def grp(codec):
    yield codec
    for opt, v in ((cc.OPT_WORKSPACE_MAX_BYTES, 0), (cc.OPT_POOL_BYTES, 0)):
        codec.set_option(opt, v)


def oracle_encode(oracle, method, raw):
    return oracle.lz4_compress(raw, 1) if method == METHOD_LZ4 else oracle.zstd_compress(raw, 1)


def pack_streams(comps):
    n = len(comps)
    sizes = np.array([len(c) for c in comps], np.uint32)
    offs = np.zeros(n, np.uint64)
    at = 0
    for i, c in enumerate(comps):
        offs[i] = at
        at += (len(c) + 15) & ~15
    packed = np.zeros(max(at, 16), np.uint8)
    for i, c in enumerate(comps):
        packed[int(offs[i]):int(offs[i]) + len(c)] = np.asarray(c, np.uint8)
    return packed, offs, sizes


def group_batch(codec, method, comps, B, atts, keys, by, cols, group_cap=None):
    """cryo_codec_group_batch on device copies of the streams and of the descriptors: (rows, records, cells of shape (groups,
    ncols), total).  Rows, records and cells are filled with SENTINEL before the call; the 64 bytes behind each -- and, when
    group_cap cuts the writing off, everything from group_cap on -- must still hold it afterwards.  cols None: no aggregate
    array and no cell buffer at all"""
    n, nc = len(comps), len(cols or [])
    cap = 290 * n if group_cap is None else group_cap
    packed, offs, sizes = pack_streams(comps)
    _, a, k = cc.filter_desc(atts, keys)
    _, b = cc.group_desc(by)
    _, g = cc.agg_desc(cols or [])
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(a.nbytes), codec.alloc(k.nbytes),
            codec.alloc(b.nbytes), codec.alloc(g.nbytes), codec.alloc(32 * n + 64), codec.alloc(24 * cap + 64),
            codec.alloc(40 * cap * nc + 64), codec.alloc(8)]
    d_src, d_off, d_sz, d_atts, d_keys, d_by, d_cols, d_rows, d_recs, d_cells, d_total = bufs
    try:
        for d, h in ((d_src, packed), (d_off, offs), (d_sz, sizes), (d_atts, a), (d_keys, k), (d_by, b), (d_cols, g)):
            d.upload(h)
        for d in (d_rows, d_recs, d_cells, d_total):
            d.memset(SENTINEL)
        codec.group_batch(method, d_src, d_off, d_sz, B, n, len(atts), d_atts, len(keys), d_keys if keys else None, len(by), d_by,
                          nc, d_cols if nc else None, d_rows, d_recs, cap, d_cells if cols is not None else None, d_total)
        codec.sync()
        rows, recs, cells = d_rows.download(), d_recs.download(), d_cells.download()
        total = int(d_total.download().view("<u8")[0])
        wrote = min(total, cap)
        assert (rows[32 * n:] == SENTINEL).all(), "a byte beyond the rows was written"
        assert (recs[24 * wrote:] == SENTINEL).all(), "a byte beyond the records was written"
        assert (cells[40 * wrote * nc:] == SENTINEL).all(), "a byte beyond the cells was written"
        return (rows[:32 * n].view(cc.GROUP_BLOCK).copy(), recs[:24 * wrote].view(cc.GROUP_REC).copy(),
                cells[:40 * wrote * nc].view(cc.AGG_CELL).reshape(wrote, nc).copy(), total)
    finally:
        for x in bufs:
            x.free()


def host_call(codec, method, comps, B, atts, keys, by, cols, group_cap=None):
    return codec.group_blocks(method, comps, B, cc.filter_desc(atts, keys), cc.group_desc(by),
                              None if cols is None else cc.agg_desc(cols), group_cap)


def same(got, want, what=""):
    rows, recs, cells, total = got
    erows, erecs, ecells, etotal = want
    assert total == etotal, (what, total, etotal)
    assert rows.shape == erows.shape and recs.shape == erecs.shape and cells.shape == ecells.shape, \
        (what, rows.shape, erows.shape, recs.shape, erecs.shape, cells.shape, ecells.shape)
    for f in erows.dtype.names:
        bad = np.flatnonzero(rows[f] != erows[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(rows[i]), tuple(erows[i])) for i in bad[:5]])
    for f in erecs.dtype.names:
        bad = np.argwhere(recs[f] != erecs[f])
        assert bad.size == 0, (what, f, [(int(i[0]), recs[i[0]], erecs[i[0]]) for i in bad[:5]])
    for f in ecells.dtype.names:
        bad = np.argwhere(cells[f] != ecells[f])
        assert bad.size == 0, (what, f, [(tuple(ij), tuple(cells[tuple(ij)]), tuple(ecells[tuple(ij)])) for ij in bad[:5]])


def both(codec, oracle, blocks, B, atts, keys, by, cols, what, methods=METHODS):
    """device buffers and host buffers, on the oracle's streams of `blocks`, against group_ref; returns the expectation"""
    want = gr.group_call(blocks, atts, keys, by, cols or [])
    for method in methods:
        comps = [oracle_encode(oracle, method, b) for b in blocks]
        same(group_batch(codec, method, comps, B, atts, keys, by, cols), want, (what, method))
        same(host_call(codec, method, comps, B, atts, keys, by, cols), want, (what, method, "host buffers"))
    return want


# ---- the turns of a wave: 64 matches each ----
@pytest.mark.parametrize("pattern", gc.PATTERNS)
def test_turn_boundaries(grp, oracle, pattern):
    """0, 1, 63, 64, 65, 128, 129 and 290 matches: in one group, all distinct, two groups alternating, runs of three across every
    64-boundary; then with tuples the key rejects and damaged ones in between, so that a match's number is not its position"""
    blocks = [gc.turn_block(pattern, m) for m in gc.TURN_SIZES]
    rows, recs, cells, total = both(grp, oracle, blocks, gc.TURN_B, gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, pattern)
    assert rows["n_match"].tolist() == list(gc.TURN_SIZES)
    want_groups = {"one": [min(m, 1) for m in gc.TURN_SIZES], "distinct": list(gc.TURN_SIZES),
                   "alternate": [min(m, 2) for m in gc.TURN_SIZES], "runs3": [len(set(gc.runs3(m))) for m in gc.TURN_SIZES]}[pattern]
    assert rows["n_groups"].tolist() == want_groups and total == sum(want_groups)
    blocks = [gc.turn_block(pattern, m, True) for m in gc.INTERLEAVED_SIZES]
    rows, _, _, _ = both(grp, oracle, blocks, gc.TURN_B, gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, (pattern, "interleaved"))
    assert rows["n_match"].tolist() == list(gc.INTERLEAVED_SIZES) and rows["n_bad"].tolist() == [m // 7 for m in gc.INTERLEAVED_SIZES]
    assert rows["n_items"].tolist() == [m + m // 2 + m // 7 for m in gc.INTERLEAVED_SIZES]


# ---- order and sign ----
def test_order_and_sign(grp, oracle):
    blocks = [gc.order_block(), gc.second_differs_block()]
    rows, recs, _, _ = both(grp, oracle, blocks, gc.ORDER_B, gc.ORDER_ATTS, [], [(1, fr.INT8)], [(4, fr.INT8)], "int8 keys")
    assert recs["key"][:5, 0].tolist() == gc.ORDER_VALUES and recs["n_rows"][:5].tolist() == [6] * 5
    rows, recs, _, _ = both(grp, oracle, blocks, gc.ORDER_B, gc.ORDER_ATTS, [], [(2, fr.INT4), (3, fr.INT2)], [(4, fr.INT8)], "int4, int2")
    assert recs["key"][0].tolist() == [-(1 << 31), -(1 << 15)] and rows["n_groups"][0] == 12
    rows, recs, _, _ = both(grp, oracle, blocks, gc.ORDER_B, gc.ORDER_ATTS, [], [(1, fr.INT8), (3, fr.INT2)], [(4, fr.INT8)], "wide, narrow")
    g0 = int(rows["first_group"][1])
    assert recs["key"][g0:].tolist() == [[ac.I64_MAX, v] for v in (-32768, -3, 0, 3, 32767)]
    assert recs["n_rows"][g0:].tolist() == [2, 2, 2, 4, 2]


# ---- NULLs ----
def test_nulls(grp, oracle):
    blocks = [gc.nulls_block()]
    rows, recs, cells, _ = both(grp, oracle, blocks, gc.ORDER_B, gc.NULL_ATTS, [], gc.NULL_BY2, [(3, fr.INT8)], "two columns")
    assert [(k.tolist(), int(n)) for k, n in zip(recs["key"], recs["nulls"])] == \
        [([4, 9], 0), ([5, 5], 0), ([5, 0], 2), ([0, 5], 1), ([0, 0], 3)]
    assert recs["n_rows"].tolist() == [1, 2, 3, 2, 2] and cells["n"][:, 0].tolist() == [1, 1, 1, 2, 0]
    assert tuple(cells[4, 0]) == (0, 0, 0, 0, 0)                                   # every row NULL there: the cell is zero
    both(grp, oracle, blocks, gc.ORDER_B, gc.NULL_ATTS, [], [(2, fr.INT4)], [(3, fr.INT8), (1, fr.INT4)], "one column")
    both(grp, oracle, blocks, gc.ORDER_B, gc.NULL_ATTS, [(1, 0, fr.ISNULL, 0)], gc.NULL_BY2, [(3, fr.INT8)], "ISNULL on a group column")
    both(grp, oracle, [ac.nulls_block(), ac.short_block(), ac.all_null_block()], ac.B, ac.ATTS, [], [(4, fr.INT4), (6, fr.INT8)],
         [(2, fr.INT8)], "the aggregate's blocks")


# ---- sums beyond 64 bits ----
def test_extremes(grp, oracle):
    blocks = [b for _, b in ac.extremes_blocks()]
    rows, recs, cells, _ = both(grp, oracle, blocks, ac.EXT_B, ac.EXT_ATTS, [], [(2, fr.INT4)], ac.EXT_COLS, "extremes")
    assert rows["n_groups"].tolist() == [1, 1, 2] and recs["n_rows"].tolist() == [290, 290, 145, 145]
    assert [ar.total_of(c) for c in cells[:, 0]] == [290 * ac.I64_MIN, 290 * ac.I64_MAX, 145 * ac.I64_MIN, 145 * ac.I64_MAX]
    assert cells["sum_hi"][:2, 0].tolist() == [-145, 144]                          # the sums need the high word


# ---- no aggregate column; columns in several roles ----
def test_without_aggregate_columns(grp, oracle):
    blocks = [gc.order_block(), gc.turn_block("runs3", 129)]
    for cols in ([], None):
        for method in METHODS:
            comps = [oracle_encode(oracle, method, b) for b in blocks]
            want = gr.group_call(blocks, gc.ORDER_ATTS[:2], [], [(1, fr.INT8)], [])
            same(group_batch(grp, method, comps, gc.ORDER_B, gc.ORDER_ATTS[:2], [], [(1, fr.INT8)], cols), want, (cols, method))
            same(host_call(grp, method, comps, gc.ORDER_B, gc.ORDER_ATTS[:2], [], [(1, fr.INT8)], cols), want, (cols, method, "host"))


def test_columns_in_several_roles(grp, oracle):
    blocks = [ac.range_block(), ac.nulls_block(), ac.short_block()]
    both(grp, oracle, blocks, ac.B, ac.ATTS, ac.RANGE_KEYS, [(4, fr.INT4)], [(4, fr.INT4), (4, fr.INT4)], "key, group, aggregate")
    rows, recs, _, _ = both(grp, oracle, blocks, ac.B, ac.ATTS, [], [(2, fr.INT8), (2, fr.INT8)], ac.COLS4, "a group column twice")
    assert (recs["key"][:, 0] == recs["key"][:, 1]).all() and set(recs["nulls"].tolist()) <= {0, 3}


# ---- the walk goes as far as the last group column ----
def test_walk_length(grp, oracle):
    blk = ac.cut_block()
    k1 = [(1, fr.INT2, fr.EQ, 5)]
    rows, recs, _, _ = both(grp, oracle, [blk, ac.range_block()], ac.B, ac.ATTS, k1, [(6, fr.INT8)], [], "column 6 beyond the key")
    assert tuple(rows[0])[:5] == (0, 3, 2, 1, 1) and recs["n_rows"][0] == 2
    rows, _, _, _ = both(grp, oracle, [blk], ac.B, ac.ATTS, k1, [(4, fr.INT4)], [], "column 4 still fits")
    assert tuple(rows[0])[:5] == (0, 3, 3, 0, 1)
    for method in METHODS:                                                # the filter, with the same keys, calls the cut tuple a match
        table, _, _, _ = grp.filter_blocks(method, [oracle_encode(oracle, method, blk)], ac.B, cc.filter_desc(ac.ATTS, k1))
        assert (table["n_match"][0], table["n_bad"][0]) == (3, 0)


# ---- damage ----
def test_damage(grp, oracle):
    blk, bad = ac.damaged_block()
    blocks = [blk, ac.bad_item_block(), blk]
    rows, recs, cells, _ = both(grp, oracle, blocks, ac.B, ac.ATTS, fc.WALK, [(4, fr.INT4)], [(6, fr.INT8)], "damaged")
    assert rows["n_bad"].tolist() == [len(bad), 1, len(bad)] and rows["n_match"].tolist() == [11, 5, 11]
    assert recs["n_rows"].tolist() == [11, 5, 11]                                  # counted, in no group
    good = ac.range_block()
    blocks = [good, None, ac.header_block(), good, None, good]
    want = gr.group_call(blocks, ac.ATTS, ac.RANGE_KEYS, [(1, fr.INT2)], ac.COLS4)
    assert want[0]["status"].tolist() == [0, fr.STREAM, fr.HEADER, 0, fr.STREAM, 0]
    assert want[0]["n_groups"].tolist() == [7, 0, 0, 7, 0, 7] and want[0]["first_group"].tolist() == [0, 7, 7, 7, 14, 14]
    for method in METHODS:
        comps = [oracle_encode(oracle, method, good if b is None else b) for b in blocks]
        comps[1] = comps[1][:len(comps[1]) - 7]
        comps[4] = comps[4][:len(comps[4]) // 2]
        assert [ar.decode(oracle, method, c, ac.B) is None for c in comps] == [b is None for b in blocks]
        same(group_batch(grp, method, comps, ac.B, ac.ATTS, ac.RANGE_KEYS, [(1, fr.INT2)], ac.COLS4), want, method)
        same(host_call(grp, method, comps, ac.B, ac.ATTS, ac.RANGE_KEYS, [(1, fr.INT2)], ac.COLS4), want, (method, "host"))


# ---- chunks ----
@pytest.fixture(scope="module")
def sixty_four(oracle):
    B = 131072
    raws = [oracle.synth(55, k, B, (1, 0, 2, 1, 0)[k % 5]) for k in range(64)]
    keys = [(1, fr.INT4, fr.GE, 1000), (1, fr.INT4, fr.LT, 9000)]
    return B, raws, keys


@pytest.mark.parametrize("method", METHODS)
def test_chunks_give_the_same_results(grp, oracle, sixty_four, method):
    """grouped by the rowid column every match is a group of its own: up to 290 per block, the side area's whole row"""
    B, raws, keys = sixty_four
    comps = [oracle_encode(oracle, method, r) for r in raws]
    comps[17] = comps[17][:len(comps[17]) - 9]
    blocks = [None if i == 17 else r for i, r in enumerate(raws)]
    want = gr.group_call(blocks, SYNTH_ATTS, keys, ROWID, ROWID)
    assert want[0]["n_groups"].max() == 290 and want[0]["n_groups"][17] == 0 and want[3] > 5000
    whole = group_batch(grp, method, comps, B, SYNTH_ATTS, keys, ROWID, ROWID)
    same(whole, want, "one chunk")
    grp.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 2 << 20)                   # at most 15 decoded blocks of 128 KiB fit: five chunks or more
    got = group_batch(grp, method, comps, B, SYNTH_ATTS, keys, ROWID, ROWID)
    same(got, want, "small budget")
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], whole[:3]))
    same(host_call(grp, method, comps, B, SYNTH_ATTS, keys, ROWID, ROWID), want, "host buffers, small budget")
    grp.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- more than 256 blocks in one chunk: the second tile of the offset scan ----
TILE_B, TILE_N, TILE_CUT = 4096, 330, 262


@pytest.fixture(scope="module")
def two_tiles(oracle):
    """ten generator blocks of 4 KiB, repeated to 330: at this size the WIDE and RANDOM blocks hold 290 bad items each, the others
    56 and 102 tuples or none; the keys pass some tuples of blocks 1 and 2 and none of blocks 6 and 7.  Block 262 stands for a
    stream the decoders reject.  Grouped by the rowid column every match is a group.  (raws, keys, the reference's result: one
    for both methods)"""
    raws = [oracle.synth(77, k, TILE_B, k % 5) for k in range(10)]
    keys = [(1, fr.INT4, fr.GE, 311), (1, fr.INT4, fr.LT, 650)]
    blocks = [None if i == TILE_CUT else raws[i % 10] for i in range(TILE_N)]
    return raws, keys, gr.group_call(blocks, SYNTH_ATTS, keys, ROWID, ROWID)


@pytest.mark.parametrize("method", METHODS)
def test_second_tile_of_the_offset_scan(grp, oracle, two_tiles, method):
    """330 blocks are one chunk under the default budget, so k_group_offsets runs two tiles of 256 and 74 rows: the running
    total carried into the second tile and the sums inside it, with a rejected stream, a block without a match and partly
    matching blocks beyond row 256; device buffers and host buffers against the reference, nothing left out"""
    raws, keys, want = two_tiles
    enc = [oracle_encode(oracle, method, r) for r in raws]
    comps = [enc[i % 10] for i in range(TILE_N)]
    comps[TILE_CUT] = comps[TILE_CUT][:len(comps[TILE_CUT]) - 9]
    assert all(np.array_equal(ar.decode(oracle, method, c, TILE_B), r) for c, r in zip(enc, raws))
    assert ar.decode(oracle, method, comps[TILE_CUT], TILE_B) is None
    t = want[0]
    assert t["status"][TILE_CUT] == fr.STREAM and set(t["status"].tolist()) == {0, fr.STREAM}
    assert (t["n_items"][256], t["n_match"][256], t["n_groups"][256]) == (56, 0, 0)   # tuples, and none of them passes
    assert 0 < t["n_match"][261] < t["n_items"][261] and 0 < t["n_match"][272] < t["n_items"][272]
    assert t["n_bad"][255] == 290 and t["first_group"][256] > 0 and want[3] == int(t["n_match"].sum())
    for what, got in (("device buffers", group_batch(grp, method, comps, TILE_B, SYNTH_ATTS, keys, ROWID, ROWID)),
                      ("host buffers", host_call(grp, method, comps, TILE_B, SYNTH_ATTS, keys, ROWID, ROWID))):
        same(got, want, (method, what))
        # every row starts where the one before ended, across row 256 as anywhere else
        g = got[0]
        assert g["first_group"][0] == 0 and (g["first_group"][1:] == g["first_group"][:-1] + g["n_groups"][:-1]).all(), (method, what)
        assert got[3] == int(g["first_group"][-1]) + int(g["n_groups"][-1]), (method, what)


# ---- caps ----
def test_caps(grp, oracle):
    blocks = [gc.turn_block("distinct", 65), gc.turn_block("alternate", 64), gc.turn_block("runs3", 129)]
    want = gr.group_call(blocks, gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS)
    need = want[3]
    assert need == 65 + 2 + 43
    for method in METHODS:
        comps = [oracle_encode(oracle, method, b) for b in blocks]
        same(host_call(grp, method, comps, gc.TURN_B, gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, need), want, "exactly the need")
        for cap in (need - 1, 66, 0):
            with pytest.raises(CryoError) as e:
                host_call(grp, method, comps, gc.TURN_B, gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, cap)
            assert e.value.code == cc.E_DSTSIZE, cap
            rows, recs, cells, total = group_batch(grp, method, comps, gc.TURN_B, gc.GX_ATTS, gc.GX_KEYS, gc.GX_BY, gc.GX_COLS, cap)
            assert total == need and recs.shape[0] == cap                  # the full need; the sentinel from group_cap on (group_batch)
            same((rows, recs, cells, need), (want[0], want[1][:cap], want[2][:cap], need), ("cut at", cap))


# ---- counters ----
@pytest.mark.parametrize("method", METHODS)
def test_transfer_and_codec_counters(grp, oracle, sixty_four, method):
    B, raws, keys = sixty_four
    raws = raws[:24]
    comps = [oracle_encode(oracle, method, r) for r in raws]
    grp.set_option(cc.OPT_POOL_BYTES, 8 * B)
    for budget in (0, 4 << 20):
        grp.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
        for cols in (ROWID + ROWID, []):
            want = gr.group_call(raws, SYNTH_ATTS, keys, ROWID, cols)
            before_t, before_c = grp.transfer_counters(), grp.counters()
            got = host_call(grp, method, comps, B, SYNTH_ATTS, keys, ROWID, cols)
            after_t, after_c = grp.transfer_counters(), grp.counters()
            same(got, want)
            assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 32 * 24 + (24 + 40 * len(cols)) * want[3]
            for k in ("pool_hits", "pool_misses", "pool_blocks"):
                assert after_t[k] == before_t[k], k
            assert after_c == before_c
    grp.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
    grp.set_option(cc.OPT_POOL_BYTES, 0)


# ---- several handles ----
def multi_group(method, comps, B, atts, keys, by, cols, devices, group_cap=None):
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    try:
        def chk(rc, what):
            if rc != 0:
                raise CryoError(rc, what, L.cryo_multi_last_error(h).decode())
        return cc.group_blocks_call(L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys),
                                    cc.group_desc(by), cc.agg_desc(cols), group_cap)
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("devices", [(0,), (0, 0), (0, 1)])
def test_multi_group_blocks(grp, oracle, sixty_four, devices):
    """one handle; two handles on one device; two devices: byte for byte the single-handle call"""
    if max(devices) >= cc.device_count():
        pytest.skip("one device visible")
    B, raws, keys = sixty_four
    raws = raws[:11]
    cols = ROWID + ROWID
    for method in METHODS:
        comps = [oracle_encode(oracle, method, r) for r in raws]
        comps[2] = comps[2][:40]
        want = gr.group_call([None if i == 2 else r for i, r in enumerate(raws)], SYNTH_ATTS, keys, ROWID, cols)
        got = multi_group(method, comps, B, SYNTH_ATTS, keys, ROWID, cols, devices)
        same(got, want, (method, devices))
        one = host_call(grp, method, comps, B, SYNTH_ATTS, keys, ROWID, cols)
        assert got[3] == one[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], one[:3]))
        same(multi_group(method, comps, B, SYNTH_ATTS, keys, ROWID, cols, devices, want[3]), want, "exactly the need")
        with pytest.raises(CryoError) as e:
            multi_group(method, comps, B, SYNTH_ATTS, keys, ROWID, cols, devices, want[3] - 1)
        assert e.value.code == cc.E_DSTSIZE
    rows, recs, cells, total = multi_group(METHOD_LZ4, [], B, SYNTH_ATTS, keys, ROWID, cols, devices)
    assert rows.size == 0 and recs.size == 0 and total == 0


# ---- arguments ----
def test_descriptor_rules(grp, oracle):
    """every argument rule of the three descriptors, on host arrays (refused before a device is touched: the transfer counters
    stand still) and on device arrays"""
    B = ac.B
    arr = np.ascontiguousarray(oracle.lz4_compress(ac.range_block(), 1))
    L = grp.L
    src, szs = (C.c_void_p * 1)(arr.ctypes.data), (C.c_uint32 * 1)(arr.nbytes)
    rows, recs, cells = np.zeros(1, cc.GROUP_BLOCK), np.zeros(290, cc.GROUP_REC), np.zeros(4 * 290, cc.AGG_CELL)
    total = C.c_uint64()
    bufs = [grp.alloc(6416), grp.alloc(96), grp.alloc(64), grp.alloc(64), grp.alloc(4096), grp.alloc(8), grp.alloc(4), grp.alloc(32),
            grp.alloc(24 * 290), grp.alloc(160 * 290), grp.alloc(8)]
    d_atts, d_keys, d_by, d_cols, d_src, d_off, d_sz, d_rows, d_recs, d_cells, d_total = bufs
    try:
        d_src.upload(np.concatenate([arr, np.zeros(4096 - arr.nbytes, np.uint8)]))
        d_off.upload(np.zeros(1, np.uint64))
        d_sz.upload(np.array([arr.nbytes], np.uint32))
        for name, atts, keys, by, cols, flags, patch, ok in gc.descriptors():
            assert gc.ref_ok(gr, atts, keys, by, cols, flags, patch) == ok, name
            f, a, k = cc.filter_desc(atts, keys, flags)
            r, b = cc.group_desc(by)
            g, c = cc.agg_desc(cols or [])
            if patch:
                which, field, index, value = patch
                if which in "frg":
                    {"f": f, "r": r, "g": g}[which].rsv = value
                else:
                    {"a": a, "k": k, "b": b, "c": c}[which][field][index] = value
            before = grp.transfer_counters()
            rc = L.cryo_codec_group_blocks(grp.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), C.byref(r), None if cols is None else C.byref(g),
                                           rows.ctypes.data, recs.ctypes.data, 290, cells.ctypes.data, C.byref(total))
            assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
            if not ok:
                assert grp.transfer_counters() == before, name
            if len(atts):
                d_atts.upload(a)
            d_keys.upload(k)
            d_by.upload(b)
            d_cols.upload(c)
            fd = cc.CryoFilter(f.natts, f.nkeys, f.flags, f.rsv, d_atts.ptr, d_keys.ptr if len(keys) else None)
            rd = cc.CryoGroup(r.nby, r.rsv, d_by.ptr)
            gd = cc.CryoAgg(g.ncols, g.rsv, d_cols.ptr)
            rc = L.cryo_codec_group_batch(grp.h, METHOD_LZ4, d_src.ptr, d_off.ptr, d_sz.ptr, B, 1, C.byref(fd), C.byref(rd),
                                          None if cols is None else C.byref(gd), d_rows.ptr, d_recs.ptr, 290, d_cells.ptr, d_total.ptr)
            grp.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    finally:
        for x in bufs:
            x.free()


def test_arguments(grp, oracle):
    comp = oracle.lz4_compress(oracle.synth(1, 0, 4096, 1), 1)
    d = [grp.alloc(512) for _ in range(11)]
    try:
        _, a, k = cc.filter_desc(SYNTH_ATTS, [(1, fr.INT4, fr.GE, 1), (1, fr.INT4, fr.LT, 5)])
        _, g = cc.agg_desc(ROWID)
        d[3].upload(a)
        d[4].upload(k)
        d[5].upload(g)
        d[8].upload(g)

        class Shifted:                                                    # a device pointer that breaks the alignment rule
            def __init__(self, buf, by):
                self.ptr = buf.ptr + by

        def call(method=METHOD_LZ4, B=4096, n=1, natts=2, nkeys=2, nby=1, by=d[8], ncols=1, cols=d[5], rows=d[6], recs=d[7], cap=16,
                 cells=d[9], total=d[10]):
            grp.group_batch(method, d[0], d[1], d[2], B, n, natts, d[3], nkeys, d[4], nby, by, ncols, cols, rows, recs, cap, cells, total)

        for kw in (dict(method=7), dict(B=4092), dict(B=8), dict(B=0), dict(natts=0), dict(natts=1601), dict(nkeys=5), dict(nby=0),
                   dict(nby=3), dict(by=None), dict(ncols=5), dict(cols=None), dict(rows=None), dict(recs=None), dict(cells=None),
                   dict(total=None), dict(rows=Shifted(d[6], 8)), dict(recs=Shifted(d[7], 4)), dict(cells=Shifted(d[9], 4)),
                   dict(cols=Shifted(d[5], 4)), dict(by=Shifted(d[8], 4)), dict(total=Shifted(d[10], 4))):
            with pytest.raises(CryoError) as e:
                call(**kw)
            assert e.value.code == cc.E_ARG, kw
        for x in (d[6], d[7], d[9]):
            x.memset(0xEE)
        call(n=0)                                                         # no block: the total is 0 and nothing else is written
        grp.sync()
        assert all((x.download() == 0xEE).all() for x in (d[6], d[7], d[9])) and not d[10].download()[:8].any()
        bad = g.copy()
        bad["type"][0] = fr.INT8                                          # not the column's size, found in the device copy
        d[8].upload(bad)
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
    finally:
        for x in d:
            x.free()
    fdesc, gdesc, adesc = cc.filter_desc(SYNTH_ATTS, []), cc.group_desc(ROWID), cc.agg_desc(ROWID)
    with pytest.raises(CryoError) as e:
        grp.group_blocks(METHOD_ZSTD, [comp], 4100, fdesc, gdesc, adesc)
    assert e.value.code == cc.E_ARG
    rows, recs, cells, total = grp.group_blocks(METHOD_LZ4, [], 4096, fdesc, gdesc, adesc)
    assert rows.size == 0 and recs.size == 0 and total == 0
    rows, recs, cells, total = grp.group_blocks(METHOD_LZ4, [comp], 4096, fdesc, gdesc, adesc)
    assert rows["n_match"][0] == rows["n_items"][0] == rows["n_groups"][0] == total == recs.size > 0
    assert (recs["n_rows"] == 1).all() and (cells["min"][:, 0] == recs["key"][:, 0]).all()
