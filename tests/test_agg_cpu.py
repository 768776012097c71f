"""CPU tests of the scan aggregate: the rules (tests/agg_ref.py) on hand-made vectors (tests/agg_cases.py) with the expected values
written out here, the descriptor rules, and cryo_aggregate_scan (host/aggregate.c) walking a mini-AM relation through the test
build, with a codec double whose agg_blocks decodes with the oracle and answers by the rules."""
import ctypes as C
import struct

import numpy as np
import pytest

import agg_cases as ac
import agg_ref as ar
import fetch_walk
import filter_cases as fc
import filter_ref as fr
import tuple_craft as tc
from pg_cryogen_amd import codec, host

B128 = 131072
E_UNSUPPORTED, E_ARG = -6, -1
M64 = (1 << 64) - 1


def cells(block, keys, cols, atts=ac.ATTS):
    row, cs = ar.agg_block(block, atts, keys, cols)
    return row, cs


# ---- the reference on hand-made vectors ----
def test_range_and_every_type():
    row, cs = cells(ac.range_block(), ac.RANGE_KEYS, ac.COLS4)                    # i = 5 .. 11 of 30
    assert row == (0, 30, 7, 0)
    assert cs[0] == (7, 1005, 1011, 7056, 0)                                      # 1000 + i
    assert cs[1] == (7, 5, 11, 56, 0)                                             # i
    assert cs[2] == (7, -11, -5, (1 << 64) - 56, -1)                              # -i: a negative sum in two's complement
    assert cs[3] == (7, 50, 110, 560, 0)                                          # 10 i
    row, cs = cells(ac.range_block(), [(4, fr.INT4, fr.GT, 1000)], [(2, fr.INT8)])
    assert row == (0, 30, 0, 0) and cs == [(0, 0, 0, 0, 0)]                       # nothing matches
    # the same column twice; a column that also carries a key
    row, cs = cells(ac.range_block(), ac.RANGE_KEYS, [(4, fr.INT4), (4, fr.INT4)])
    assert cs == [(7, 50, 110, 560, 0)] * 2


def test_nulls_and_short_tuples():
    # key on column 4 = 7: positions 1, 2, 3, 5, 6, 7; column 2 is NULL at position 2, column 6 at position 6
    row, cs = cells(ac.nulls_block(), fc.K4, [(2, fr.INT8), (6, fr.INT8), (4, fr.INT4)])
    assert row == (0, 7, 6, 0)
    assert cs == [(5, 100, 100, 500, 0), (5, 900, 900, 4500, 0), (6, 7, 7, 42, 0)]
    # no key: every tuple matches; a column beyond the tuple's natts is NULL
    row, cs = cells(ac.short_block(), [], [(6, fr.INT8), (4, fr.INT4), (1, fr.INT2)])
    assert row == (0, 5, 5, 0)
    assert cs == [(2, 900, 900, 1800, 0), (3, 7, 7, 21, 0), (4, 5, 5, 20, 0)]
    # every match NULL in the column: n = 0, min = max = 0, and the matches still count
    row, cs = cells(ac.all_null_block(), fc.K4, [(2, fr.INT8), (6, fr.INT8)])
    assert row == (0, 8, 8, 0) and cs == [(0, 0, 0, 0, 0), (8, 1, 8, 36, 0)]


def test_walk_length_differs_from_the_filter():
    blk = ac.cut_block()
    k1 = [(1, fr.INT2, fr.EQ, 5)]
    assert [r[:2] for r in fr.filter_block(blk, ac.ATTS, k1)[2]] == [(1, fr.OK), (2, fr.OK), (3, fr.OK)]     # the filter: a match
    row, cs = cells(blk, k1, [(6, fr.INT8)])
    assert row == (0, 3, 2, 1) and cs == [(2, 900, 900, 1800, 0)]                 # here: TUPLE, the walk goes on to column 6
    row, cs = cells(blk, k1, [(4, fr.INT4)])
    assert row == (0, 3, 3, 0) and cs == [(3, 7, 7, 21, 0)]                       # a column the cut tuple still holds


def test_bad_items_and_tuples_are_counted_and_add_nothing():
    blk, bad = ac.damaged_block()
    row, cs = cells(blk, fc.WALK, [(6, fr.INT8), (2, fr.INT8)])
    assert len(bad) == 10 and row == (0, 21, 11, 10) and cs == [(11, 900, 900, 9900, 0), (11, 100, 100, 1100, 0)]
    row, cs = cells(ac.bad_item_block(), fc.K6, [(2, fr.INT8)])
    assert row == (0, 6, 5, 1) and cs == [(5, 100, 100, 500, 0)]


def test_stream_and_header_blocks_are_all_zero():
    assert cells(None, [], ac.COLS4) == ((fr.STREAM, 0, 0, 0), [(0, 0, 0, 0, 0)] * 4)
    assert cells(ac.header_block(), [], [(2, fr.INT8)]) == ((fr.HEADER, 0, 0, 0), [(0, 0, 0, 0, 0)])
    rows, cs = ar.agg_call([ac.range_block(), None, ac.header_block(), ac.range_block()], ac.ATTS, ac.RANGE_KEYS, [(2, fr.INT8)])
    assert rows["status"].tolist() == [0, fr.STREAM, fr.HEADER, 0] and rows["n_match"].tolist() == [7, 0, 0, 7]
    assert cs["n"][:, 0].tolist() == [7, 0, 0, 7] and not cs[1:3].view(np.uint8).any()
    assert ar.combine(rows, cs) == [(14, 1005, 1011, 14112)]


def test_extremes_need_128_bits():
    got = {name: cells(blk, [], ac.EXT_COLS, ac.EXT_ATTS) for name, blk in ac.extremes_blocks()}
    assert all(row == (0, 290, 290, 0) for row, _ in got.values())
    # 290 x INT64_MIN = -145 x 2^64; 290 x INT64_MAX = 145 x 2^64 - 290; 145 x (INT64_MAX + INT64_MIN) = -145
    assert got["min"][1][0] == (290, ac.I64_MIN, ac.I64_MIN, 0, -145)
    assert got["max"][1][0] == (290, ac.I64_MAX, ac.I64_MAX, (1 << 64) - 290, 144)
    assert got["mix"][1][0] == (290, ac.I64_MIN, ac.I64_MAX, (1 << 64) - 145, -1)
    assert got["min"][1][1] == (290, -(1 << 31), -(1 << 31), (-290 << 31) & M64, -1)
    assert got["max"][1][1] == (290, (1 << 31) - 1, (1 << 31) - 1, 290 * ((1 << 31) - 1), 0)
    assert got["mix"][1][1] == (290, -(1 << 31), (1 << 31) - 1, (1 << 64) - 145, -1)
    assert got["min"][1][2] == (290, -32768, -32768, (-290 * 32768) & M64, -1)
    assert got["max"][1][2] == (290, 32767, 32767, 290 * 32767, 0)
    assert got["mix"][1][2] == (290, -32768, 32767, (1 << 64) - 145, -1)
    assert ar.split(290 * ac.I64_MAX) == ((1 << 64) - 290, 144) and ar.split(-1) == (M64, -1) and ar.split(0) == (0, 0)


def test_turn_blocks():
    for n, blk, marked in ac.turn_blocks():
        row, cs = cells(blk, ac.TURN_KEYS, [(1, fr.INT4)], ac.TURN_ATTS)
        assert row == (0, n, len(marked), 0)
        assert cs[0][:3] == ((len(marked), 1001, 1000 + n) if n else (0, 0, 0)) and cs[0][3] == sum(1000 + p for p in marked)
    assert [len(m) for _, _, m in ac.turn_blocks()] == [0, 1, 2, 2, 3, 4, 5, 10]


def test_reference_on_generator_blocks(oracle):
    """rowid = block x 290 + pos is the int4 column of `narrow` and `wide`: the cell of a range is the arithmetic series"""
    for d, block, B in ((1, 0, 131072), (0, 3, 131072), (1, 2, 1 << 20)):
        raw = oracle.synth(21, block, B, d)
        lo, hi = block * 290 + 40, block * 290 + 140
        row, cs = ar.agg_block(raw, [(4, 4), (-1, 4)], [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)], [(1, fr.INT4)])
        assert row == (0, 290, 100, 0) and cs == [(100, lo, hi - 1, sum(range(lo, hi)), 0)]


def test_descriptor_rules():
    for name, atts, keys, cols, flags, patch, ok in ac.descriptors():
        assert ac.ref_ok(ar, atts, keys, cols, flags, patch) == ok, name


# ---- the walk, through a codec double ----
class AggregatingDouble:
    """the oracle double of tests/codec_double.py plus an aggregate table that decodes with the oracle and answers from agg_ref"""

    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self._agg = host.AGG_BLOCKS_FN(self.agg_blocks)
        self.agg_ops = host.CryoCodecAggOps(self._agg)

    def agg_blocks(self, ctx, method, srcs, sizes, n, bs, filt, agg, rows, cells):
        f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents
        atts = np.ctypeslib.as_array(C.cast(f.atts, C.POINTER(C.c_uint8)), (4 * f.natts,)).view(codec.FILTER_ATT)
        keys = np.ctypeslib.as_array(C.cast(f.keys, C.POINTER(C.c_uint8)), (16 * f.nkeys,)).view(codec.FILTER_KEY) if f.nkeys else []
        cols = np.ctypeslib.as_array(C.cast(g.cols, C.POINTER(C.c_uint8)), (8 * g.ncols,)).view(codec.AGG_COL) if g.ncols else []
        atts = [(int(a["attlen"]), int(a["attalign"])) for a in atts]
        keys = [(int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"])) for k in keys]
        cols = [(int(c["att"]), int(c["type"])) for c in cols]
        if not ar.desc_ok(atts, keys, cols, f.flags, f.rsv, g.rsv):
            return E_ARG
        blocks = []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(ar.decode(self.base.ora, method, comp, bs))
        self.calls.append((method, n))
        r, c = ar.agg_call(blocks, atts, keys, cols)
        C.memmove(rows, r.ctypes.data, r.nbytes)
        C.memmove(cells, np.ascontiguousarray(c).ctypes.data, c.nbytes)
        return 0


@pytest.fixture()
def HA():
    L = host.lib()
    dbl = AggregatingDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_agg_ops(C.byref(dbl.agg_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_aggregate_set_window(0, 0)
    L.cryo_cache_shutdown()
    L.cryo_host_set_agg_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


ATTS2 = [(4, 4), (8, 8)]
COLS2 = [(2, fr.INT8), (1, fr.INT4)]


def _relation(L, oracle, nblocks=9, big=False):
    """nblocks chains of 40 tuples (rowid int4, int8): even ones LZ4, odd ones zstd, xid 500 + k.  big: the int8 column holds
    INT64_MAX, so the relation's sum needs more than 64 bits.  Returns (mem, rel, decoded blocks, first pages)"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws, firsts = [], []
    for k in range(nblocks):
        tuples = [tc.form_tuple(ATTS2, [40 * k + i, ac.I64_MAX if big else -(40 * k + i) * 3]) for i in range(1, 41)]
        raw = tc.build_block(B128, tuples)
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def _want_block(first, xid, raw, keys, cols):
    row, cs = ar.agg_block(raw, ATTS2, keys, cols)
    return ("block", first, xid, row[1], row[2], row[3], [(c[0], c[1], c[2], (c[4] << 64) + c[3]) for c in cs])


def _combined(events, ncols):
    out = []
    for j in range(ncols):
        cs = [e[6][j] for e in events if e[0] == "block" and e[6][j][0] > 0]
        out.append((sum(c[0] for c in cs), min((c[1] for c in cs), default=0), max((c[2] for c in cs), default=0), sum(c[3] for c in cs)))
    return out


def test_aggregate_scan_walk_through_a_double(HA, oracle):
    L, dbl, errors = HA
    mem, rel, raws, firsts = _relation(L, oracle)
    # behind the nine good chains: a block with a damaged item and a damaged tuple, a chain that cannot be read, an unknown
    # method, a stream the decoders reject, a block with a bad header, and a good chain behind them all
    bad = raws[2].copy()
    bad[12 + 8 * 4:16 + 8 * 4] = 0                                        # item 5: len 0
    off7 = struct.unpack_from("<I", bad, 8 + 8 * 6)[0]
    bad[off7 + 22] = 16                                                   # tuple 7: hoff 16
    item_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 901, oracle.lz4_compress(bad, 1))
    short_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 904, oracle.lz4_compress(raws[0], 1))
    odd_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 905, oracle.lz4_compress(raws[0], 1))
    dead_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 906, oracle.lz4_compress(raws[3], 1))
    hdr = raws[1].copy()
    hdr[0:4] = np.frombuffer(struct.pack("<I", 12), np.uint8)
    hdr_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 908, oracle.zstd_compress(hdr, 1))
    tail_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 907, oracle.zstd_compress(raws[0], 1))
    page = L.cryo_memrel_page(mem, short_first)
    csize = struct.unpack_from("<I", C.string_at(page, 64), 40)[0]
    C.memmove(page + 40, struct.pack("<I", csize + 100000), 4)
    C.memmove(L.cryo_memrel_page(mem, odd_first) + 36, struct.pack("<i", 9), 4)
    C.memset(L.cryo_memrel_page(mem, dead_first) + 48, 0xFF, 64)

    keys = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 250)]
    events, t = host.aggregate_scan(rel, ATTS2, keys, COLS2)
    want = [_want_block(firsts[k], 500 + k, raws[k], keys, COLS2) for k in range(9)]
    want += [_want_block(item_first, 901, bad, keys, COLS2),
             ("report", short_first, fetch_walk.CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED), ("report", odd_first, fetch_walk.METHOD, 9),
             ("report", dead_first, fr.STREAM, 0), ("report", hdr_first, fr.HEADER, 0), _want_block(tail_first, 907, raws[0], keys, COLS2)]
    assert events == want                                                 # one row and one xid per block, in block order
    assert want[9][3:6] == (40, 38, 2) and want[0][4] == 11 and want[8][4] == 0
    assert dbl.calls == [(host.COMP_LZ4, 7), (host.COMP_ZSTD, 6)]         # both methods in one relation: one call each
    blocks = [e for e in events if e[0] == "block"]
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"]) == \
        (15, 40 * 11, sum(e[4] for e in blocks), 2, 4, 2)
    assert t["bytes_back"] == 13 * (16 + 40 * 2)
    assert t["cells"] == _combined(events, 2)
    assert t["cells"][1][:3] == (t["matches"], 30, 249) and t["cells"][0][3] == -3 * t["cells"][1][3]
    # a frozen block is handed over with FrozenTransactionId, as the read path does
    L.cryo_memrel_set_frozen(mem, firsts[3], True)
    events, _ = host.aggregate_scan(rel, ATTS2, keys, COLS2)
    assert [e[2] for e in events if e[0] == "block"][:5] == [500, 501, 502, 2, 504]
    # descriptors the codec refuses; null arguments
    with pytest.raises(host.AggregateScanError) as e:
        host.aggregate_scan(rel, ATTS2, keys, [(2, fr.INT4)])
    assert e.value.code == E_ARG and e.value.events == []
    with pytest.raises(host.AggregateScanError) as e:
        host.aggregate_scan(rel, ATTS2, keys, [])
    assert e.value.code == E_ARG
    f, g = codec.filter_desc(ATTS2, keys), codec.agg_desc(COLS2)
    nb, nr = host.AGG_BLOCK_FN(0), host.FETCH_REPORT_FN(0)
    assert L.cryo_aggregate_scan(C.byref(rel), None, C.byref(g[0]), nb, nr, None, None) == E_ARG
    assert L.cryo_aggregate_scan(C.byref(rel), C.byref(f[0]), None, nb, nr, None, None) == E_ARG
    assert L.cryo_aggregate_scan(None, C.byref(f[0]), C.byref(g[0]), nb, nr, None, None) == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_aggregate_scan_windows(HA, oracle):
    """the window lowered to 4 chains, then to the compressed bytes of about three: several codec calls, the same delivery"""
    L, dbl, _ = HA
    mem, rel, raws, firsts = _relation(L, oracle)
    keys = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 250)]
    whole, t0 = host.aggregate_scan(rel, ATTS2, keys, COLS2)
    assert dbl.calls == [(host.COMP_LZ4, 5), (host.COMP_ZSTD, 4)] and t0["codec_calls"] == 2
    dbl.calls.clear()
    L.cryo_aggregate_set_window(4, 0)
    got, t = host.aggregate_scan(rel, ATTS2, keys, COLS2)
    assert got == whole and [e[1] for e in got] == firsts
    assert dbl.calls == [(host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 1)]
    assert t["codec_calls"] == 5
    assert {k: v for k, v in t.items() if k != "codec_calls"} == {k: v for k, v in t0.items() if k != "codec_calls"}
    dbl.calls.clear()
    csize = len(oracle.lz4_compress(raws[0], 1))
    L.cryo_aggregate_set_window(0, 3 * csize + csize // 2)
    got, t = host.aggregate_scan(rel, ATTS2, keys, COLS2)
    assert got == whole and t["codec_calls"] == len(dbl.calls) >= 3 and t["cells"] == t0["cells"]
    L.cryo_memrel_destroy(mem)


def test_totals_beyond_64_bits(HA, oracle):
    """six blocks of 40 x INT64_MAX: each block's sum needs 69 bits, the relation's 72; the totals carry across the words"""
    L, dbl, _ = HA
    mem, rel, raws, firsts = _relation(L, oracle, nblocks=6, big=True)
    L.cryo_aggregate_set_window(4, 0)                                     # two windows: the totals run on across them
    events, t = host.aggregate_scan(rel, ATTS2, [], COLS2)
    assert len(events) == 6 and all(e[6][0] == (40, ac.I64_MAX, ac.I64_MAX, 40 * ac.I64_MAX) for e in events)
    assert t["cells"][0] == (240, ac.I64_MAX, ac.I64_MAX, 240 * ac.I64_MAX) and 240 * ac.I64_MAX > 1 << 70
    assert t["cells"] == _combined(events, 2) and t["cells"][1] == (240, 1, 240, 240 * 241 // 2)
    L.cryo_memrel_destroy(mem)


def test_without_an_aggregate_table_the_scan_is_unsupported(HA, oracle):
    L, dbl, _ = HA
    mem, rel, raws, firsts = _relation(L, oracle, nblocks=2)
    L.cryo_host_set_agg_ops(None)
    with pytest.raises(host.AggregateScanError) as e:
        host.aggregate_scan(rel, ATTS2, [], COLS2)
    assert e.value.code == E_UNSUPPORTED and e.value.events == [] and e.value.totals["blocks"] == 0
    L.cryo_memrel_destroy(mem)
