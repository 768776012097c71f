"""GPU tests of the scan aggregate (cryo_codec_agg_batch, cryo_codec_agg_blocks, cryo_multi_agg_blocks).

Every row and every cell is compared with tests/agg_ref.py, the numpy statement of the rules in include/cryo_codec.h, applied to
the ORACLE's decode of each stream.  The device buffers are filled with a sentinel before every call: nothing beyond the rows and
the cells of the call may be written."""
import ctypes as C

import numpy as np
import pytest

import agg_cases as ac
import agg_ref as ar
import filter_cases as fc
import filter_ref as fr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
SYNTH_ATTS = [(4, 4), (-1, 4)]
ROWID = [(1, fr.INT4)]
METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def agg(codec):
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


def agg_batch(codec, method, comps, B, atts, keys, cols):
    """cryo_codec_agg_batch on device copies of the streams and of the descriptors: (rows, cells of shape (n, ncols)); rows and
    cells are filled with SENTINEL before the call and the 64 bytes behind each must still hold it afterwards"""
    n, nc = len(comps), len(cols)
    packed, offs, sizes = pack_streams(comps)
    _, a, k = cc.filter_desc(atts, keys)
    _, g = cc.agg_desc(cols)
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(a.nbytes), codec.alloc(k.nbytes),
            codec.alloc(g.nbytes), codec.alloc(16 * n + 64), codec.alloc(40 * n * nc + 64)]
    d_src, d_off, d_sz, d_atts, d_keys, d_cols, d_rows, d_cells = bufs
    try:
        d_src.upload(packed)
        d_off.upload(offs)
        d_sz.upload(sizes)
        d_atts.upload(a)
        d_keys.upload(k)
        d_cols.upload(g)
        d_rows.memset(SENTINEL)
        d_cells.memset(SENTINEL)
        codec.agg_batch(method, d_src, d_off, d_sz, B, n, len(atts), d_atts, len(keys), d_keys if keys else None, nc, d_cols,
                        d_rows, d_cells)
        codec.sync()
        rows, cells = d_rows.download(), d_cells.download()
        assert (rows[16 * n:] == SENTINEL).all() and (cells[40 * n * nc:] == SENTINEL).all(), "a byte beyond the call's output was written"
        return rows[:16 * n].view(cc.AGG_BLOCK).copy(), cells[:40 * n * nc].view(cc.AGG_CELL).reshape(n, nc).copy()
    finally:
        for b in bufs:
            b.free()


def host_call(codec, method, comps, B, atts, keys, cols):
    return codec.agg_blocks(method, comps, B, cc.filter_desc(atts, keys), cc.agg_desc(cols))


def same(got, want, what=""):
    rows, cells = got
    erows, ecells = want
    assert rows.shape == erows.shape and cells.shape == ecells.shape, (what, rows.shape, erows.shape, cells.shape, ecells.shape)
    for f in erows.dtype.names:
        bad = np.flatnonzero(rows[f] != erows[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(rows[i]), tuple(erows[i])) for i in bad[:5]])
    for f in ecells.dtype.names:
        bad = np.argwhere(cells[f] != ecells[f])
        assert bad.size == 0, (what, f, [(tuple(ij), tuple(cells[tuple(ij)]), tuple(ecells[tuple(ij)])) for ij in bad[:5]])


def both(codec, oracle, blocks, B, atts, keys, cols, what, methods=METHODS):
    """device buffers and host buffers, on the oracle's streams of `blocks`, against agg_ref; returns the expectation"""
    want = ar.agg_call(blocks, atts, keys, cols)
    for method in methods:
        comps = [oracle_encode(oracle, method, b) for b in blocks]
        same(agg_batch(codec, method, comps, B, atts, keys, cols), want, (what, method))
        same(host_call(codec, method, comps, B, atts, keys, cols), want, (what, method, "host buffers"))
    return want


# ---- the turns of a wave: 64 items each ----
def test_turn_boundaries(agg, oracle):
    """0, 1, 63, 64, 65, 128, 129 and 290 items; the matches sit in the first and the last lane of each turn"""
    turns = ac.turn_blocks()
    blocks = [b for _, b, _ in turns]
    rows, cells = both(agg, oracle, blocks, ac.TURN_B, ac.TURN_ATTS, ac.TURN_KEYS, [(1, fr.INT4)], "marked")
    assert rows["n_items"].tolist() == list(ac.TURN_SIZES) and rows["n_match"].tolist() == [len(m) for _, _, m in turns]
    assert cells["max"][:, 0].tolist() == [1000 + n if n else 0 for n in ac.TURN_SIZES]
    rows, cells = both(agg, oracle, blocks, ac.TURN_B, ac.TURN_ATTS, [(1, fr.INT4, fr.GE, 0)], [(1, fr.INT4)], "all")
    assert rows["n_match"].tolist() == list(ac.TURN_SIZES)
    both(agg, oracle, blocks, ac.TURN_B, ac.TURN_ATTS, [(1, fr.INT4, fr.LT, 0)], [(1, fr.INT4)], "none", [METHOD_LZ4])


# ---- sums beyond 64 bits ----
def test_extremes(agg, oracle):
    blocks = [b for _, b in ac.extremes_blocks()]
    rows, cells = both(agg, oracle, blocks, ac.EXT_B, ac.EXT_ATTS, [], ac.EXT_COLS, "extremes")
    assert rows["n_match"].tolist() == [290] * 3
    assert [ar.total_of(c) for c in cells[:, 0]] == [290 * ac.I64_MIN, 290 * ac.I64_MAX, -145]
    assert cells["sum_hi"][:, 0].tolist() == [-145, 144, -1]                       # the int8 sums need the high word
    assert cells["min"][:, 0].tolist() == [ac.I64_MIN, ac.I64_MAX, ac.I64_MIN] and cells["max"][2, 0] == ac.I64_MAX
    assert cells["min"][2].tolist() == [ac.I64_MIN, -(1 << 31), -(1 << 15)] and cells["max"][2].tolist() == [ac.I64_MAX, (1 << 31) - 1, (1 << 15) - 1]
    # the keys at the extremes too: only the maxima pass
    rows, cells = both(agg, oracle, blocks, ac.EXT_B, ac.EXT_ATTS, [(1, fr.INT8, fr.EQ, ac.I64_MAX)], ac.EXT_COLS, "maxima only")
    assert rows["n_match"].tolist() == [0, 290, 145] and ar.total_of(cells[2, 0]) == 145 * ac.I64_MAX


# ---- NULLs ----
def test_nulls(agg, oracle):
    cols = [(2, fr.INT8), (6, fr.INT8), (4, fr.INT4)]
    blocks = [ac.nulls_block(), ac.short_block(), ac.all_null_block(), ac.range_block()]
    rows, cells = both(agg, oracle, blocks, ac.B, ac.ATTS, fc.K4, cols, "key on 4")
    assert rows["n_match"].tolist() == [6, 3, 8, 0] and cells["n"].tolist() == [[5, 5, 6], [3, 2, 3], [0, 8, 8], [0, 0, 0]]
    assert tuple(cells[2, 0]) == (0, 0, 0, 0, 0)                                   # every match NULL there: n = 0, min = max = 0
    rows, cells = both(agg, oracle, blocks, ac.B, ac.ATTS, [], cols, "no key")
    assert rows["n_match"].tolist() == [7, 5, 8, 30] and cells["n"][1].tolist() == [4, 2, 3]   # natts ends before the column
    both(agg, oracle, blocks, ac.B, ac.ATTS, [(2, 0, fr.ISNULL, 0)], cols, "ISNULL on an aggregate column")


# ---- the walk goes as far as the last aggregate column ----
def test_walk_length(agg, oracle):
    blk = ac.cut_block()
    k1 = [(1, fr.INT2, fr.EQ, 5)]
    rows, cells = both(agg, oracle, [blk, ac.range_block()], ac.B, ac.ATTS, k1, [(6, fr.INT8)], "column 6 beyond the key")
    assert tuple(rows[0]) == (0, 3, 2, 1) and tuple(cells[0, 0]) == (2, 900, 900, 1800, 0)
    rows, _ = both(agg, oracle, [blk], ac.B, ac.ATTS, k1, [(4, fr.INT4)], "column 4 still fits")
    assert tuple(rows[0]) == (0, 3, 3, 0)
    # the documented difference: the filter, with the same keys, walks to column 1 only and calls the cut tuple a match
    for method in METHODS:
        table, recs, _, _ = agg.filter_blocks(method, [oracle_encode(oracle, method, blk)], ac.B, cc.filter_desc(ac.ATTS, k1))
        assert (table["n_match"][0], table["n_bad"][0]) == (3, 0) and recs["pos"][:3].tolist() == [1, 2, 3]


# ---- damage ----
def test_crafted_bad_tuples(agg, oracle):
    blk, bad = ac.damaged_block()
    blocks = [blk, ac.bad_item_block(), blk]
    rows, cells = both(agg, oracle, blocks, ac.B, ac.ATTS, fc.WALK, [(6, fr.INT8), (2, fr.INT8)], "damaged")
    assert rows["n_bad"].tolist() == [len(bad), 1, len(bad)] and rows["n_match"].tolist() == [11, 5, 11]
    assert [ar.total_of(c) for c in cells[:, 0]] == [9900, 4500, 9900] and cells["n"][:, 1].tolist() == [11, 5, 11]
    # a key that lets nothing through: the bad ones are still counted
    rows, cells = both(agg, oracle, blocks, ac.B, ac.ATTS, [(6, fr.INT8, fr.LT, 0)], [(6, fr.INT8)], "damaged, no match")
    assert rows["n_bad"].tolist() == [len(bad), 1, len(bad)] and not cells.view(np.uint8).any()


def test_rejected_streams_between_good_neighbours(agg, oracle):
    good = ac.range_block()
    blocks = [good, None, ac.header_block(), good, None, good]
    want = ar.agg_call(blocks, ac.ATTS, ac.RANGE_KEYS, ac.COLS4)
    assert want[0]["status"].tolist() == [0, fr.STREAM, fr.HEADER, 0, fr.STREAM, 0]
    for method in METHODS:
        comps = [oracle_encode(oracle, method, good if b is None else b) for b in blocks]
        comps[1] = comps[1][:len(comps[1]) - 7]
        comps[4] = comps[4][:len(comps[4]) // 2]
        assert [ar.decode(oracle, method, c, ac.B) is None for c in comps] == [b is None for b in blocks]
        for got in (agg_batch(agg, method, comps, ac.B, ac.ATTS, ac.RANGE_KEYS, ac.COLS4),
                    host_call(agg, method, comps, ac.B, ac.ATTS, ac.RANGE_KEYS, ac.COLS4)):
            same(got, want, method)
            assert not got[1][[1, 2, 4]].view(np.uint8).any() and got[0]["n_items"].tolist() == [30, 0, 0, 30, 0, 30]


# ---- column combinations ----
def test_column_combinations(agg, oracle):
    blocks = [ac.range_block(), ac.nulls_block(), ac.short_block(), ac.range_block(), ac.all_null_block()]
    for cols in ([(2, fr.INT8)], [(4, fr.INT4), (1, fr.INT2)], ac.COLS4[:3], ac.COLS4, [(6, fr.INT8), (6, fr.INT8)],
                 [(4, fr.INT4), (2, fr.INT8), (4, fr.INT4), (2, fr.INT8)], [(1, fr.INT2)]):
        for keys in (ac.RANGE_KEYS, [(1, fr.INT2, fr.GE, 5), (6, fr.INT8, fr.NE, -7)]):
            both(agg, oracle, blocks, ac.B, ac.ATTS, keys, cols, (cols, keys), [METHOD_LZ4 if len(cols) % 2 else METHOD_ZSTD])


# ---- the generator's blocks ----
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_generator_blocks(agg, oracle, B):
    """`narrow` and `wide` blocks with a range on the rowid column that cuts through two of them: the cells equal agg_ref and the
    numpy reduction of the tuples filter_blocks returns for the same keys"""
    for dist in (1, 0):
        raws = [oracle.synth(31, k, B, dist) for k in range(4)]
        keys = [(1, fr.INT4, fr.GE, 290 + 100), (1, fr.INT4, fr.LT, 2 * 290 + 50)]
        want = ar.agg_call(raws, SYNTH_ATTS, keys, ROWID)
        assert want[0]["n_match"].tolist() == [0, 191, 49, 0] and want[0]["n_items"].tolist() == [290] * 4   # 0 < n_match < n_items
        for method in METHODS:
            comps = [oracle_encode(oracle, method, r) for r in raws]
            got = host_call(agg, method, comps, B, SYNTH_ATTS, keys, ROWID)
            same(got, want, (dist, method))
            same(agg_batch(agg, method, comps, B, SYNTH_ATTS, keys, ROWID), want, (dist, method, "device buffers"))
            table, recs, dst, _ = agg.filter_blocks(method, comps, B, cc.filter_desc(SYNTH_ATTS, keys))
            for i in range(4):
                v = np.array([int.from_bytes(t[24:28], "little", signed=True) for _, t in fr.tuples_of(table, recs, dst, i)], np.int64)
                cell = got[1][i, 0]
                assert (int(cell["n"]), ar.total_of(cell)) == (v.size, int(v.sum())), (dist, method, i)
                assert (int(cell["min"]), int(cell["max"])) == ((int(v.min()), int(v.max())) if v.size else (0, 0)), (dist, method, i)


# ---- chunks ----
@pytest.fixture(scope="module")
def sixty_four(oracle):
    B = 131072
    raws = [oracle.synth(55, k, B, (1, 0, 2, 1, 0)[k % 5]) for k in range(64)]
    keys = [(1, fr.INT4, fr.GE, 1000), (1, fr.INT4, fr.LT, 9000)]
    return B, raws, keys, ar.agg_call(raws, SYNTH_ATTS, keys, ROWID + ROWID)


@pytest.mark.parametrize("method", METHODS)
def test_chunks_give_the_same_results(agg, oracle, sixty_four, method):
    B, raws, keys, want = sixty_four
    cols = ROWID + ROWID
    comps = [oracle_encode(oracle, method, r) for r in raws]
    comps[17] = comps[17][:len(comps[17]) - 9]
    rows, cells = want[0].copy(), want[1].copy()
    rows[17], cells[17] = (fr.STREAM, 0, 0, 0), (0, 0, 0, 0, 0)
    whole = agg_batch(agg, method, comps, B, SYNTH_ATTS, keys, cols)
    same(whole, (rows, cells), "one chunk")
    agg.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 2 << 20)                   # at most 15 decoded blocks of 128 KiB fit: five chunks or more
    got = agg_batch(agg, method, comps, B, SYNTH_ATTS, keys, cols)
    same(got, (rows, cells), "small budget")
    assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])
    same(host_call(agg, method, comps, B, SYNTH_ATTS, keys, cols), (rows, cells), "host buffers, small budget")
    agg.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- counters ----
@pytest.mark.parametrize("method", METHODS)
def test_transfer_and_codec_counters(agg, oracle, sixty_four, method):
    B, raws, keys, want = sixty_four
    raws, want = raws[:40], (want[0][:40], want[1][:40])
    comps = [oracle_encode(oracle, method, r) for r in raws]
    agg.set_option(cc.OPT_POOL_BYTES, 8 * B)
    for budget in (0, 4 << 20):
        agg.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
        for cols in (ROWID + ROWID, ROWID):
            before_t, before_c = agg.transfer_counters(), agg.counters()
            got = host_call(agg, method, comps, B, SYNTH_ATTS, keys, cols)
            after_t, after_c = agg.transfer_counters(), agg.counters()
            same(got, (want[0], want[1][:, :len(cols)]))
            assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 16 * 40 + 40 * 40 * len(cols)
            for k in ("pool_hits", "pool_misses", "pool_blocks"):
                assert after_t[k] == before_t[k], k
            assert after_c == before_c
    agg.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
    agg.set_option(cc.OPT_POOL_BYTES, 0)


# ---- several handles ----
def multi_agg(method, comps, B, atts, keys, cols, devices):
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    try:
        def chk(rc, what):
            assert rc == 0, (what, rc, L.cryo_multi_last_error(h))
        return cc.agg_blocks_call(L.cryo_multi_agg_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.agg_desc(cols))
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("devices", [(0,), (0, 0), (0, 1)])
def test_multi_agg_blocks(agg, oracle, sixty_four, devices):
    """one handle; two handles on one device; two devices: rows and cells in call order, equal to the single-device call"""
    if max(devices) >= cc.device_count():
        pytest.skip("one device visible")
    B, raws, keys, want = sixty_four
    raws = raws[:11]
    cols = ROWID + ROWID
    for method in METHODS:
        comps = [oracle_encode(oracle, method, r) for r in raws]
        comps[2] = comps[2][:40]
        rows, cells = want[0][:11].copy(), want[1][:11].copy()
        rows[2], cells[2] = (fr.STREAM, 0, 0, 0), (0, 0, 0, 0, 0)
        got = multi_agg(method, comps, B, SYNTH_ATTS, keys, cols, devices)
        same(got, (rows, cells), (method, devices))
        one = host_call(agg, method, comps, B, SYNTH_ATTS, keys, cols)
        assert np.array_equal(got[0], one[0]) and np.array_equal(got[1], one[1])
    rows, cells = multi_agg(METHOD_LZ4, [], B, SYNTH_ATTS, keys, cols, devices)
    assert rows.size == 0 and cells.shape[0] == 0


# ---- arguments ----
def test_descriptor_rules(agg, oracle):
    """every argument rule of the two descriptors, on host arrays (refused before a device is touched: the transfer counters
    stand still) and on device arrays"""
    B = ac.B
    arr = np.ascontiguousarray(oracle.lz4_compress(ac.range_block(), 1))
    L = agg.L
    src, szs = (C.c_void_p * 1)(arr.ctypes.data), (C.c_uint32 * 1)(arr.nbytes)
    rows, cells = np.zeros(1, cc.AGG_BLOCK), np.zeros(4, cc.AGG_CELL)
    bufs = [agg.alloc(6416), agg.alloc(96), agg.alloc(64), agg.alloc(4096), agg.alloc(8), agg.alloc(4), agg.alloc(16), agg.alloc(160)]
    d_atts, d_keys, d_cols, d_src, d_off, d_sz, d_rows, d_cells = bufs
    try:
        d_src.upload(np.concatenate([arr, np.zeros(4096 - arr.nbytes, np.uint8)]))
        d_off.upload(np.zeros(1, np.uint64))
        d_sz.upload(np.array([arr.nbytes], np.uint32))
        for name, atts, keys, cols, flags, patch, ok in ac.descriptors():
            assert ac.ref_ok(ar, atts, keys, cols, flags, patch) == ok, name
            f, a, k = cc.filter_desc(atts, keys, flags)
            g, c = cc.agg_desc(cols)
            if patch:
                which, field, index, value = patch
                if which == "f":
                    f.rsv = value
                elif which == "g":
                    g.rsv = value
                else:
                    {"a": a, "k": k, "c": c}[which][field][index] = value
            before = agg.transfer_counters()
            rc = L.cryo_codec_agg_blocks(agg.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), C.byref(g), rows.ctypes.data, cells.ctypes.data)
            assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
            if not ok:
                assert agg.transfer_counters() == before, name
            if len(atts):
                d_atts.upload(a)
            d_keys.upload(k)
            d_cols.upload(c)
            fd = cc.CryoFilter(f.natts, f.nkeys, f.flags, f.rsv, d_atts.ptr, d_keys.ptr if len(keys) else None)
            gd = cc.CryoAgg(g.ncols, g.rsv, d_cols.ptr)
            rc = L.cryo_codec_agg_batch(agg.h, METHOD_LZ4, d_src.ptr, d_off.ptr, d_sz.ptr, B, 1, C.byref(fd), C.byref(gd), d_rows.ptr,
                                        d_cells.ptr)
            agg.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    finally:
        for b in bufs:
            b.free()


def test_arguments(agg, oracle):
    comp = oracle.lz4_compress(oracle.synth(1, 0, 4096, 1), 1)
    d = [agg.alloc(512) for _ in range(8)]
    try:
        _, a, k = cc.filter_desc(SYNTH_ATTS, [(1, fr.INT4, fr.GE, 1), (1, fr.INT4, fr.LT, 5)])
        _, g = cc.agg_desc(ROWID)
        d[3].upload(a)
        d[4].upload(k)
        d[5].upload(g)

        class Shifted:                                                    # a device pointer that breaks the alignment rule
            def __init__(self, buf, by):
                self.ptr = buf.ptr + by

        def call(method=METHOD_LZ4, B=4096, n=1, natts=2, nkeys=2, ncols=1, cols=d[5], rows=d[6], cells=d[7]):
            agg.agg_batch(method, d[0], d[1], d[2], B, n, natts, d[3], nkeys, d[4], ncols, cols, rows, cells)

        for kw in (dict(method=7), dict(B=4092), dict(B=8), dict(B=0), dict(natts=0), dict(natts=1601), dict(nkeys=5), dict(ncols=0),
                   dict(ncols=5), dict(cols=None), dict(rows=None), dict(cells=None), dict(rows=Shifted(d[6], 8)),
                   dict(cells=Shifted(d[7], 4)), dict(cols=Shifted(d[5], 4))):
            with pytest.raises(CryoError) as e:
                call(**kw)
            assert e.value.code == cc.E_ARG, kw
        d[6].memset(0xEE)
        call(n=0)                                                         # no block: nothing is written
        agg.sync()
        assert (d[6].download() == 0xEE).all()
        bad = g.copy()
        bad["type"][0] = fr.INT8                                          # not the column's size, found in the device copy
        d[5].upload(bad)
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
    finally:
        for b in d:
            b.free()
    fdesc, adesc = cc.filter_desc(SYNTH_ATTS, []), cc.agg_desc(ROWID)
    with pytest.raises(CryoError) as e:
        agg.agg_blocks(METHOD_ZSTD, [comp], 4100, fdesc, adesc)
    assert e.value.code == cc.E_ARG
    rows, cells = agg.agg_blocks(METHOD_LZ4, [], 4096, fdesc, adesc)
    assert rows.size == 0 and cells.shape[0] == 0
    rows, cells = agg.agg_blocks(METHOD_LZ4, [comp], 4096, fdesc, adesc)
    assert rows["n_match"][0] == rows["n_items"][0] == cells["n"][0, 0] > 0
