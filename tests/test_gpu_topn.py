"""GPU tests of the ordered scan (cryo_codec_topn_batch, cryo_codec_topn_blocks, cryo_multi_topn_blocks).

Every row of the block table, every record and every row byte is compared with tests/topn_ref.py, the plain-Python statement of the
rules in include/cryo_codec.h, applied to the ORACLE's decode of each stream.  The output buffers are filled with a sentinel before
every call: nothing at or beyond the total or the cap may be written.  The block kernel takes two waves per workgroup, so batches
of 1, 2, 3 and 5 blocks are a lone wave, a full workgroup, one over and two workgroups and a wave."""
import ctypes as C

import numpy as np
import pytest

import agg_ref as ar
import filter_ref as fr
import float_ref as fl
import large_scan_cases as ls
import topn_cases as tcs
import topn_ref as tr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import project_batch
from topn_calls import same_multi, same_topn as same, topn_batch, topn_host, topn_multi

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def top(codec):
    yield codec
    for opt, v in ((cc.OPT_WORKSPACE_MAX_BYTES, 0), (cc.OPT_POOL_BYTES, 0)):
        codec.set_option(opt, v)


class Streams:
    """the oracle's stream of a block, encoded once per method for the whole module"""

    def __init__(self, oracle):
        self.oracle, self.seen = oracle, {}

    def __call__(self, method, block):
        key = (method, block.tobytes())
        if key not in self.seen:
            self.seen[key] = self.oracle.lz4_compress(block, 1) if method == METHOD_LZ4 else self.oracle.zstd_compress(block, 1)
        return self.seen[key]


@pytest.fixture(scope="module")
def enc(oracle):
    return Streams(oracle)


def both(codec, enc, blocks, B, atts, keys, by, limit, cols, what, methods=METHODS, truth=None, want=None):
    """device buffers and host buffers, on the oracle's streams of `blocks`, against topn_ref; returns the expectation"""
    want = want or tr.topn_call(blocks, atts, keys, by, limit, cols, truth)
    for method in methods:
        comps = [enc(method, b) for b in blocks]
        same(topn_batch(codec, method, comps, B, atts, keys, by, limit, cols, truth=truth), want, (what, limit, method))
        same(topn_host(codec, method, comps, B, atts, keys, by, limit, cols, truth=truth), want, (what, limit, method, "host buffers"))
    return want


# ---- the crafted blocks: orders, flags, NULLs, extremes, floats, filter kinds ----
@pytest.mark.parametrize("nb", [1, 2, 3, 5])
def test_crafted_blocks(top, enc, nb):
    """crafted blocks alternate with the block of the filter-kind cases; the hand-made order holds wherever the block stands"""
    other = tcs.named_block()
    for name, B, atts, block, keys, by, cols, order, keys_at in tcs.cases():
        blocks = [block if i % 2 == 0 else other for i in range(nb)]
        for limit, methods in ((2, METHODS), (1000, [METHOD_LZ4])):
            want = tr.topn_call(blocks, atts, keys, by, limit, cols)
            for i in range(0, nb, 2):
                kept = tr.kept_of(*want[:3], i)
                assert [k[3] for k in kept] == order[:limit], name
                assert all(k[:3] == keys_at[k[3]] for k in kept if k[3] in keys_at), name
            both(top, enc, blocks, B, atts, keys, by, limit, cols, (name, nb), methods, want=want)


def test_filter_kinds_and_their_kernels(top, enc):
    """no key, an integer range (k_topn_block<false>), a set key, a byte-string key with an undecided value and a truth table
    (k_topn_block<true>), a float key (k_topnf_block); the undecided tuple counts in n_bad and is not ranked"""
    by = [(tcs.K, fr.INT8, tcs.DESC)]
    block, und = tcs.named_block(), tcs.named_block(True)
    w = both(top, enc, [block], tcs.B, tcs.ATTS, [], by, 4, tcs.COLS, "no key")
    assert w[1]["pos"].tolist() == [6, 1, 2, 3]
    bkey = [(tcs.NAME, tr.br.BYTES, fl.GE, b"c")]
    w = both(top, enc, [und, block], tcs.B, tcs.ATTS, bkey, by, 10, tcs.COLS, "undecided")
    assert w[1]["pos"].tolist() == [6, 4, 5, 6, 3, 4, 5] and w[0]["n_bad"].tolist() == [1, 0] and w[0]["n_match"].tolist() == [3, 4]
    keys, truth, order = tcs.truth_case()
    w = both(top, enc, [block], tcs.B, tcs.ATTS, keys, by, 10, tcs.COLS, "truth table", truth=truth)
    assert w[1]["pos"].tolist() == order
    w = both(top, enc, [block, und], tcs.B, tcs.ATTS, [(tcs.X, fl.FLOAT8, fl.GT, 7.5)], [(tcs.X, fl.FLOAT8, 0), (tcs.K, fr.INT8, 0)], 2,
             tcs.COLS, "float key")
    assert w[1]["pos"].tolist() == [2, 1, 2, 1]


# ---- the turns of a wave and the limits ----
@pytest.mark.parametrize("limit", tcs.LIMITS)
def test_turns_and_limits(top, enc, limit):
    """0, 1, 63, 64, 65, 128, 129 and 290 items per block under every limit: keys repeat and every fifth is NULL, so ties are
    broken by position in every turn; two order columns with all four flags between them"""
    blocks = [tcs.turn_block(n) for n in tcs.TURN_SIZES]
    by = [(2, fr.INT8, tcs.DESC | tcs.NULLS_FIRST), (1, fr.INT4, 0)] if limit % 2 else [(2, fr.INT8, 0), (1, fr.INT4, tcs.DESC)]
    w = both(top, enc, blocks, tcs.TURN_B, tcs.TURN_ATTS, [], by, limit, tcs.TURN_COLS, "turns", [METHOD_LZ4])
    assert w[0]["n_match"].tolist() == list(tcs.TURN_SIZES) and w[0]["n_rows"].tolist() == [min(n, limit) for n in tcs.TURN_SIZES]


def test_every_key_equal_is_position_order(top, enc):
    import tuple_craft as tc
    atts = tcs.TURN_ATTS
    blocks = [tc.build_block(tcs.TURN_B, [tc.form_tuple(atts, [p, 7]) for p in range(1, n + 1)]) for n in (290, 129)]
    for flags in tcs.FLAG_SETS:
        w = both(top, enc, blocks, tcs.TURN_B, atts, [], [(2, fr.INT8, flags)], 200, tcs.TURN_COLS, ("equal", flags), [METHOD_LZ4])
        assert w[1]["pos"].tolist() == list(range(1, 201)) + list(range(1, 130))


def test_strictly_ascending_and_descending_input(top, enc):
    import tuple_craft as tc
    atts = tcs.TURN_ATTS
    up = tc.build_block(tcs.TURN_B, [tc.form_tuple(atts, [p, p - 150]) for p in range(1, 291)])
    down = tc.build_block(tcs.TURN_B, [tc.form_tuple(atts, [p, 150 - p]) for p in range(1, 291)])
    for flags, first in ((0, [1, 290]), (tcs.DESC, [290, 1])):
        w = both(top, enc, [up, down], tcs.TURN_B, atts, [], [(2, fr.INT8, flags)], 65, tcs.TURN_COLS, ("monotone", flags), [METHOD_ZSTD])
        assert [int(w[1]["pos"][0]), int(w[1]["pos"][65])] == first


# ---- blocks without an answer, bad items ----
def test_stream_and_header_blocks_and_bad_items(top, enc, oracle):
    good, bad = tcs.named_block(), tcs.bad_items_block()
    blocks = [good, None, tcs.header_block(), bad, None, good]
    by = [(tcs.K, fr.INT8, 0)]
    want = tr.topn_call(blocks, tcs.ATTS, [], by, 3, tcs.COLS)
    assert want[0]["status"].tolist() == [0, fr.STREAM, fr.HEADER, 0, fr.STREAM, 0] and want[0]["row_first"].tolist() == [0, 3, 3, 3, 6, 6]
    assert want[0]["n_bad"].tolist() == [0, 0, 0, 2, 0, 0] and want[1]["pos"][3:6].tolist() == [5, 3, 1]
    for method in METHODS:
        comps = [enc(method, good if b is None else b) for b in blocks]
        comps[1] = comps[1][:len(comps[1]) - 7]                            # truncated streams
        comps[4] = comps[4][:len(comps[4]) // 2]
        assert [ar.decode(oracle, method, c, tcs.B) is None for c in comps] == [b is None for b in blocks]
        same(topn_batch(top, method, comps, tcs.B, tcs.ATTS, [], by, 3, tcs.COLS), want, method)
        same(topn_host(top, method, comps, tcs.B, tcs.ATTS, [], by, 3, tcs.COLS), want, (method, "host"))


# ---- caps ----
def test_caps(top, enc):
    """row_cap cuts inside a block, at a block's edge and at 0: the total is counted in full, nothing at or beyond the cap is
    written (topn_batch checks the sentinel), and the host-buffer call answers CRYO_E_DSTSIZE"""
    blocks = [tcs.turn_block(65), tcs.turn_block(1), tcs.turn_block(129)]
    by = [(2, fr.INT8, 0)]
    want = tr.topn_call(blocks, tcs.TURN_ATTS, [], by, 64, tcs.TURN_COLS)
    need = want[3]
    assert need == 64 + 1 + 64
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        same(topn_host(top, method, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 64, tcs.TURN_COLS, need), want, "exactly the need")
        for cap in (need - 1, 70, 65, 64, 0):
            with pytest.raises(CryoError) as e:
                topn_host(top, method, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 64, tcs.TURN_COLS, cap)
            assert e.value.code == cc.E_DSTSIZE, cap
            table, rec, rows, total = topn_batch(top, method, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 64, tcs.TURN_COLS, cap)
            assert total == need and len(rec) == cap and len(rows) == cap
            same((table, rec, rows, need), (want[0], want[1][:cap], want[2][:cap], need), ("cut at", cap))


# ---- several chunks ----
@pytest.mark.parametrize("method", METHODS)
def test_chunks_give_the_same_bytes(top, enc, method):
    """40 blocks of 16 KiB under a budget of 256 KiB are several chunks (a block takes its 16 KiB decoded and 290 x 44 bytes of
    side area), the running total carried in device memory between them"""
    blocks = [tcs.turn_block(tcs.TURN_SIZES[i % 8]) for i in range(40)]
    by = [(2, fr.INT8, tcs.DESC)]
    want = tr.topn_call(blocks, tcs.TURN_ATTS, [], by, 10, tcs.TURN_COLS)
    comps = [enc(method, b) for b in blocks]
    whole = topn_batch(top, method, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 10, tcs.TURN_COLS)
    same(whole, want, "one chunk")
    top.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 256 << 10)
    same(topn_batch(top, method, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 10, tcs.TURN_COLS), want, "small budget")
    same(topn_host(top, method, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 10, tcs.TURN_COLS), want, "small budget, host buffers")
    top.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- without a reference: an ordered projection of every match ----
@pytest.mark.parametrize("limit", [290, 1000])
def test_rows_resorted_by_position_are_the_projection(top, enc, limit):
    blocks = [tcs.turn_block(290), tcs.turn_block(64), tcs.turn_block(129)]
    by = [(2, fr.INT8, tcs.DESC), (1, fr.INT4, tcs.DESC)]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    table, rec, rows, total = topn_batch(top, METHOD_LZ4, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, limit, tcs.TURN_COLS)
    ptable, prec, prows, (pw, _) = project_batch(top, METHOD_LZ4, comps, tcs.TURN_B, tcs.TURN_ATTS, [], tcs.TURN_COLS)
    assert total == pw == 290 + 64 + 129
    for i in range(3):
        at, k = int(table["row_first"][i]), int(table["n_rows"][i])
        assert at == int(ptable["row_first"][i]) and k == int(ptable["n_match"][i])
        back = np.argsort(rec["pos"][at:at + k], kind="stable")
        assert np.array_equal(rows[at:at + k][back], prows[at:at + k]) and np.array_equal(rec["pos"][at:at + k][back], prec["pos"][at:at + k])


# ---- a block above 1 MiB ----
def test_large_block(top, enc):
    B = ls.MIB + 8
    tuples = [ls.row(i, ls.text(3400 + i % 7), (i * 7919) % 257 - 128 if i % 11 else None, i % 5, float(i % 13) - 6.5) for i in range(1, 291)]
    block = ls.block_of(B, tuples)
    by = [(ls.K, fr.INT8, tcs.DESC), (ls.X, fl.FLOAT8, tcs.NULLS_FIRST)]
    w = both(top, enc, [block], B, ls.ATTS, [(ls.G, fr.INT2, fr.NE, 2)], by, 100, [ls.ID, ls.K, ls.X], "large block")
    assert int(w[0]["n_items"][0]) == 290 and int(w[0]["n_match"][0]) == 232 and w[3] == 100


# ---- workspace history ----
def test_hostile_workspace(top, enc):
    blocks = [tcs.turn_block(n) for n in (129, 290, 65)]
    by = [(2, fr.INT8, tcs.NULLS_FIRST), (1, fr.INT4, tcs.DESC)]
    want = tr.topn_call(blocks, tcs.TURN_ATTS, [], by, 70, tcs.TURN_COLS)
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    same(topn_host(top, METHOD_ZSTD, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 70, tcs.TURN_COLS), want, "sizing run")
    for value in (0x00, 0xFF, 0x01, 0xA5):
        top.debug_fill(value)
        same(topn_batch(top, METHOD_ZSTD, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 70, tcs.TURN_COLS), want, ("after a fill", value))
        top.debug_fill(value)
        same(topn_host(top, METHOD_ZSTD, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, 70, tcs.TURN_COLS), want, ("after a fill, host", value))


# ---- several handles ----
@pytest.mark.parametrize("G", [2, 3])
def test_multi(enc, G):
    blocks = [tcs.turn_block(tcs.TURN_SIZES[(3 * i + 1) % 8]) for i in range(7)]
    by = [(2, fr.INT8, tcs.DESC)]
    for limit in (5, 1000):
        want = tr.multi_call(blocks, tcs.TURN_ATTS, [], by, limit, tcs.TURN_COLS, G)
        comps = [enc(METHOD_LZ4, b) for b in blocks]
        same_multi(topn_multi(G, METHOD_LZ4, comps, tcs.TURN_B, tcs.TURN_ATTS, [], by, limit, tcs.TURN_COLS), want, limit, (G, limit))


# ---- arguments ----
def test_descriptor_rules_on_device_arrays(top, enc):
    comp = np.ascontiguousarray(enc(METHOD_LZ4, tcs.named_block()))
    bufs = [top.alloc(6416), top.alloc(96), top.alloc(64), top.alloc(64), top.alloc(4096), top.alloc(8), top.alloc(4), top.alloc(32),
            top.alloc(24 * 290), top.alloc(64 * 290), top.alloc(8), top.alloc(64)]
    d_atts, d_keys, d_by, d_cols, d_src, d_off, d_sz, d_table, d_rec, d_rows, d_total, d_consts = bufs
    try:
        d_src.upload(np.concatenate([comp, np.zeros(4096 - comp.nbytes, np.uint8)]))
        d_off.upload(np.zeros(1, np.uint64))
        d_sz.upload(np.array([comp.nbytes], np.uint32))
        for name, atts, keys, by, limit, cols, patch, ok in tcs.descriptors():
            if not by or not cols:
                continue                                                  # an empty array has no device copy: test_arguments
            da, dk, consts, rebase = cc.filter_desc_device(atts, keys)
            (o, oa), (p, pa) = cc.order_desc(by, limit), cc.project_desc(cols)
            if patch:
                which, index, value = patch
                if which == "p":
                    p.rsv = value
                else:
                    {"b": oa, "c": pa}[which]["rsv" if which == "b" else "rsv2"][index] = value
            d_atts.upload(da)
            d_keys.upload(rebase(d_consts.ptr))
            d_by.upload(oa)
            d_cols.upload(pa)
            fd = cc.CryoFilter(len(atts), len(keys), 0, 0, d_atts.ptr, d_keys.ptr if len(keys) else None)
            od, pd = cc.CryoOrder(o.nby, o.limit, d_by.ptr), cc.CryoProject(p.ncols, p.rsv, d_cols.ptr)
            rc = top.L.cryo_codec_topn_batch(top.h, METHOD_LZ4, d_src.ptr, d_off.ptr, d_sz.ptr, tcs.B, 1, C.byref(fd), C.byref(od), C.byref(pd),
                                             d_rows.ptr, d_rec.ptr, 290, d_table.ptr, d_total.ptr)
            top.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
    finally:
        for x in bufs:
            x.free()


def test_arguments(top, enc):
    comp = enc(METHOD_LZ4, tcs.named_block())
    fdesc, odesc, pdesc = cc.filter_desc(tcs.ATTS, []), cc.order_desc([(tcs.K, fr.INT8, 0)], 3), cc.project_desc(tcs.COLS)
    with pytest.raises(CryoError) as e:
        top.topn_blocks(METHOD_ZSTD, [comp], 4100, fdesc, odesc, pdesc, 16)
    assert e.value.code == cc.E_ARG
    table, rec, rows, total = top.topn_blocks(METHOD_LZ4, [], 4096, fdesc, odesc, pdesc, 16)
    assert table.size == 0 and total == 0
    table, rec, rows, total = top.topn_blocks(METHOD_LZ4, [comp], 4096, fdesc, odesc, pdesc, 16)
    assert total == 3 and rec["pos"][:3].tolist() == [5, 4, 3] and rec["key"][:3, 0].tolist() == [10, 20, 30]
