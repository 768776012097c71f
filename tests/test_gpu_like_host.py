"""GPU tests of the pattern scan keys (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE) in the host-buffer calls -- cryo_codec_filter_blocks /
_agg_blocks / _group_blocks (plain, buckets, text) / _project_blocks / _topn_blocks -- and in cryo_multi_*_blocks with two handles.

Every row, record, cell and byte is compared with tests/like_ref.py on the blocks the ORACLE encoded, as in
tests/test_gpu_like.py, whose hand-made blocks, batches and seeded random calls these are; the host buffers are filled with a
sentinel before every call.  In this form a pattern with a trailing escape is refused before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import bucket_ref as bk
import like_calls as lk
import like_cases as lc
import like_ref as lr
import topn_calls
import truth_calls as tcall
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import REC_SENTINEL, SENTINEL, Encoder, multi_call, same_agg, same_fields, same_filter, same_group, same_project
from test_gpu_bucket import hosted as bucket_hosted
from test_gpu_group_text import hosted as text_hosted, multi as text_multi, same_text
from test_gpu_like import CASES, SLICES, columns

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


# ---- the hand-made blocks ----
@pytest.mark.parametrize("part", range(SLICES))
def test_crafted_blocks_filter(dev, enc, part):
    """every hand-made block in batches of 1, 4, 5 and 9 blocks, the methods alternating the other way round than in the
    device-resident test: records and tuples, and COUNT_ONLY"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(CASES):
        if idx % SLICES != part:
            continue
        blocks = lk.batch(idx // SLICES, blk, B, atts)
        want, cwant = lr.filter_call(blocks, atts, keys, 0, W), lr.filter_call(blocks, atts, keys, lr.COUNT_ONLY, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name       # block 0's, as written by hand
        method = METHODS[(idx + 1) % 2]
        comps = [enc(method, b) for b in blocks]
        got = tcall.filter_host(dev, method, comps, B, atts, keys, 0, W)
        same_filter(got, want, (name, method))
        assert {int(r["pos"]): int(r["status"]) for r in got[1][:len(matches) + len(bad)] if r["status"]} == bad, name
        same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, lr.COUNT_ONLY, W), cwant, (name, method, "count only"))


@pytest.mark.parametrize("part", range(SLICES))
def test_crafted_blocks_agg_group_project_and_topn(dev, enc, part):
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(CASES):
        if idx % SLICES != part:
            continue
        method = METHODS[(idx // SLICES + 1) % 2]
        cols, by, pcols, order = columns(atts)
        blocks = lk.batch(idx // SLICES, blk, B, atts)
        comps = [enc(method, b) for b in blocks]
        want = lr.agg_call(blocks, atts, keys, cols, W)
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        same_agg(tcall.agg_host(dev, method, comps, B, atts, keys, cols, W), want, name)
        same_project(tcall.project_host(dev, method, comps, B, atts, keys, pcols, W), lr.project_call(blocks, atts, keys, pcols, W), name)
        want = lr.topn_call(blocks, atts, keys, order, 7, pcols, W)
        topn_calls.same_topn(topn_calls.topn_host(dev, method, comps, B, atts, keys, order, 7, pcols, truth=W), want, name)
        blocks = lk.batch(idx // SLICES, blk, B, atts, (1, 2, 3))
        comps = [enc(method, b) for b in blocks]
        same_group(tcall.group_host(dev, method, comps, B, atts, keys, by, cols[1:], W), lr.group_call(blocks, atts, keys, by, cols[1:], W), name)


# ---- one seeded random test per call: the draws of tests/test_gpu_like.py ----
@pytest.fixture(scope="module")
def drawn():
    return {seed: lk.random_call(seed) for seed in range(1, 8)}


def test_random_filter(dev, enc, drawn):
    blocks, keys, W = drawn[1]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    same_filter(tcall.filter_host(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, 0, W), lr.filter_call(blocks, lk.WIDE, keys, 0, W), "random")
    same_filter(tcall.filter_host(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, lr.COUNT_ONLY, W),
                lr.filter_call(blocks, lk.WIDE, keys, lr.COUNT_ONLY, W), "random, count only")


def test_random_agg_integer_and_float_columns(dev, enc, drawn):
    blocks, keys, W = drawn[2]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    for cols in ([(3, lr.INT8), (5, lr.INT4)], [(6, lk.FLOAT8), (3, lr.INT8), (1, lr.INT4)]):
        same_agg(tcall.agg_host(dev, METHOD_ZSTD, comps, lk.WIDE_B, lk.WIDE, keys, cols, W), lr.agg_call(blocks, lk.WIDE, keys, cols, W), ("random", cols))


def test_random_group_plain_and_float(dev, enc, drawn):
    blocks, keys, W = drawn[3]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    for by, cols in (([(5, lr.INT4)], [(3, lr.INT8)]), ([(5, lr.INT4), (3, lr.INT8)], [(6, lk.FLOAT8), (1, lr.INT4)])):
        same_group(tcall.group_host(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, by, cols, W), lr.group_call(blocks, lk.WIDE, keys, by, cols, W),
                   ("random", by))


def test_random_group_buckets(dev, enc, drawn):
    blocks, keys, W = drawn[4]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    by, cols, buckets = [(3, lr.INT8)], [(1, lr.INT4), (6, lk.FLOAT8)], [bk.width(-3, 10)]
    same_group(bucket_hosted(dev, METHOD_LZ4, comps, lk.WIDE, keys, by, cols, buckets, truth=W),
               lr.bucket_group_call(blocks, lk.WIDE, keys, by, cols, buckets, W), "random, buckets")


def test_random_group_text(dev, enc, drawn):
    blocks, keys, W = drawn[5]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    by, cols = [(4, lr.BYTES), (5, lr.INT4)], [(3, lr.INT8), (6, lk.FLOAT8)]
    same_text(text_hosted(dev, METHOD_ZSTD, comps, keys, by, cols, truth=W, size=lk.WIDE_B), lr.text_group_call(blocks, lk.WIDE, keys, by, cols, W),
              "random, text")


def test_random_project(dev, enc, drawn):
    blocks, keys, W = drawn[6]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    same_project(tcall.project_host(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, [6, 1, 3, 5], W),
                 lr.project_call(blocks, lk.WIDE, keys, [6, 1, 3, 5], W), "random")


def test_random_topn(dev, enc, drawn):
    blocks, keys, W = drawn[7]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    for by in ([(3, lr.INT8, cc.ORDER_DESC), (1, lr.INT4, 0)], [(6, lk.FLOAT8, 0), (1, lr.INT4, cc.ORDER_DESC)]):
        want = lr.topn_call(blocks, lk.WIDE, keys, by, 9, [1, 3, 6], W)
        topn_calls.same_topn(topn_calls.topn_host(dev, METHOD_ZSTD, comps, lk.WIDE_B, lk.WIDE, keys, by, 9, [1, 3, 6], truth=W), want, ("random", by))


# ---- two handles ----
def test_multi_with_two_handles(enc, drawn):
    """cryo_multi_agg_blocks, _filter_blocks (COUNT_ONLY) and _group_blocks with a text group column, two handles on device 0"""
    blocks, keys, W = drawn[5]
    blocks = blocks + blocks[:2]                                             # five blocks: shares of three and two
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    cols = [(3, lr.INT8), (6, lk.FLOAT8)]
    same_agg(multi_call([0, 0], lambda L, h, chk: cc.agg_blocks_call(L.cryo_multi_agg_blocks, h, chk, METHOD_LZ4, comps, lk.WIDE_B,
                                                                       cc.filter_desc(lk.WIDE, keys, 0, W), cc.agg_desc(cols))),
             lr.agg_call(blocks, lk.WIDE, keys, cols, W), "two handles")
    ctab = multi_call([0, 0], lambda L, h, chk: cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, METHOD_LZ4, comps, lk.WIDE_B,
                                                                        cc.filter_desc(lk.WIDE, keys, lr.COUNT_ONLY, W)))[0]
    same_fields(ctab, lr.filter_call(blocks, lk.WIDE, keys, lr.COUNT_ONLY, W)[0], "two handles, count only")
    by = [(4, lr.BYTES), (5, lr.INT4)]
    same_text(text_multi((0, 0), METHOD_LZ4, comps, keys, by, cols, truth=W, size=lk.WIDE_B), lr.text_group_call(blocks, lk.WIDE, keys, by, cols, W),
              "two handles, text groups")


# ---- the descriptor ----
def test_descriptor_rules_on_host_arrays(dev, enc):
    B = lc.B
    comp = np.ascontiguousarray(enc(METHOD_LZ4, tc.build_block(B, [lc.T(1, b"p", b"abc", 10, b"t")])))
    L = dev.L
    src, szs = (C.c_void_p * 1)(comp.ctypes.data), (C.c_uint32 * 1)(comp.nbytes)
    dst, rec, table, tot = np.zeros(B, np.uint8), np.zeros(290, cc.FILTER_REC), np.zeros(1, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
    for name, atts, keys, key_rsv, ok in lc.descriptors():
        f, a, k = cc.filter_desc(atts, keys)
        before = k.copy(), bytes(f.consts)
        for n in (1, 0):                                                     # without a block the descriptor is checked all the same
            rc = L.cryo_codec_filter_blocks(dev.h, METHOD_LZ4, src, szs, n, B, C.byref(f), dst.ctypes.data, dst.nbytes, rec.ctypes.data,
                                            rec.size, table.ctypes.data, tot)
            assert rc == (cc.OK if ok else cc.E_ARG), (name, n, rc)
        assert np.array_equal(k, before[0]) and bytes(f.consts) == before[1], name                  # the caller's memory is only read
    bad, comps, cols = [lc.K3(lr.NOT_LIKE, b"abc\\")], [comp], [(1, lr.INT4)]
    for call in (lambda: tcall.agg_host(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, cols),
                 lambda: tcall.group_host(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, cols, cols),
                 lambda: tcall.project_host(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, [1]),
                 lambda: topn_calls.topn_host(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, [(1, lr.INT4, 0)], 3, [1])):
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
