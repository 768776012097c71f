"""GPU tests of the pattern scan keys (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE) in the device-resident calls: cryo_codec_filter_batch /
_agg_batch / _group_batch (plain, buckets, text) / _project_batch / _topn_batch.

Every row, record, cell and byte is compared with tests/like_ref.py, the plain-Python statement of the rules in
include/cryo_codec.h, applied to the blocks the ORACLE encoded; the hand-made blocks of tests/like_cases.py also carry their
expectations written out by hand.  Outputs are filled with a sentinel before every call, and after every device-resident call
the caller's key array -- after the filter's, the patterns too -- is read back: the library must not have written them.  On the
commit before the keys existed every call here is refused with CRYO_E_ARG."""
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
from like_ref import P
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import Device, Encoder, same_agg, same_filter, same_group, same_project
from test_gpu_bucket import batch as bucket_batch
from test_gpu_group_text import batch as text_batch, same_text

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
CASES = lc.cases()
SLICES = 4


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def columns(atts):
    """(aggregate columns, group columns, projected columns, order columns) of a descriptor of the cases: its integer columns"""
    ints = [(i, {4: lr.INT4, 8: lr.INT8}[attlen]) for i, (attlen, _) in enumerate(atts, 1) if attlen > 0]
    return ints, ints[:1], [i for i, _ in ints], [(ints[-1][0], ints[-1][1], 0)]


# ---- the hand-made blocks ----
@pytest.mark.parametrize("part", range(SLICES))
def test_crafted_blocks_filter(dev, enc, part):
    """every hand-made block in batches of 1, 4, 5 and 9 blocks, the methods alternating (every fifth case both): records and
    tuples, and COUNT_ONLY"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(CASES):
        if idx % SLICES != part:
            continue
        blocks = lk.batch(idx // SLICES, blk, B, atts)
        want = lr.filter_call(blocks, atts, keys, 0, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name       # block 0's, as written by hand
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        cwant = lr.filter_call(blocks, atts, keys, lr.COUNT_ONLY, W)
        for method in METHODS if idx % 5 == 0 else [METHODS[idx % 2]]:
            comps = [enc(method, b) for b in blocks]
            got = lk.filter_batch(dev, method, comps, B, atts, keys, 0, W, shift=idx % 8)
            same_filter(got, want, (name, method))
            first = got[1][:len(matches) + len(bad)]
            assert {int(r["pos"]): int(r["status"]) for r in first if r["status"]} == bad, name
            same_filter(lk.filter_batch(dev, method, comps, B, atts, keys, lr.COUNT_ONLY, W), cwant, (name, method, "count only"))


@pytest.mark.parametrize("part", range(SLICES))
def test_crafted_blocks_agg_group_project_and_topn(dev, enc, part):
    """the same blocks through the aggregate and the projection (1, 4, 5, 9 blocks), the grouped scan (1, 2, 3 blocks) and the
    ordered scan, the methods alternating"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(CASES):
        if idx % SLICES != part:
            continue
        method = METHODS[(idx // SLICES) % 2]
        cols, by, pcols, order = columns(atts)
        blocks = lk.batch(idx // SLICES, blk, B, atts)
        comps = [enc(method, b) for b in blocks]
        want = lr.agg_call(blocks, atts, keys, cols, W)
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        same_agg(tcall.agg_batch(dev, method, comps, B, atts, keys, cols, W), want, name)
        want = lr.project_call(blocks, atts, keys, pcols, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name
        same_project(tcall.project_batch(dev, method, comps, B, atts, keys, pcols, W), want, name)
        want = lr.topn_call(blocks, atts, keys, order, 7, pcols, W)
        topn_calls.same_topn(topn_calls.topn_batch(dev, method, comps, B, atts, keys, order, 7, pcols, truth=W), want, name)
        blocks = lk.batch(idx // SLICES, blk, B, atts, (1, 2, 3))
        comps = [enc(method, b) for b in blocks]
        want = lr.group_call(blocks, atts, keys, by, cols[1:], W)
        assert want[0]["n_match"][0] == len(matches), name
        same_group(tcall.group_batch(dev, method, comps, B, atts, keys, by, cols[1:], W), want, name)


# ---- one seeded random test per call ----
@pytest.fixture(scope="module")
def drawn():
    """{seed: (blocks, keys, truth)}: every block holds a match and a tuple that is none by the reference"""
    return {seed: lk.random_call(seed) for seed in range(1, 9)}


def test_random_filter(dev, enc, drawn):
    blocks, keys, W = drawn[1]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    same_filter(lk.filter_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, 0, W), lr.filter_call(blocks, lk.WIDE, keys, 0, W), "random")
    same_filter(lk.filter_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, lr.COUNT_ONLY, W),
                lr.filter_call(blocks, lk.WIDE, keys, lr.COUNT_ONLY, W), "random, count only")


def test_random_agg_integer_and_float_columns(dev, enc, drawn):
    blocks, keys, W = drawn[2]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    for cols in ([(3, lr.INT8), (5, lr.INT4)], [(6, lk.FLOAT8), (3, lr.INT8), (1, lr.INT4)]):
        want = lr.agg_call(blocks, lk.WIDE, keys, cols, W)
        assert (want[1]["n"][:, 0] > 0).all()
        same_agg(tcall.agg_batch(dev, METHOD_ZSTD, comps, lk.WIDE_B, lk.WIDE, keys, cols, W), want, ("random", cols))
    fkeys = keys[:1] + [(6, lk.FLOAT8, lr.LT, 1e200)]                       # beside a float key
    want = lr.agg_call(blocks, lk.WIDE, fkeys, [(3, lr.INT8)], None)
    assert 0 < want[0]["n_match"].sum() < want[0]["n_items"].sum()
    same_agg(tcall.agg_batch(dev, METHOD_ZSTD, comps, lk.WIDE_B, lk.WIDE, fkeys, [(3, lr.INT8)], None), want, "random, float key")


def test_random_group_plain_and_float(dev, enc, drawn):
    blocks, keys, W = drawn[3]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    for by, cols in (([(5, lr.INT4)], [(3, lr.INT8)]), ([(5, lr.INT4), (3, lr.INT8)], [(6, lk.FLOAT8), (1, lr.INT4)])):
        want = lr.group_call(blocks, lk.WIDE, keys, by, cols, W)
        assert (want[0]["n_groups"] > 1).all()
        same_group(tcall.group_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, by, cols, W), want, ("random", by))


def test_random_group_buckets(dev, enc, drawn):
    blocks, keys, W = drawn[4]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    by, cols, buckets = [(3, lr.INT8)], [(1, lr.INT4), (6, lk.FLOAT8)], [bk.width(-3, 10)]
    want = lr.bucket_group_call(blocks, lk.WIDE, keys, by, cols, buckets, W)
    assert (want[0]["n_groups"] > 1).all() and (want[0]["n_match"] > 0).all()
    same_group(bucket_batch(dev, METHOD_LZ4, comps, lk.WIDE, keys, by, cols, buckets, truth=W), want, "random, buckets")


def test_random_group_text(dev, enc, drawn):
    blocks, keys, W = drawn[5]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    by, cols = [(4, lr.BYTES), (5, lr.INT4)], [(3, lr.INT8), (6, lk.FLOAT8)]
    want = lr.text_group_call(blocks, lk.WIDE, keys, by, cols, W)
    assert (want[0]["n_groups"] > 1).all() and (want[0]["n_match"] > 0).all()
    same_text(text_batch(dev, METHOD_ZSTD, comps, keys, by, cols, truth=W, size=lk.WIDE_B), want, "random, text")


def test_random_project(dev, enc, drawn):
    blocks, keys, W = drawn[6]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    want = lr.project_call(blocks, lk.WIDE, keys, [6, 1, 3, 5], W)
    same_project(tcall.project_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, keys, [6, 1, 3, 5], W), want, "random")


def test_random_topn(dev, enc, drawn):
    blocks, keys, W = drawn[7]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    for by in ([(3, lr.INT8, cc.ORDER_DESC), (1, lr.INT4, 0)], [(6, lk.FLOAT8, 0), (1, lr.INT4, cc.ORDER_DESC)]):
        want = lr.topn_call(blocks, lk.WIDE, keys, by, 9, [1, 3, 6], W)
        assert want[3] == 9 * len(blocks)
        topn_calls.same_topn(topn_calls.topn_batch(dev, METHOD_ZSTD, comps, lk.WIDE_B, lk.WIDE, keys, by, 9, [1, 3, 6], truth=W), want, ("random", by))


# ---- the descriptor ----
def test_descriptor_rules_on_device_arrays(dev, enc):
    """the argument rules of a pattern key on device arrays; a trailing escape is found once the pattern has been read back,
    so with a block alone"""
    B = lc.B
    comp = np.ascontiguousarray(enc(METHOD_LZ4, tc.build_block(B, [lc.T(1, b"p", b"abc", 10, b"t")])))
    L = dev.L
    for name, atts, keys, key_rsv, ok in lc.descriptors():
        assert key_rsv is None and lr.desc_ok(atts, keys) == ok, name
        with Device(dev, [comp], atts, keys, shift=1) as d:
            d_dst, d_rec, d_tab, d_tot = d.alloc(B), d.alloc(8 * 290), d.alloc(32), d.alloc(16)
            g = cc.CryoFilter(len(atts), len(keys), 0, 0, d.atts.ptr, d.keys.ptr)
            rc = L.cryo_codec_filter_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(g), d_dst.ptr, B, d_rec.ptr,
                                           290, d_tab.ptr, d_tot.ptr)
            dev.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
            escape = any(lr.is_like_key(k) and isinstance(k[3], P) and lr.tokens(k[3].pattern or b"") is None for k in keys)
            rc = L.cryo_codec_filter_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 0, C.byref(g), d_dst.ptr, B, d_rec.ptr,
                                           290, d_tab.ptr, d_tot.ptr)
            dev.sync()
            assert rc == (cc.OK if ok or escape else cc.E_ARG), (name, "device arrays, no block", rc)
    # the other calls refuse what the filter refuses
    bad, comps, cols = [lc.K3(lr.LIKE, b"abc\\")], [comp], [(1, lr.INT4)]
    for call in (lambda: tcall.agg_batch(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, cols),
                 lambda: tcall.group_batch(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, cols, cols),
                 lambda: tcall.project_batch(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, [1]),
                 lambda: topn_calls.topn_batch(dev, METHOD_LZ4, comps, B, lc.ATTS, bad, [(1, lr.INT4, 0)], 3, [1])):
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG


def test_descriptors_without_a_pattern_key_are_what_they_were(dev, enc):
    """a pattern that every value matches beside the old keys, under a table that ignores it, gives the bytes of the call
    without it: the pattern kernels do what the others do"""
    blocks, _, _ = lk.random_call(8)
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    old = [(3, lr.INT8, lr.GE, -10), (4, lr.BYTES, lr.NE, b"us"), (6, lk.FLOAT8, lr.LT, 1e200)]
    new = old + [(2, lr.BYTES, lr.LIKE, P(b"%x%"))]
    W = lr.tr.and_table(3)                                                   # over four keys the same bits ignore keys[3] ...
    W4 = sum(1 << m for m in range(16) if m & 7 == 7)                        # ... spelled out: true when the three old keys are
    a = tcall.filter_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, old, 0, W)
    b = lk.filter_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, new, 0, W4)
    assert a[0]["n_match"].sum() > 0
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes() if isinstance(x, np.ndarray) else x == y
    cols = [(6, lk.FLOAT8), (3, lr.INT8)]
    same_agg(tcall.agg_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, new, cols, W4), tcall.agg_batch(dev, METHOD_LZ4, comps, lk.WIDE_B, lk.WIDE, old, cols, W))
