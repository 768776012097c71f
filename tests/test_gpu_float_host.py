"""GPU tests of the float scan keys and float aggregate columns in the host-buffer calls cryo_codec_filter_blocks / _agg_blocks /
_group_blocks / _project_blocks and in cryo_multi_*_blocks, and of the blocks' cells combined on the host.

Every row, record, cell and byte is compared with tests/float_ref.py applied to the blocks the ORACLE encoded; the device-resident
calls are test_gpu_float.py's."""
import numpy as np
import pytest

import float_cases as fc
import float_ref as fl
import truth_calls as tcall
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc
from scan_calls import REC_SENTINEL, SENTINEL, Encoder, multi_call, same_agg, same_filter, same_group, same_project
from test_gpu_float import BY, COLS, PCOLS, batch, cell_words

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


@pytest.fixture(scope="module")
def random_blocks():
    return fc.random_blocks()


def test_crafted_blocks_host_buffers(dev, enc):
    """every third hand-made block in batches of 1, 4, 5 and 9 blocks through the four host-buffer calls"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(fc.cases()):
        if idx % 3 and W is None:
            continue
        method = METHODS[idx % 2]
        blocks = batch(idx, blk, B)
        comps = [enc(method, b) for b in blocks]
        want = fl.filter_call(blocks, atts, keys, 0, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name
        same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, 0, W), want, name)
        cwant = fl.filter_call(blocks, atts, keys, fl.COUNT_ONLY, W)
        same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, fl.COUNT_ONLY, W), cwant, (name, "count only"))
        same_agg(tcall.agg_host(dev, method, comps, B, atts, keys, COLS, W), fl.agg_call(blocks, atts, keys, COLS, W), name)
        same_project(tcall.project_host(dev, method, comps, B, atts, keys, PCOLS, W), fl.project_call(blocks, atts, keys, PCOLS, W), name)
        blocks = batch(idx, blk, B, (1, 2, 3))
        comps = [enc(method, b) for b in blocks]
        same_group(tcall.group_host(dev, method, comps, B, atts, keys, BY, COLS, W), fl.group_call(blocks, atts, keys, BY, COLS, W), name)


def test_crafted_sums_host_buffers_and_combined(dev, enc):
    """the hand-written sums through cryo_codec_agg_blocks, one block each in one call; the blocks' cells combined in block order
    (codec.cell_float_combine) are what the reference's combination gives"""
    blocks = [fc.sum_block(values) for _, values, _ in fc.SUM_CASES]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    rows, cells = tcall.agg_host(dev, METHOD_ZSTD, comps, fc.SUM_B, fc.ATTS, fc.SUM_KEYS, fc.SUM_COLS)
    same_agg((rows, cells), fl.agg_call(blocks, fc.ATTS, fc.SUM_KEYS, fc.SUM_COLS), "sums")
    for i, (name, _, expect) in enumerate(fc.SUM_CASES):
        assert cell_words(cells[i, 0]) == fc.words(expect), name
    finite = [i for i, (name, _, e) in enumerate(fc.SUM_CASES) if isinstance(e[3], float) and abs(e[3]) != fc.INF]
    for picked in (finite, list(range(len(blocks)))):
        total, want = (0, 0.0, 0.0, 0.0, 0.0), (0, 0, 0, 0, 0)
        for i in picked:
            total = cc.cell_float_combine(total, cc.cell_float(cells[i, 0]))
            want = fl.combine_words(want, cell_words(cells[i, 0]))
        assert fc.words(total) == want
    assert fc.words(total)[3:] == (fl.NAN_BITS, 0)                                  # a NaN among all the blocks


def test_random_tuples_host_buffers(dev, enc, random_blocks):
    blocks, atts = random_blocks, fc.ATTS
    for turn, (keys, W, cols) in enumerate(fc.random_descriptors()[:6]):
        method = METHODS[turn % 2]
        comps = [enc(method, b) for b in blocks]
        same_filter(tcall.filter_host(dev, method, comps, fc.B, atts, keys, 0, W), fl.filter_call(blocks, atts, keys, 0, W), keys)
        same_agg(tcall.agg_host(dev, method, comps, fc.B, atts, keys, cols, W), fl.agg_call(blocks, atts, keys, cols, W), (keys, cols))
        same_group(tcall.group_host(dev, method, comps, fc.B, atts, keys, BY, cols, W), fl.group_call(blocks, atts, keys, BY, cols, W), (keys, cols))
        same_project(tcall.project_host(dev, method, comps, fc.B, atts, keys, PCOLS, W), fl.project_call(blocks, atts, keys, PCOLS, W), keys)


def test_chunks_host_buffers(dev, enc, random_blocks):
    """a workspace cap that forces several internal chunks: the pinned copy of the mapped keys serves them all"""
    blocks, atts = random_blocks, fc.ATTS
    keys = [(2, fl.FLOAT8, fl.LE, 0.5), (5, fl.FLOAT4, fl.NE, 0.0)]
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 64 << 10)
    want = fl.filter_call(blocks, atts, keys)
    assert want[0]["n_match"][12:].sum() > 0
    same_filter(tcall.filter_host(dev, METHOD_ZSTD, comps, fc.B, atts, keys), want, "small budget")
    same_agg(tcall.agg_host(dev, METHOD_ZSTD, comps, fc.B, atts, keys, COLS), fl.agg_call(blocks, atts, keys, COLS), "small budget")
    same_group(tcall.group_host(dev, METHOD_ZSTD, comps, fc.B, atts, keys, BY, COLS), fl.group_call(blocks, atts, keys, BY, COLS), "small budget")
    same_project(tcall.project_host(dev, METHOD_ZSTD, comps, fc.B, atts, keys, PCOLS), fl.project_call(blocks, atts, keys, PCOLS), "small budget")


def test_multi_handles(dev, enc, random_blocks):
    """one handle, and two handles on one device: the aggregate's and the grouping's outputs do not depend on the split; the
    filter's and the projection's tables do not either"""
    blocks = random_blocks[:11]
    B, atts = fc.B, fc.ATTS
    keys, W = [(2, fl.FLOAT8, fl.GT, -2.0), (3, fl.FLOAT4, fl.LT, fc.NAN), (6, fl.INT8, fl.GE, 0)], fl.tr.dnf([1, 6], 3)
    rb = fl.sr.pr.row_layout(atts, PCOLS)[1]
    for devices in [(0,), (0, 0)]:
        method = METHODS[len(devices) - 1]
        comps = [enc(method, b) for b in blocks]
        n = len(comps)
        same_agg(multi_call(devices, lambda L, h, chk: cc.agg_blocks_call(
            L.cryo_multi_agg_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W), cc.agg_desc(COLS))),
            fl.agg_call(blocks, atts, keys, COLS, W), devices)
        same_group(multi_call(devices, lambda L, h, chk: cc.group_blocks_call(
            L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W), cc.group_desc(BY), cc.agg_desc(COLS))),
            fl.group_call(blocks, atts, keys, BY, COLS, W), devices)
        table, recs, dst, total = multi_call(devices, lambda L, h, chk: cc.filter_blocks_call(
            L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W),
            np.full(n * B, SENTINEL, np.uint8), np.full(n * 290, REC_SENTINEL, cc.FILTER_REC)))
        want = fl.filter_call(blocks, atts, keys, 0, W)
        rows = np.full((290 * n, rb), SENTINEL, np.uint8)
        rec = np.full(8 * 290 * n, SENTINEL, np.uint8).view(cc.PROJECT_REC)
        ptab, prec, prows, (tw, tr) = multi_call(devices, lambda L, h, chk: cc.project_blocks_call(
            L.cryo_multi_project_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W), cc.project_desc(PCOLS), rb, rows, rec))
        pwant = fl.project_call(blocks, atts, keys, PCOLS, W)
        if len(devices) == 1:
            same_filter((table, recs, dst, total), want, devices)
            same_project((ptab, prec[:tr], prows[:tw], (tw, tr)), pwant, devices)
        else:
            for f in ("status", "n_items", "n_match", "n_bad"):
                assert np.array_equal(table[f], want[0][f]) and np.array_equal(ptab[f], pwant[0][f]), (devices, f)
