"""GPU test that the launch layer of the scan calls (kernels.h: ScanChunk, ScanDesc and each call's own struct) hands every
block kernel the arguments it handed them before: the same two blocks go through every kernel route of cryo_codec_filter_blocks,
_agg_blocks, _project_blocks and _topn_blocks, and through the three pattern routes of cryo_codec_group_blocks that
tests/test_gpu_group_routes.py does not reach.  Every route must return what the plain route of its call returns, byte for byte,
and the plain route what the call's reference returns (tests/filter_ref.py, agg_ref.py, project_ref.py, topn_ref.py, group_ref.py).

The blocks are that file's: group_cases.turn_block at its block size with its row type, of 1 and 65 matches -- 65 is the smallest
count that needs a second turn of the wave --, as LZ4 streams.  The routes and the kernels they reach (kernels.h, scan_route):
    plain   the descriptor alone                    k_filter_match<false>  k_agg_block<false>  k_project_block<false>  k_topn_block<false>
    truth   with a truth table                      k_filter_match<true>   k_agg_block<true>   k_project_block<true>   k_topn_block<true>
    float   with a float4 key every row passes      k_filterf_match        k_aggf_block        k_projectf_block        k_topnf_block
    like    with LIKE '%' on the text column        k_filterl_match        k_aggl_block        k_projectl_block        k_topnl_block
and of the grouped scan (group_route):
    like            LIKE '%'                                                  k_groupl_block
    buckets, like   CRYO_GROUP_BUCKETS with the bucket CRYO_BUCKET_NONE       k_groupbl_block
    text, like      CRYO_GROUP_TEXT, a text second group column               k_grouptl_block
A struct field swapped or dropped on the way to one of these kernels changes its output or its status."""
import numpy as np
import pytest

import agg_ref as ar
import filter_ref as fr
import group_cases as gc
import group_ref as gr
import project_ref as pr
import topn_ref as tr
from pg_cryogen_amd import METHOD_LZ4, codec as cc
from scan_calls import REC_SENTINEL, SENTINEL, Encoder, same_agg, same_fields, same_filter, same_group, same_project
from test_gpu_group_routes import ATTS, CONST, EVERY, FLOAT, G, NONE, T, X, Y, row

pytestmark = pytest.mark.gpu

SIZES = (1, 65)
LIKE = (5, cc.KEY_BYTES, cc.OP_LIKE, cc.like("%"))       # the text column holds CONST in every row
ROUTES = {"plain": ([EVERY], None), "truth": ([EVERY], cc.truth_dnf([1], 1)), "float": ([EVERY, FLOAT], None), "like": ([EVERY, LIKE], None)}
AGG_COLS = [X, Y, X, G]
ROW_COLS = [1, 3, 4]                                     # g int4, x int8, y int4: offsets 0, 8, 16; 24 bytes
BY = [(3, cc.KEY_INT8, cc.ORDER_DESC | cc.ORDER_NULLS_FIRST), (1, cc.KEY_INT4, 0)]   # x is NULL at every third match (row): there g decides
LIMIT = 10                                               # below 65: the second block's ranking is cut


@pytest.fixture(scope="module")
def blocks():
    return [gc.turn_block("straddle", m, atts=ATTS, row=row) for m in SIZES]


@pytest.fixture(scope="module")
def comps(oracle, blocks):
    enc = Encoder(oracle)
    return [enc(METHOD_LZ4, b) for b in blocks]


def every_route(call):
    """{route: call(filter descriptor)}, the plain route first"""
    return {name: call(cc.filter_desc(ATTS, keys, 0, truth)) for name, (keys, truth) in ROUTES.items()}


def test_filter_routes(codec, blocks, comps):
    def call(desc):
        table, rec, dst, total = codec.filter_blocks(METHOD_LZ4, comps, gc.TURN_B, desc, dst=np.full(len(comps) * gc.TURN_B, SENTINEL, np.uint8),
                                                     rec=np.full(len(comps) * 290, REC_SENTINEL, cc.FILTER_REC))
        return table, rec, dst, total
    got = every_route(call)
    want = fr.filter_call(blocks, ATTS, [EVERY])
    assert want[0]["n_match"].tolist() == list(SIZES) and want[3][1] == sum(SIZES)
    same_filter(got["plain"], want, "plain")
    for name, g in got.items():
        assert g[3] == got["plain"][3] and all(a.tobytes() == b.tobytes() for a, b in zip(g[:3], got["plain"][:3])), name


def test_agg_routes(codec, blocks, comps):
    got = every_route(lambda desc: codec.agg_blocks(METHOD_LZ4, comps, gc.TURN_B, desc, cc.agg_desc(AGG_COLS)))
    want = ar.agg_call(blocks, ATTS, [EVERY], AGG_COLS)
    assert want[0]["n_match"].tolist() == list(SIZES) and (want[1]["n"][1, :2] < 65).all()          # the NULLs of x and y
    same_agg(got["plain"], want, "plain")
    for name, g in got.items():
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, got["plain"])), name


def test_project_routes(codec, blocks, comps):
    rb = pr.row_layout(ATTS, ROW_COLS)[1]

    def call(desc):
        table, rec, rows, (tw, trec) = codec.project_blocks(METHOD_LZ4, comps, gc.TURN_B, desc, cc.project_desc(ROW_COLS), rb)
        return table, rec[:trec].copy(), rows[:tw].copy(), (tw, trec)
    got = every_route(call)
    want = pr.project_call(blocks, ATTS, [EVERY], ROW_COLS)
    assert rb == 24 and tuple(want[3]) == (sum(SIZES), sum(SIZES))
    same_project(got["plain"], want, "plain")
    for name, g in got.items():
        assert g[3] == got["plain"][3] and all(a.tobytes() == b.tobytes() for a, b in zip(g[:3], got["plain"][:3])), name


def test_topn_routes(codec, blocks, comps):
    rb = pr.row_layout(ATTS, ROW_COLS)[1]

    def call(desc):
        table, rec, rows, total = codec.topn_blocks(METHOD_LZ4, comps, gc.TURN_B, desc, cc.order_desc(BY, LIMIT), cc.project_desc(ROW_COLS), rb)
        return table, rec[:total].copy(), rows[:total].copy(), total
    got = every_route(call)
    want = tr.topn_call(blocks, ATTS, [EVERY], BY, LIMIT, ROW_COLS)
    assert want[3] == 1 + LIMIT and want[0]["n_match"].tolist() == list(SIZES)
    assert got["plain"][3] == want[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got["plain"][:3], want[:3])), "plain"
    for name, g in got.items():
        assert g[3] == got["plain"][3] and all(a.tobytes() == b.tobytes() for a, b in zip(g[:3], got["plain"][:3])), name


def test_group_pattern_routes(codec, blocks, comps):
    def call(keys, by, buckets=None, text=False):
        return codec.group_blocks(METHOD_LZ4, comps, gc.TURN_B, cc.filter_desc(ATTS, keys), cc.group_desc(by, buckets, text), cc.agg_desc(AGG_COLS))
    want = gr.group_call(blocks, ATTS, [EVERY], [G], AGG_COLS)
    assert want[0]["n_match"].tolist() == list(SIZES) and want[0]["n_groups"].tolist() == [1, 64]      # one run over the places 63 and 64, across the turns
    plain = call([EVERY], [G])
    same_group(plain, want, "plain")
    for name, got in (("like", call([EVERY, LIKE], [G])), ("buckets, like", call([EVERY, LIKE], [G], buckets=NONE))):
        same_group(got, want, name)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], plain[:3])), name
    # text, like: the comparison test_gpu_group_routes.py makes for its text routes
    name = "text, like"
    rows, recs, cells, total, key = call([EVERY, LIKE], [G, T], text=True)
    assert total == want[3], name
    same_fields(rows, want[0], (name, "rows"))
    assert rows.tobytes() == plain[0].tobytes(), name
    assert np.array_equal(recs["key"][:, 0], plain[1]["key"][:, 0]) and np.array_equal(recs["n_rows"], plain[1]["n_rows"]), name
    assert (recs["key"][:, 1] == len(CONST)).all() and not recs["nulls"].any(), name
    assert cells.shape == (total, len(AGG_COLS)) and cells.tobytes() == plain[2].tobytes(), name
    same_fields(cells, want[2], (name, "cells"))
    assert key.shape == (total, 1), name
    assert (key["len"] == len(CONST)).all() and not key["rsv"].any(), name
    assert (key["bytes"][:, 0, :len(CONST)] == np.frombuffer(CONST, np.uint8)).all() and not key["bytes"][:, 0, len(CONST):].any(), name
