"""GPU test of the one run reduction under every block kernel of the grouped scan (group_lds.h: group_reduce).

The same blocks and the same integer aggregate columns go through every kernel route a caller of cryo_codec_group_blocks can
reach; every route must return the records and aggregate cells of the plain call, byte for byte, and the plain call those of
tests/group_ref.py.  The blocks are group_cases.turn_block's at its block size, with 1, 63, 64, 65, 128, 129 and 290 matches --
the turns of a wave -- in one group (one lane walks the whole run), in as many groups as matches (the prefix of heads carried
across the turns) and with one run over the places 63 .. 65 (a head in one turn whose run ends in the next); with no aggregate
column and with four, whose values are NULL in places.

The routes and the kernel each reaches (group.hip, launch_group):
    plain                 the descriptor alone                                              k_group_block<false>
    truth                 with a truth table                                                k_group_block<true>
    float                 with a float4 key every row passes                                k_groupf_block
    buckets               CRYO_GROUP_BUCKETS, the bucket CRYO_BUCKET_NONE                   k_groupb_block<false>
    buckets, float        both                                                              k_groupb_block<true>
    text                  CRYO_GROUP_TEXT, a text second group column with one value        k_groupt_block<false>
    text, float           both                                                              k_groupt_block<true>"""
import numpy as np
import pytest

import group_cases as gc
import group_ref as gr
from pg_cryogen_amd import METHOD_LZ4, codec as cc
from scan_calls import Encoder, same_fields, same_group

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (4, 4), (8, 8), (4, 4), (-1, 4)]        # (g int4, f float4, x int8, y int4, t text): at most 48 bytes a tuple
G, F, X, Y, T = (1, cc.KEY_INT4), (2, cc.KEY_FLOAT4), (3, cc.KEY_INT8), (4, cc.KEY_INT4), (5, cc.KEY_BYTES)
ONE_F = 0x3F800000                                      # 1.0f
CONST = b"k"
SIZES = (1, 63, 64, 65, 128, 129, 290)
PATTERNS = ("one", "distinct", "straddle")
COLS = {0: [], 4: [X, Y, X, G]}
EVERY = (1, cc.KEY_INT4, cc.OP_GE, -(1 << 31))          # a key every row passes
FLOAT = (2, cc.KEY_FLOAT4, cc.OP_GE, 0.0)               # another, on the float column
NONE = [(cc.BUCKET_NONE, 0, 0, 0)]


def row(p, g):
    """x: NULL at every third match, else a value that needs both halves of the sum; y: NULL at every fifth"""
    return [g, ONE_F, None if p % 3 == 1 else (p * 2654435761 % (1 << 41)) - (1 << 40), None if p % 5 == 2 else 7 * p - 1000, CONST]


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


@pytest.fixture(scope="module")
def blocks():
    return {pattern: [gc.turn_block(pattern, m, atts=ATTS, row=row) for m in SIZES] for pattern in PATTERNS}


def call(codec, comps, keys, by, cols, truth=None, buckets=None, text=False):
    return codec.group_blocks(METHOD_LZ4, comps, gc.TURN_B, cc.filter_desc(ATTS, keys, 0, truth), cc.group_desc(by, buckets, text),
                              cc.agg_desc(cols) if cols else None)


@pytest.mark.parametrize("ncols", sorted(COLS))
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_route_reduces_alike(codec, enc, blocks, pattern, ncols):
    cols = COLS[ncols]
    comps = [enc(METHOD_LZ4, b) for b in blocks[pattern]]
    want = gr.group_call(blocks[pattern], ATTS, [EVERY], [G], cols)
    groups = {"one": [1] * len(SIZES), "distinct": list(SIZES), "straddle": [m - max(0, min(m, 66) - 64) for m in SIZES]}[pattern]
    assert want[0]["n_match"].tolist() == list(SIZES) and want[0]["n_groups"].tolist() == groups and want[3] == sum(groups)
    if ncols:
        assert (want[2]["n"][:, 0] < want[1]["n_rows"]).any() and (want[2]["n"][:, 1] < want[1]["n_rows"]).any()   # the NULLs
    plain = call(codec, comps, [EVERY], [G], cols)
    same_group(plain, want, (pattern, ncols, "plain"))
    for name, got in (("truth", call(codec, comps, [EVERY], [G], cols, truth=cc.truth_dnf([1], 1))),
                      ("float", call(codec, comps, [EVERY, FLOAT], [G], cols)),
                      ("buckets", call(codec, comps, [EVERY], [G], cols, buckets=NONE)),
                      ("buckets, float", call(codec, comps, [EVERY, FLOAT], [G], cols, buckets=NONE))):
        same_group(got, want, (pattern, ncols, name))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], plain[:3])), (pattern, ncols, name)
    for name, got in (("text", call(codec, comps, [EVERY], [G, T], cols, text=True)),
                      ("text, float", call(codec, comps, [EVERY, FLOAT], [G, T], cols, text=True))):
        rows, recs, cells, total, key = got
        assert total == want[3], (pattern, ncols, name)
        same_fields(rows, want[0], (pattern, ncols, name, "rows"))
        assert rows.tobytes() == plain[0].tobytes(), (pattern, ncols, name)
        assert np.array_equal(recs["key"][:, 0], plain[1]["key"][:, 0]) and np.array_equal(recs["n_rows"], plain[1]["n_rows"]), (pattern, ncols, name)
        assert (recs["key"][:, 1] == len(CONST)).all() and not recs["nulls"].any(), (pattern, ncols, name)
        assert cells.shape == (total, ncols) and cells.tobytes() == plain[2].tobytes(), (pattern, ncols, name)
        same_fields(cells, want[2], (pattern, ncols, name, "cells"))
        assert key.shape == (total, 1), (pattern, ncols, name)             # without an aggregate column a group's only cell
        assert (key["len"] == len(CONST)).all() and not key["rsv"].any(), (pattern, ncols, name)
        assert (key["bytes"][:, 0, :len(CONST)] == np.frombuffer(CONST, np.uint8)).all() and not key["bytes"][:, 0, len(CONST):].any(), \
            (pattern, ncols, name)
