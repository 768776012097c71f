"""CPU test of tests/group_text_ref.py, the reference of the text group columns (include/cryo_codec.h, "Text group columns"):
what it says about the hand-made blocks of tests/group_text_cases.py is what was written out by hand there, its results keep the
layout rules of the contract, and its descriptor rules are the header's.  The GPU tests hold the kernels against it."""
import numpy as np
import pytest

import group_ref as gr
import group_text_cases as gc
import group_text_ref as gt
from filter_ref import EQ, INT2, INT4, INT8
from float_ref import FLOAT8

CASES = gc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made_blocks(case):
    name, block, keys, by, cols, groups, n_bad = case
    got = gt.group_call([block], gc.ATTS, keys, by, cols)
    rows, recs, cells, total, kc = got
    assert gt.groups_of(got, by, 0) == groups
    assert int(rows[0]["n_bad"]) == n_bad and int(rows[0]["n_match"]) == sum(n for _, n in groups) == int(recs["n_rows"].sum())
    assert total == len(groups) and cells.shape == (total, len(cols)) and kc.shape == (total, sum(t == gt.BYTES for _, t in by))
    assert kc.dtype.itemsize == 40


def test_a_null_cell_is_all_zero_and_the_key_is_the_length():
    _, block, keys, by, cols, _, _ = CASES[0]
    rows, recs, cells, total, kc = gt.group_call([block], gc.ATTS, keys, by, cols)
    assert recs["key"].tolist() == [[0, 0], [0, 0]] and recs["nulls"].tolist() == [0, 1]       # '' has length 0 and is no NULL
    assert not kc.view(np.uint8).any()
    _, block, keys, by, cols, _, _ = CASES[1]
    rows, recs, cells, total, kc = gt.group_call([block], gc.ATTS, keys, by, cols)
    assert recs["key"][:, 0].tolist() == [1, 2, 3, 3] and kc["len"][:, 0].tolist() == [1, 2, 3, 3]
    assert bytes(kc["bytes"][2, 0]) == b"ab\0" + bytes(29) and bytes(kc["bytes"][3, 0]) == b"abc" + bytes(29)


def test_integer_columns_alone_are_the_plain_call():
    blocks = [c[1] for c in CASES]
    for by, cols in (([gc.D], [gc.X]), ([gc.D, gc.X], []), ([gc.X], [gc.D, gc.X])):
        want = gr.group_call(blocks, gc.ATTS, [(3, INT8, EQ, 10)], by, cols)
        got = gt.group_call(blocks, gc.ATTS, [(3, INT8, EQ, 10)], by, cols)
        assert got[3] == want[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3])) and got[4].shape == (want[3], 0)


def test_blocks_of_a_call_and_a_rejected_stream():
    blocks = [CASES[1][1], None, CASES[6][1]]
    rows, recs, cells, total, kc = gt.group_call(blocks, gc.ATTS, [], [gc.T_, gc.D], [gc.X])
    assert rows["status"].tolist() == [0, 1, 0] and rows["n_groups"].tolist() == [4, 0, 4] and rows["first_group"].tolist() == [0, 4, 4]
    assert total == 8 and gt.groups_of((rows, recs, cells, total, kc), [gc.T_, gc.D], 2) == CASES[6][5]


A = gc.ATTS
RULES = [
    ("a text column", [gc.T_], [gc.X], gt.TEXT, True),
    ("text and int", [gc.T_, gc.D], [], gt.TEXT, True),
    ("int and text", [gc.D, gc.T_], None, gt.TEXT, True),
    ("text and text", [gc.T_, gc.U], [gc.X, gc.D], gt.TEXT, True),
    ("the same text column twice", [gc.T_, gc.T_], [gc.X], gt.TEXT, True),
    ("integer columns under the flag", [gc.D, gc.X], [gc.X], gt.TEXT, True),
    ("a float aggregate column beside a text column", [gc.T_], [(6, FLOAT8)], gt.TEXT, True),
    ("a text column without the flag", [gc.T_], [gc.X], 0, False),
    ("a text column behind an integer column without the flag", [gc.D, gc.T_], [gc.X], 0, False),
    ("BYTES on an int4 column", [(5, gt.BYTES)], [gc.X], gt.TEXT, False),
    ("BYTES on an int8 column", [(3, gt.BYTES)], [gc.X], gt.TEXT, False),
    ("an integer type on a text column", [(2, INT4)], [gc.X], gt.TEXT, False),
    ("BYTES as an aggregate column", [gc.D], [gc.T_], gt.TEXT, False),
    ("BYTES as an aggregate column beside a text group column", [gc.T_], [gc.X, gc.U], gt.TEXT, False),
    ("a float group column under the flag", [(6, FLOAT8)], [], gt.TEXT, False),
    ("column 0", [(0, gt.BYTES)], [], gt.TEXT, False),
    ("column 7 of 6", [(7, gt.BYTES)], [], gt.TEXT, False),
    ("type 17", [(2, 17)], [], gt.TEXT, False),
    ("three group columns", [gc.T_, gc.U, gc.D], [], gt.TEXT, False),
    ("no group column", [], [gc.X], gt.TEXT, False),
    ("rsv 5: text and buckets", [gc.T_], [gc.X], gt.TEXT | gt.BUCKETS, False),
    ("rsv 2", [gc.D], [gc.X], 2, False),
    ("rsv 3", [gc.D], [gc.X], 3, False),
    ("rsv 6", [gc.T_], [gc.X], 6, False),
    ("rsv 8", [gc.T_], [gc.X], 8, False),
    ("rsv 0x80000004", [gc.T_], [gc.X], 0x80000004, False),
]


@pytest.mark.parametrize("rule", RULES, ids=[r[0] for r in RULES])
def test_descriptor_rules(rule):
    name, by, cols, rsv, ok = rule
    assert gt.desc_ok(A, [], by, cols, rsv) == ok
    assert not gt.desc_ok(A, [], by, cols, rsv, by_rsv=[1])                # a group column's reserved field


def test_a_narrow_integer_column_beside_a_text_column():
    atts = [(2, 2), (-1, 4)]
    assert gt.desc_ok(atts, [], [(1, INT2), (2, gt.BYTES)], [(1, INT2)])
    assert not gt.desc_ok(atts, [], [(1, INT4), (2, gt.BYTES)], [])
