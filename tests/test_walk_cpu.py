"""The Python references of the four scans against expectations that involve no walk (tests/walk_gen.py), on wide random tuples:
multi-byte null bitmaps, t_hoff up to 240, 1600 columns, every fixed width and alignment the argument rule admits, varlenas aligned
to 8, busy header words -- and every cut of a tuple.  filter_ref, agg_ref, group_ref, project_ref and bytes_key_ref each restate
the walk of include/cryo_codec.h; here each must equal what the rows the tuples were made from say, and each other.  No GPU."""
import inspect

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import agg_cases
import agg_ref as ar
import bytes_key_cases
import bytes_key_ref as br
import filter_cases
import filter_ref as fr
import group_cases
import group_ref as gr
import project_cases
import project_ref as pr
import tuple_craft as tc
import walk_gen as wg
from tuple_craft import HASNULL, HASVARWIDTH, XMAX_INVALID, Long, Toast, maxalign


# ---- tuple_craft: the knobs' defaults change no tuple ----
def minimal_form_tuple(atts, values, xmin=1000):
    """tuple_craft.form_tuple as it stood before it had header knobs, kept word for word"""
    import struct
    natts = len(values)
    hasnull = any(v is None for v in values)
    bitmap = bytearray((natts + 7) // 8 if hasnull else 0)
    hoff = maxalign(23 + len(bitmap))
    data = bytearray()
    infomask = XMAX_INVALID | (HASNULL if hasnull else 0)
    for i, v in enumerate(values):
        attlen, attalign = atts[i]
        if v is None:
            continue
        if hasnull:
            bitmap[i // 8] |= 1 << (i % 8)
        if attlen > 0:
            data += bytes(-len(data) % attalign)
            data += int(v).to_bytes(attlen, "little", signed=True)
            continue
        infomask |= HASVARWIDTH
        if isinstance(v, Toast):
            data += bytes([0x01, v.tag]) + bytes(range(16))
        elif isinstance(v, Long) or len(v) > 126:
            payload = v.payload if isinstance(v, Long) else bytes(v)
            data += bytes(-len(data) % attalign)
            data += struct.pack("<I", (len(payload) + 4) << 2) + payload
        else:
            data += bytes([((len(v) + 1) << 1) | 1]) + bytes(v)
    head = bytearray(23)
    struct.pack_into("<I", head, 0, xmin)
    struct.pack_into("<HH", head, 18, natts, infomask)
    head[22] = hoff
    return bytes(head) + bytes(bitmap) + bytes(hoff - 23 - len(bitmap)) + bytes(data)


def test_form_tuple_defaults_are_the_minimal_header(monkeypatch):
    """every tuple the crafted blocks of filter_cases, agg_cases, group_cases, project_cases and bytes_key_cases ask for -- each
    call of form_tuple while every block-making function of theirs runs -- is byte for byte what the function gave before"""
    real, calls = tc.form_tuple, []

    def spy(atts, values, *a, **kw):
        calls.append((list(atts), list(values), a, kw))
        return real(atts, values, *a, **kw)

    monkeypatch.setattr(tc, "form_tuple", spy)
    per_module = {}
    for mod in (filter_cases, agg_cases, group_cases, project_cases, bytes_key_cases):
        before = len(calls)
        for name, fn in inspect.getmembers(mod, inspect.isfunction):
            if fn.__module__ == mod.__name__ and not inspect.signature(fn).parameters and name not in ("descriptors",):
                fn()
        per_module[mod.__name__] = len(calls) - before
    for m in group_cases.TURN_SIZES:
        for pattern in group_cases.PATTERNS:
            group_cases.turn_block(pattern, m)
    for n in project_cases.TURN_SIZES:
        project_cases.turn_block(n)
        project_cases.turn_block_alternating(n)
    assert all(v > 0 for v in per_module.values()), per_module
    for atts, values, a, kw in calls:
        assert not kw or set(kw) <= {"xmin"}
        assert real(atts, values, *a, **kw) == minimal_form_tuple(atts, values, *a, **kw)


def test_form_tuple_knobs():
    atts, values = [(4, 4), (-1, 4), (8, 8)], [7, b"ab", -1]
    plain = tc.form_tuple(atts, values)
    t = tc.form_tuple(atts, values, infomask2_flags=0xE000, infomask_flags=0xFF0C, extra_hoff=16, force_bitmap=True)
    assert int.from_bytes(t[18:20], "little") == 3 | 0xE000
    assert int.from_bytes(t[20:22], "little") == 0xFF0C | HASNULL | HASVARWIDTH | XMAX_INVALID
    assert t[22] == 24 + 16 and t[23] == 0b111 and not any(t[24:40]) and t[40:] == plain[24:]
    assert tc.form_tuple(atts, [7, None, -1], extra_hoff=8)[22] == 32


# ---- the references against the construction ----
def assert_same_arrays(a, b, what):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what
        else:
            assert x == y, what


def run_references(case, blks, plan, keysets, with_filter_ref=True):
    """every reference on the blocks, for each key set: against the construction, and against each other where two cover a call"""
    blocks, atts = [b.data for b in blks], case.call_atts
    n = 0
    for keys in keysets:
        ints_only = not any(br.is_bytes_key(k) for k in keys)
        what = (case.name, keys)
        f = br.filter_call(blocks, atts, keys)
        wg.check_filter(case, blks, keys, f, what)
        a = br.agg_call(blocks, atts, keys, plan.agg_cols)
        wg.check_agg(case, blks, keys, plan.agg_cols, a, what)
        g = br.group_call(blocks, atts, keys, plan.by, plan.group_cols)
        wg.check_group(case, blks, keys, plan.by, plan.group_cols, g, what)
        wg.check_project(case, blks, keys, plan.project_cols, pr.project_call(blocks, atts, keys, plan.project_cols), what)
        if ints_only:
            f2 = fr.filter_call(blocks, atts, keys)
            wg.check_filter(case, blks, keys, f2, what)
            assert_same_arrays(f, f2, what)
            a2 = ar.agg_call(blocks, atts, keys, plan.agg_cols)
            wg.check_agg(case, blks, keys, plan.agg_cols, a2, what)
            assert_same_arrays(a, a2, what)
            g2 = gr.group_call(blocks, atts, keys, plan.by, plan.group_cols)
            wg.check_group(case, blks, keys, plan.by, plan.group_cols, g2, what)
            assert_same_arrays(g, g2, what)
        n += sum(len(b.items) for b in blks)
    return n


@pytest.mark.parametrize("name", wg.NAMES)
def test_references_equal_the_construction(name):
    case = wg.case(name)
    run_references(case, case.blocks, case.plan, case.plan.keysets + case.plan.bytes_keysets)


@pytest.mark.parametrize("name", wg.NAMES)
def test_references_on_every_cut(name):
    """one tuple cut to each of its lengths: TUPLE below `need`, the uncut tuple's verdict and capture from there on"""
    case = wg.case(name)
    plan = case.sweep_plan()
    assert run_references(case, case.sweeps(), plan, [plan.keysets[0], plan.keysets[3]] + plan.bytes_keysets[:1]) > 0


# ---- the generator has not degenerated ----
@pytest.mark.parametrize("name", wg.NAMES)
def test_coverage_of_a_descriptor(name):
    case = wg.case(name)
    assert 1 <= len(case.blocks) <= wg.MAX_BLOCKS and case.B in (8192, 16384)
    assert sum(len(b.items) for b in case.blocks) == len(case.rows)                  # no row is left out of the blocks
    hits = [wg.expect_match(r, case.plan.keysets[1]) for r in case.rows]
    assert True in hits and False in hits
    cols = case.plan.referenced()
    assert any(len(r) >= c and r[c - 1] is None for r in case.rows for c in cols), "no NULL by bitmap on a referenced column"
    assert any(len(r) < c for r in case.rows for c in cols), "no NULL by a short tnatts on a referenced column"
    for keys in case.plan.bytes_keysets:
        states = {wg.expect_match(r, keys) for r in case.rows}
        assert states == {True, False, None}, (keys, states)                        # in-line, and compressed or external


def test_coverage_of_the_whole_set():
    hoffs, flags, pads, widths = set(), set(), set(), set()
    for name in wg.NAMES:
        case = wg.case(name)
        for t, row, knobs in zip(case.tuples, case.rows, case.knobs):
            hoffs.add(t[22])
            flags.add(int.from_bytes(t[18:20], "little") & 0xF800)
            assert int.from_bytes(t[18:20], "little") & 0x07FF == len(row)
            for j, v in enumerate(row):
                if case.atts[j] == (-1, 8) and wg.has_long_header(v):
                    pads.add(wg.pad_before(case.atts, row, j))
        widths |= set(case.atts)
        if name == "bitmap-edges":
            assert any(len(r) > len(case.call_atts) for r in case.rows)             # tnatts beyond the descriptor the call passes
    assert {24, 32, 224} <= hoffs and any(h >= 40 for h in hoffs - {224}), sorted(hoffs)
    assert flags == set(wg.FLAGS), flags
    assert set(range(1, 8)) <= pads, pads
    assert set(wg.ODD + wg.PLAIN) <= widths
    rows = wg.case("max-columns").rows
    assert {0, 1, 1592, 1599, 1600} <= {len(r) for r in rows}
    assert any(len(r) == 1600 and None not in r for r in rows) and any(len(r) == 1600 and r.count(None) == 1 for r in rows)


# ---- the tuple-level functions on many more tuples ----
@settings(max_examples=250, deadline=None)
@given(st.randoms(use_true_random=False))
def test_tuple_functions_property(rng):
    """filter_tuple, agg_tuple, project_tuple and tuple_verdict on a drawn tuple and on its cuts around every column's end: the
    verdict of expect_match and the cut rule, and the values of the row"""
    atts, row, knobs, t, keys, cols, pcols = wg.draw_tuple_case(rng)
    hoff = t[22]
    ends = [hoff + wg.data_end(atts, row, j) for j in range(len(row)) if row[j] is not None]
    cuts = set(range(1, min(len(t), hoff + 9) + 1)) | {e + d for e in ends for d in (-1, 0, 1)} | {len(t) - 1, len(t)}
    match = wg.expect_match(row, keys)
    value = lambda c: row[c - 1] if c <= len(row) else None                          # noqa: E731
    nulls = sum(1 << j for j, c in enumerate(pcols) if value(c) is None)
    last_f, last_a, last_p = wg._last(keys), wg._last(keys, cols), wg._last(keys, pcols)
    for c in sorted(x for x in cuts if 1 <= x <= len(t)):
        cut = t[:c]
        verdict = lambda last: fr.TUPLE if c < wg.need(atts, row, hoff, last) else fr.OK if match else fr.NOMATCH  # noqa: E731
        assert fr.filter_tuple(cut, atts, keys) == verdict(last_f), (c, "filter_tuple")
        want = verdict(last_a)
        vals = [value(col) for col, _ in cols] if want == fr.OK else None
        assert ar.agg_tuple(cut, atts, keys, cols) == (want, vals), (c, "agg_tuple")
        assert br.tuple_verdict(cut, atts, keys, cols) == (want, vals), (c, "tuple_verdict")
        got = pr.project_tuple(cut, atts, keys, pcols)
        want = verdict(last_p)
        if want != fr.OK:
            assert got == (want, None, None), (c, "project_tuple")
        else:
            assert got == (fr.OK, nulls, wg.expect_rows(atts, [row], keys, pcols)[0][1]), (c, "project_tuple")
