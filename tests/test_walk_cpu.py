"""The Python references of the four scans against expectations that involve no walk (tests/walk_gen.py), on wide random tuples:
multi-byte null bitmaps, t_hoff up to 240, 1600 columns, every fixed width and alignment the argument rule admits, varlenas aligned
to 8, busy header words -- and every cut of a tuple.  filter_ref, agg_ref, group_ref, project_ref and bytes_key_ref each restate
the walk of include/cryo_codec.h; here each must equal what the rows the tuples were made from say, and each other.  No GPU."""
import hashlib
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
import float_ref as flr
import project_ref as pr
import topn_ref as tn
import tuple_craft as tc
import walk_gen as wg
import walk_routes as wr
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
    verdict of expect_match and the cut rule, and the values of the row; topn_ref.topn_tuple and float_ref.tuple_verdict under an
    order spec, a set key and a float-typed key as well"""
    atts, row, knobs, t, keys, cols, pcols, (by, nkeys) = wg.draw_tuple_case(rng)
    nmatch = wg.expect_match(row, nkeys)
    last_n, last_t = wg._last(nkeys, cols), wg._last(nkeys, list(pcols) + list(by))
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
        verdict = lambda last: fr.TUPLE if c < wg.need(atts, row, hoff, last) else fr.OK if nmatch else fr.NOMATCH  # noqa: E731
        want = verdict(last_n)
        assert flr.tuple_verdict(cut, atts, nkeys, cols) == (want, [value(col) for col, _ in cols] if want == fr.OK else None), (c, "float_ref")
        got = tn.topn_tuple(cut, atts, nkeys, by, pcols)
        want = verdict(last_t)
        if want != fr.OK:
            assert got == (want, None, None, None, None), (c, "topn_tuple")
        else:
            order = [value(col) for col, _, _ in by]
            assert got[0] == fr.OK and got[2:] == (sum(1 << j for j, v in enumerate(order) if v is None),) + wg._row_bytes(atts, row, pcols), (c, "topn_tuple")
            for j, (col, typ, _) in enumerate(by):
                if order[j] is None:
                    assert got[1][j] == 0
                elif typ in wg.INT_TYPE.values():
                    assert got[1][j] == order[j]
                else:                                                                # the image keeps the float order
                    x = wg.float_rank(wg.as_float(order[j], typ))
                    for other in (0, -1, order[j]) + wg.extremes(atts[col - 1][0]):
                        y = wg.float_rank(wg.as_float(other, typ))
                        assert (x > y) - (x < y) == (got[1][j] > tn.image(other, typ)) - (got[1][j] < tn.image(other, typ)), (c, "image")


# ---- the newer kernels and routes: the ordered scan, text and bucket grouping; float, pattern and set keys, a truth table ----
ALL_NAMES = wg.NAMES + wg.NEW_NAMES
DIGESTS = {
    "bitmap-edges": "3b06135ea20e6445298994554f269196",
    "odd-widths": "eb9b112f4111a41079e9fdda8e722981",
    "varlena-8": "e20246f43b853941ae7279803c1067ca",
    "max-columns": "7645597ee9bf0846fd574da74c622f74",
    "random-1": "7b5a3c6a837404af063f004f1275a666",
    "random-7": "0f92c6423dd13a17300716f3ebbf77d1",
    "random-8": "271bb00ea241546aa3da04e971640560",
    "random-9": "19a20b3dcccd187253b0571046a73fc4",
    "random-17": "5b8f88688e9f2507ee9d1119bbd596d9",
    "random-64": "e619d3bea345b89f3c5c70dc27ef48a9",
    "random-65": "21d5e97654fe4818e9d3f5321fac75b1",
    "random-200": "710215379b1fe9630b2940807b7cb700",
}


@pytest.mark.parametrize("name", wg.NAMES)
def test_the_older_cases_keep_their_bytes(name):
    """the plans of the newer calls draw from no generator a case consumes: every block is what it was before they existed"""
    h = hashlib.sha256()
    for b in wg.case(name).blocks:
        h.update(b.data.tobytes())
    assert h.hexdigest()[:32] == DIGESTS[name]


def run_newer(case, blks, plan, kind, route, short=False):
    """the references of the calls of one kind under a route against the construction; returns how many calls there were"""
    blocks, atts = [b.data for b in blks], case.call_atts
    made = wr.calls(case, blks, plan, kind, route, short) if wr.runs(plan, kind, route) else []
    for call in made:
        wr.check(case, blks, call, wr.reference(blocks, atts, call, route), route)
    return len(made)


@pytest.mark.parametrize("kind", wr.NEW_KINDS)
@pytest.mark.parametrize("name", ALL_NAMES)
def test_newer_references_equal_the_construction(name, kind):
    """topn_ref, group_text_ref and bucket_ref under the plain key sets: every order spec, column list and kind of limit, both
    text groupings, every bucket"""
    case = wg.case(name)
    assert run_newer(case, case.blocks, case.plan, kind, "plain") > 0 or (kind == "group_text" and not case.plan.text_col)


@pytest.mark.parametrize("route", wr.ROUTES)
@pytest.mark.parametrize("name", ALL_NAMES)
def test_route_references_equal_the_construction(name, route):
    """float_ref, like_ref and set_key_ref with the truth table, in all seven calls"""
    case = wg.case(name)
    n = sum(run_newer(case, case.blocks, case.plan, kind, route) for kind in wr.KINDS)
    assert n > 0 or not wr.runs(case.plan, "filter", route)


@pytest.mark.parametrize("name", wg.SWEEP_NAMES)
def test_newer_references_on_every_cut(name):
    """one tuple cut to each of its lengths under the ordered scan, the text grouping (where the case has a text column) and
    the bucket grouping; bitmap-edges also under the pattern and the float route of the ordered scan"""
    case = wg.case(name)
    plan, blks = case.sweep_plan(), case.sweeps()
    assert run_newer(case, blks, plan, "topn", "plain", True) > 0
    assert run_newer(case, blks, plan, "group_text", "plain", True) > 0 or name == "max-columns"
    assert run_newer(case, blks, plan, "group_bucket", "plain", True) > 0
    if name == "bitmap-edges":
        assert run_newer(case, blks, plan, "topn", "like") > 0 and run_newer(case, blks, plan, "topn", "float") > 0


# ---- the newer plans say something ----
def _block_rows(case, blk):
    return [(pos, case.rows[i]) for pos, (i, _) in enumerate(blk.items, 1)]


def _topn_facts(case, route):
    """per ordered call of a route and block: (call, matches, kept rows as expect_topn gives them)"""
    out = []
    for call in wr.calls(case, case.blocks, case.plan, "topn", route) if wr.runs(case.plan, "topn", route) else []:
        _, keys, truth, (by, limit, cols) = call
        for blk in case.blocks:
            n, kept = wg.expect_topn(_block_rows(case, blk), keys, by, limit, cols, case.call_atts, truth)
            out.append((call, n, kept))
    return out


def test_coverage_of_the_ordered_calls():
    words, relations, null_first, null_last = set(), set(), False, False
    for name in ALL_NAMES:
        case = wg.case(name)
        facts = _topn_facts(case, "plain")
        tie = False
        for (_, keys, truth, (by, limit, cols)), n, kept in facts:
            words.add(pr.row_layout(case.call_atts, cols)[1] // 8)
            relations.add((limit > n) - (limit < n))
            orders = [tuple(w[4]) for w in kept]
            tie = tie or len(set(orders)) < len(orders)                              # two kept rows the position alone orders
            for w in kept:
                for (_, _, flags), v in zip(by, w[4]):
                    null_first = null_first or (v is None and bool(flags & wg.NULLS_FIRST))
                    null_last = null_last or (v is None and not flags & wg.NULLS_FIRST)
        assert {f for spec in case.plan.topn_by for _, _, f in spec} == set(wg.FLAG_SETS), name
        assert {len(spec) for spec in case.plan.topn_by} == {1, 2}, name
        assert any(att in cols for _, _, _, (by, _, cols) in [f[0] for f in facts] for att, _, _ in by), name
        if any(wg.is_int(a) for a in case.call_atts[8:]):
            assert any(att > 8 for spec in case.plan.topn_by for att, _, _ in spec), name
        if sum(1 for a in case.call_atts if wg.is_int(a)) >= 2:
            assert tie, name
    assert words == set(range(1, 9)), words
    assert relations == {-1, 0, 1} and null_first and null_last
    seen = set()
    for name in ALL_NAMES:                                                           # a float order column over NaN, -0.0 and +0.0
        case = wg.case(name)
        for (_, _, _, (by, _, _)), _, kept in _topn_facts(case, "float"):
            att, typ, _ = by[0]
            vals = [wg.as_float(w[4][0], typ) for w in kept if w[4][0] is not None]
            if any(x != x for x in vals) and any(x == 0 and str(x)[0] == "-" for x in vals) and any(x == 0 and str(x)[0] != "-" for x in vals):
                seen.add(name)
    assert "bitmap-edges-dense" in seen, seen


@pytest.mark.parametrize("name", ALL_NAMES)
def test_coverage_of_the_groupings(name):
    case = wg.case(name)
    plan, atts = case.plan, case.call_atts
    if plan.text_col:
        empty = short = null = toast = long_ = 0
        for keys, truth in wr.keysets_of(plan, "plain"):
            for t, r in ((t, r) for t in sorted({att for by in plan.text_by for att, typ in by if typ == wg.BYTES}) for r in case.rows):
                if wg.expect_match(r, keys, truth) is not True:
                    continue
                v = r[t - 1] if t <= len(r) else None
                key = None if v is None else wg.text_key(v)
                null += key is None
                toast += isinstance(v, Toast)
                long_ += key == wg.AWAY and isinstance(v, (bytes, Long))
                empty += key == b""
                short += isinstance(key, bytes) and 9 <= len(key) <= 32
        assert empty and short and null and toast and long_, (name, empty, short, null, toast, long_)
    if any(a == (8, 8) for a in atts):
        below_min = below_all = 0
        decided = set()
        for by, buckets in plan.buckets:
            for keys, truth in wr.keysets_of(plan, "plain"):
                for r in case.rows:
                    if wg.expect_match(r, keys, truth) is not True:
                        continue
                    for (att, _), bucket in zip(by, buckets):
                        v = r[att - 1] if att <= len(r) else None
                        if v is None or bucket == wg.RAW:
                            continue
                        key = wg.bucket_key(bucket, atts[att - 1][0], v)
                        if key != wg.AWAY:
                            decided.add((att, bucket[0], key))
                        elif bucket[0] == wg.WIDTH:
                            below_min += 1
                            assert bucket[2] + bucket[3] * ((v - bucket[2]) // bucket[3]) < wg.INT64_MIN
                        else:
                            below_all += 1
                            assert all(v < m for m in bucket[3])
        assert below_min and below_all and len(decided) >= 2, (name, below_min, below_all, len(decided))
    kinds = {(b[0], b[1]) for _, buckets in plan.buckets for b in buckets}
    assert (wg.WIDTH, wg.INFINITE) in kinds and {len(b[3]) > 8 for _, bs in plan.buckets for b in bs if b[0] == wg.BOUNDS} == {False, True}


@pytest.mark.parametrize("name", ALL_NAMES)
def test_coverage_of_the_key_sets(name):
    case = wg.case(name)
    plan = case.plan
    for keys in plan.float_keysets + plan.like_keysets + plan.set_keysets + [plan.table_keys]:
        truth = plan.table if keys is plan.table_keys else None
        states = {wg.expect_match(r, keys, truth) for r in case.rows}
        assert {True, False} <= states, (name, keys, states)
        if keys in plan.like_keysets:
            assert None in states, (name, keys)
    assert len(plan.set_keysets[0][0][3]) <= 8 < len(plan.set_keysets[2][0][3])
    if name == "bitmap-edges-dense":
        assert max(len(b.items) for b in case.blocks) > 64
        for keys, truth in wr.all_keysets(plan):
            assert any(wg.expect_match(case.rows[i], keys, truth) is True for b in case.blocks for i, _ in b.items[64:]), keys
