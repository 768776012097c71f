"""CPU tests of the float scan keys and float aggregate columns: the reference (tests/float_ref.py) against the expectations
written out by hand in tests/float_cases.py, the properties of the map and of the double-double sum that the contract states
(monotone, self-inverse; |sum + err - exact| <= 2^-90 * sum |v|, checked in exact rational arithmetic), codec.cell_float_combine
against the reference, the header's text and values, the Python descriptors, and the host walks through a
codec double (tests/float_double.py) against cryo_agg_cell_f_combine.  No GPU."""
import ctypes as C
import os
import random
import re
import struct
from fractions import Fraction

import numpy as np
import pytest

import fetch_walk
import float_cases as fc
import float_ref as fl
import tuple_craft as tc
from pg_cryogen_amd import codec as cc, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = Fraction(1, 2 ** 90)


def special_bits():
    vals = [0.0, -0.0, fc.INF, -fc.INF, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0]
    return [fl.bits_of(v) for v in vals] + [fl.NAN_BITS, fc.NAN_SIGN & (1 << 64) - 1, fc.NAN_PAYLOAD, (1 << 64) - 1]


# ---- the map ----
def test_map_is_monotone_and_self_inverse():
    rng = random.Random(1)
    sample = special_bits() + [rng.getrandbits(64) for _ in range(4000)]
    for b in sample:
        m = fl.fmap(b)
        assert -(1 << 63) <= m <= fl.INT64_MAX
        x = fl.double_of(b)
        if x != x:
            assert m == fl.INT64_MAX and fl.unmap(m) == fl.NAN_BITS
        elif x == 0:
            assert m == 0 and fl.unmap(m) == 0
        else:
            assert fl.unmap(m) == b and fl.fmap(fl.unmap(m)) == m          # its own inverse apart from the two canonical cases
    for a in sample[:300]:
        for b in sample[:300]:
            for op in (fl.LT, fl.LE, fl.EQ, fl.GE, fl.GT, fl.NE):
                assert fl.fr._compare(op, fl.fmap(a), fl.fmap(b)) == fl.compare(op, a, b), (hex(a), hex(b), op)


def test_widening_is_exact():
    assert fl.widen(fc.SUB4, fl.FLOAT4) == fl.bits_of(2.0 ** -149)
    assert fl.widen(0x007FFFFF, fl.FLOAT4) == fl.bits_of(2.0 ** -126 - 2.0 ** -149)          # the largest float4 subnormal
    assert fl.widen(fc.MAX4, fl.FLOAT4) == fl.bits_of(3.4028234663852886e38)
    assert fl.widen(fl.f4(-0.0), fl.FLOAT4) == 1 << 63
    assert fl.fmap(fl.widen(fc.NAN4_SIGN, fl.FLOAT4)) == fl.INT64_MAX == fl.fmap(fl.widen(fc.NAN4_PAYLOAD, fl.FLOAT4))
    assert fl.widen(fl.f4(fc.INF), fl.FLOAT4) == fl.INF_BITS


# ---- the reference against the hand-written expectations ----
def test_reference_on_the_crafted_key_cases():
    for name, B, atts, blk, keys, truth, matches, bad in fc.cases():
        assert fl.desc_ok(atts, keys, fl.tr.TRUTH if truth else 0, truth or 0), name
        table, recs, packed, total = fl.filter_call([blk], atts, keys, truth=truth)
        assert recs["pos"][recs["status"] == 0].tolist() == matches, name
        assert {int(r["pos"]): int(r["status"]) for r in recs if r["status"]} == bad, name
        assert (table["n_match"][0], table["n_bad"][0]) == (len(matches), len(bad)), name


def test_reference_on_the_crafted_sums():
    for name, values, expect in fc.SUM_CASES:
        blk = fc.sum_block(values)
        rows, cells = fl.agg_call([blk], fc.ATTS, fc.SUM_KEYS, fc.SUM_COLS)
        assert rows["n_match"][0] == len(values), name
        got = tuple(int(w) for w in np.frombuffer(cells[0, 0].tobytes(), "<u8"))
        assert got == fc.words(expect), (name, [hex(w) for w in got], [hex(w) for w in fc.words(expect)])
        assert cc.cell_float(cells[0, 0])[0] == expect[0]
        assert cc.cell_sum(cells[0, 1]) == sum(p for p, _ in values)                          # the integer column beside it: the ids
        # the grouped call over one group (k = 1 on every match): position order
        grows, recs, gcells, total = fl.group_call([blk], fc.ATTS, fc.SUM_KEYS, [(6, fl.INT8)], fc.SUM_COLS)
        assert total == 1 and recs["n_rows"][0] == len(values), name
        gexp = fc.words(expect[:3] + fc.GROUP_SUMS.get(name, expect[3:]))
        assert tuple(int(w) for w in np.frombuffer(gcells[0, 0].tobytes(), "<u8")) == gexp, name


def test_min_and_max_follow_the_order():
    """max is NaN if any value is NaN, min only if all are; both canonical"""
    vals = [(1, fc.NAN_PAYLOAD), (2, fl.f8(-0.0)), (3, fl.f8(-fc.INF)), (4, fl.f8(3.0))]
    n, lo, hi, s, e = fl.cell_words(vals, fl.FLOAT8)
    assert (n, lo, hi, s, e) == (4, fl.bits_of(-fc.INF), fl.NAN_BITS, fl.NAN_BITS, 0)
    assert fl.cell_words([(1, fl.f4(-0.0)), (9, fc.SUB4)], fl.FLOAT4)[1:3] == (0, fl.bits_of(2.0 ** -149))


# ---- the accuracy the header states ----
def finite_values(values, typ):
    out = []
    for pos, raw in values:
        b = fl.widen(raw, typ)
        if b & fl.MAG < fl.INF_BITS:
            out.append((pos, fl.double_of(b)))
    return out


def within_bound(pair, values):
    exact = sum(Fraction(v) for _, v in values)
    return abs(Fraction(pair[0]) + Fraction(pair[1]) - exact) <= BOUND * sum(abs(Fraction(v)) for _, v in values)


def test_sum_meets_the_bound_and_plain_summation_does_not():
    checked = 0
    for name, values, expect in fc.SUM_CASES:
        vals = finite_values([(p, fl.f8(v) if isinstance(v, float) else v) for p, v in values if v is not None], fl.FLOAT8)
        for reduce in (fl.reduce_agg, fl.reduce_group):
            pair = reduce(vals)
            if all(x == x and abs(x) != fc.INF for x in pair):                                 # no overflow inside the reduction
                assert within_bound(pair, vals), name
                assert pair[0] == pair[0] + pair[1], name                                      # sum = RN(sum + err)
                checked += 1
        if name.startswith("cancellation"):
            plain = 0.0
            for _, v in vals:
                plain += v
            assert not within_bound((plain, 0.0), vals), name                                  # so the bound tests something
    assert checked >= 16
    rng = random.Random(7)
    for trial in range(60):
        n = rng.choice((1, 2, 63, 64, 65, 290))
        vals = [(p, rng.choice((-1, 1)) * rng.random() * 2.0 ** rng.randint(-300, 300)) for p in range(1, n + 1)]
        if trial % 3 == 0:                                                                     # heavy cancellation
            vals += [(n + 1 + i, -v) for i, (_, v) in enumerate(vals[:n // 2])]
            vals = vals[:290]
        for reduce in (fl.reduce_agg, fl.reduce_group):
            assert within_bound(reduce(vals), vals), (trial, reduce.__name__)


def test_sum_is_commutative_on_pairs():
    rng = random.Random(3)
    for _ in range(2000):
        x = (rng.uniform(-1, 1) * 2.0 ** rng.randint(-60, 60), rng.uniform(-1, 1) * 2.0 ** rng.randint(-120, 0))
        y = (rng.uniform(-1, 1) * 2.0 ** rng.randint(-60, 60), rng.uniform(-1, 1) * 2.0 ** rng.randint(-120, 0))
        assert fl.pair_add(x, y) == fl.pair_add(y, x)


# ---- combining cells ----
def test_cell_float_combine_against_the_reference():
    cells = [fc.words(e) for _, _, e in fc.SUM_CASES]
    rng = random.Random(9)
    for _ in range(40):
        vals = [(p, fl.f8(rng.uniform(-1, 1) * 2.0 ** rng.randint(-40, 40))) for p in range(1, rng.randint(2, 80))]
        cells.append(fl.cell_words(vals, fl.FLOAT8))
    for a in cells:
        for b in cells:
            want = fl.combine_words(a, b)
            got = cc.cell_float_combine(cc.cell_float(fl.as_cell(a)), cc.cell_float(fl.as_cell(b)))
            assert fc.words(got) == want, (a, b, got)
    # the P / M / Q rule across blocks, by hand
    inf, ninf, nan, fin, ovf = (fc.words(e) for e in ((1, fc.INF, fc.INF, fc.INF, 0.0), (1, -fc.INF, -fc.INF, -fc.INF, 0.0),
                                                     (1, fl.NAN_BITS, fl.NAN_BITS, fl.NAN_BITS, 0.0), (2, 1.0, 2.0, 3.0, 0.0),
                                                     (2, 1.5e308, 1.5e308, fl.NAN_BITS, fl.NAN_BITS)))
    assert fl.combine_words(inf, ninf)[3:] == (fl.NAN_BITS, 0)
    assert fl.combine_words(fin, inf) == (3, fl.bits_of(1.0), fl.INF_BITS, fl.INF_BITS, 0)
    assert fl.combine_words(ninf, fin)[3:] == (fl.INF_BITS | 1 << 63, 0)
    assert fl.combine_words(fin, nan)[2:] == (fl.NAN_BITS, fl.NAN_BITS, 0)
    assert fl.combine_words(fin, ovf)[3:] == (fl.NAN_BITS, fl.NAN_BITS)
    assert fl.combine_words(ovf, inf)[3:] == (fl.INF_BITS, 0)                                   # the flags come first, as inside a block
    assert fl.combine_words(fin, fin) == (4, fl.bits_of(1.0), fl.bits_of(2.0), fl.bits_of(6.0), 0)
    big = fc.words((1, 1.5e308, 1.5e308, 1.5e308, 0.0))
    assert fl.combine_words(big, big)[3:] == (fl.NAN_BITS, fl.NAN_BITS)                          # the overflow may come with the last (+)


# ---- the header, the binding ----
def test_header_states_the_contract():
    h = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"CRYO_KEY_FLOAT4\s*=\s*8\b", h) and re.search(r"CRYO_KEY_FLOAT8\s*=\s*9\b", h)
    assert re.search(r"typedef struct \{ uint64_t n; double min, max, sum, err; \} cryo_agg_cell_f;", h)
    assert "sizeof(cryo_agg_cell_f) == 40" in h
    for phrase in ("float8_cmp_internal", "2^-90", "TwoSum", "FastTwoSum", "0x7FF8000000000000", "value out of range: overflow"):
        assert phrase in h, phrase
    assert (cc.KEY_FLOAT4, cc.KEY_FLOAT8) == (8, 9) == (fl.FLOAT4, fl.FLOAT8)
    assert cc.AGG_CELL_F.itemsize == cc.AGG_CELL.itemsize == 40
    walk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "filter_walk.h")).read()
    assert re.search(r"kKeyFloat4 = 8u, kKeyFloat8 = 9u", walk)
    mk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bagg_float\.hip\b.*\bgroup_float\.hip\b", mk, flags=re.M)


def test_python_descriptors():
    f, a, k = cc.filter_desc(fc.ATTS, [(2, cc.KEY_FLOAT8, cc.OP_GT, 1.5), (3, cc.KEY_FLOAT4, cc.OP_EQ, fc.NAN_PAYLOAD),
                                       (2, cc.KEY_FLOAT8, cc.OP_LE, -0.0), (5, cc.KEY_FLOAT4, cc.OP_ISNULL, 0)])
    assert k["value"].tolist() == [fl.f8(1.5), fc.NAN_PAYLOAD, -(1 << 63), 0] and k["rsv"].tolist() == [0, 0, 0, 0]
    assert k["type"].tolist() == [9, 8, 9, 8]
    assert cc.float_key_bits(float("nan")) == fl.NAN_BITS
    _, cols = cc.agg_desc([(2, cc.KEY_FLOAT8), (1, cc.KEY_INT4)])
    assert cols["type"].tolist() == [9, 2]
    cell = fl.as_cell(fc.words((3, -1.5, fl.NAN_BITS, 2.0, 5e-324)))
    n, lo, hi, s, e = cc.cell_float(cell)
    assert (n, lo, s, e) == (3, -1.5, 2.0, 5e-324) and hi != hi
    for name, atts, keys, key_rsv, ok in fc.descriptors():
        assert fl.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
    assert fl.col_ok(fc.ATTS, (2, fl.FLOAT8)) and fl.col_ok(fc.ATTS, (5, fl.FLOAT4)) and not fl.col_ok(fc.ATTS, (2, fl.FLOAT8), group=True)
    assert not fl.col_ok(fc.ATTS, (6, fl.FLOAT4)) and not fl.col_ok([(8, 4)], (1, fl.FLOAT8))


# ---- the host walks, through a codec double ----
B128 = 131072
ATTS3 = [(4, 4), (8, 8), (4, 4)]                          # (rowid int4, x float8, y float4)


@pytest.fixture()
def HS():
    import float_double
    L = host.lib()
    dbl = float_double.FloatDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_filter_ops(C.byref(dbl.filter_ops))
    L.cryo_host_set_agg_ops(C.byref(dbl.agg_ops))
    L.cryo_host_set_group_ops(C.byref(dbl.group_ops))
    L.cryo_host_set_project_ops(C.byref(dbl.project_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_cache_shutdown()
    L.cryo_host_set_project_ops(None)
    L.cryo_host_set_group_ops(None)
    L.cryo_host_set_agg_ops(None)
    L.cryo_host_set_filter_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


def _x(r):
    """x of row r: a cancellation set spread over the blocks, an infinity-free relation"""
    return [fc.P900, 0.1 * r, -fc.P900, fc.M900, fc.P840, -1.5 * r][r % 6]


def _relation(L, oracle, nblocks=4, special=None):
    """nblocks chains of 40 tuples (rowid, x, y = rowid / 4), rowid from 1 on; even chains LZ4, odd ones zstd; special: {rowid: x}"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4243, C.byref(rel))
    raws = []
    for k in range(nblocks):
        rows = []
        for r in range(40 * k + 1, 40 * k + 41):
            x = (special or {}).get(r, _x(r))
            rows.append(tc.form_tuple(ATTS3, [r, None if r % 9 == 0 else x if isinstance(x, int) else fl.f8(x), fl.f4(r / 4)]))
        raw = tc.build_block(B128, rows)
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)
        raws.append(raw)
    return mem, rel, raws


def _words(cell):
    """the five unsigned words of a cell as host.aggregate_scan reports it: (n, min, max, 128-bit sum) of signed integers"""
    n, lo, hi, s = cell
    m = (1 << 64) - 1
    return (n, lo & m, hi & m, s & m, (s >> 64) & m)


def test_host_walks_combine_float_cells_by_type(HS, oracle):
    L, dbl, errors = HS
    keys, cols = [(3, fl.FLOAT4, fl.GT, 2.0), (2, fl.FLOAT8, fl.LE, float("nan"))], [(2, fl.FLOAT8), (1, fl.INT4), (3, fl.FLOAT4)]
    for special in (None, {50: fc.INF}, {50: fc.INF, 130: -fc.INF}, {77: fc.NAN_PAYLOAD}, {20: 1.5e308, 21: 1.5e308}):
        mem, rel, raws = _relation(L, oracle, special=special)
        events, t = host.aggregate_scan(rel, ATTS3, keys, cols)
        rows, cells = fl.agg_call(raws, ATTS3, keys, cols)
        per_block = [e[6] for e in events if e[0] == "block"]
        assert len(per_block) == 4 and t["matches"] == int(rows["n_match"].sum()) > 100
        want = [(0, 0, 0, 0, 0)] * 3
        for i in range(4):
            for j in (0, 2):
                got = _words(per_block[i][j])
                assert got == tuple(int(w) for w in np.frombuffer(cells[i, j].tobytes(), "<u8")), (special, i, j)
                want[j] = fl.combine_words(want[j], got)                                      # in block order
        assert _words(t["cells"][0]) == want[0] and _words(t["cells"][2]) == want[2], special
        rowids = [r for r in range(9, 161) if r % 9]                                           # y > 2 and x not NULL: x <= NaN holds for the rest
        assert t["cells"][1] == (len(rowids), rowids[0], rowids[-1], sum(rowids))              # the integer column, as ever
        n, lo, hi, s, e = cc.cell_float(fl.as_cell(want[0]))
        if special is None:
            vals = [(r, _x(r)) for r in rowids]
            exact = sum(Fraction(v) for _, v in vals)
            assert abs(Fraction(s) + Fraction(e) - exact) <= BOUND * sum(abs(Fraction(v)) for _, v in vals)
            assert (lo, hi) == (-fc.P900, fc.P900)
        elif len(special) == 2 and 50 in special:
            assert s != s and e == 0.0
        elif 50 in special:
            assert (s, e, hi) == (fc.INF, 0.0, fc.INF)
        elif 77 in special:
            assert s != s and e == 0.0 and hi != hi and lo == -fc.P900
        else:
            assert s != s and e != e                                                          # the overflow, kept through the combination
        L.cryo_memrel_destroy(mem)
    assert not errors


def test_host_walks_carry_float_keys(HS, oracle):
    L, dbl, errors = HS
    mem, rel, raws = _relation(L, oracle, nblocks=2)
    keys = [(2, fl.FLOAT8, fl.LT, -0.0), (3, fl.FLOAT4, fl.GE, 5.0)]
    want = [r for r in range(20, 81) if r % 9 and _x(r) < 0]
    events, t = host.filter_scan(rel, ATTS3, keys)
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == want and t["matches"] == len(want) > 10
    events, t = host.group_scan(rel, ATTS3, keys, [(1, fl.INT4)], [(2, fl.FLOAT8)])
    assert [g[0] for e in events if e[0] == "block" for g in e[6]] == [(r,) for r in want]
    assert [_words(g[2][0]) for e in events if e[0] == "block" for g in e[6]] == \
        [(1, fl.bits_of(_x(r)), fl.bits_of(_x(r)), fl.bits_of(_x(r)), 0) for r in want]
    events, t = host.project_scan(rel, ATTS3, keys, [2, 1])
    assert [struct.unpack("<di4x", e[5]) for e in events] == [(_x(r), r) for r in want]
    # the walks hand the keys through as the C ABI carries them: the double's bits in value
    assert all(k == [(2, fl.FLOAT8, fl.LT, -(1 << 63)), (3, fl.FLOAT4, fl.GE, fl.f8(5.0))] for k in dbl.keys_seen), dbl.keys_seen[0]
    for bad_keys, by in (([(2, fl.FLOAT8, fl.IN, [1])], [(1, fl.INT4)]), ([], [(2, fl.FLOAT8)])):
        with pytest.raises(host.GroupScanError) as e:
            host.group_scan(rel, ATTS3, bad_keys, by, [(2, fl.FLOAT8)])
        assert e.value.code == -1
    assert not errors
    L.cryo_memrel_destroy(mem)
