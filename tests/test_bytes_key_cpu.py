"""CPU tests of the byte-string scan keys: tests/bytes_key_ref.py against the hand-written expectations of
tests/bytes_key_cases.py, the descriptor rules, the header's text, the Python wrapper's descriptors in host and device form, and
the three host walks (host/filter.c, host/aggregate.c, host/group.c) through a codec double that answers by the rules: reason 9
is reported, and an undecided tuple counts as bad."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import agg_ref as ar
import bytes_key_cases as bc
import bytes_key_ref as br
import fetch_walk
import filter_cases as fc
import filter_ref as fr
import tuple_craft as tc
from pg_cryogen_amd import codec, host
from tuple_craft import Toast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B128 = 131072
E_ARG = -1


# ---- the reference against the hand-written expectations ----
def test_reference_gives_the_hand_written_positions():
    seen = set()
    for name, B, atts, blk, keys, matches, bad in bc.cases():
        status, n, recs = br.filter_block(blk, atts, keys)
        assert status == br.OK, name
        assert [r[0] for r in recs if r[1] == br.OK] == matches, name
        assert {r[0]: r[1] for r in recs if r[1] != br.OK} == bad, name
        assert all(r[2] == 0 for r in recs if r[1] != br.OK), name                  # an undecided tuple has no bytes
        table = br.filter_call([blk], atts, keys, br.COUNT_ONLY)[0]
        assert (table["n_match"][0], table["n_bad"][0]) == (len(matches), len(bad)), name
        seen.add(name)
    assert len(seen) == len(bc.cases()) > 13 * 6


def test_reference_compare_is_memcmp_then_length():
    for a, b, c in ((b"", b"", 0), (b"", b"a", -1), (b"a", b"", 1), (b"ab", b"abc", -1), (b"abc", b"ab", 1), (b"\x7f", b"\x80", -1),
                    (b"\xff", b"\x00", 1), (b"a\x00", b"a", 1), (b"b", b"ab", 1), (b"ab\xee", b"ab", 1)):
        assert br.compare_bytes(a, b) == c, (a, b)


def test_aggregate_and_group_treat_undecided_as_bad():
    """an undecided tuple counts in n_bad and is in no cell and no group; without a byte-string key the references agree"""
    atts = [(4, 4), (-1, 4), (8, 8)]
    tuples = [tc.form_tuple(atts, [r, Toast() if r % 7 == 0 else b"k" + bytes([48 + r % 3]), 100 * r]) for r in range(1, 22)]
    blk = tc.build_block(4096, tuples)
    keys = [(2, br.BYTES, br.EQ, b"k1")]
    rows, cells = br.agg_call([blk, None], atts, keys, [(3, br.INT8), (1, br.INT4)])
    assert tuple(rows[0]) == (br.OK, 21, 6, 3) and tuple(rows[1]) == (br.STREAM, 0, 0, 0)       # 1 4 10 13 16 19; 7 14 21
    assert tuple(cells[0, 0])[:4] == (6, 100, 1900, 6300) and tuple(cells[0, 1])[:4] == (6, 1, 19, 63)
    rows, recs, cells, total = br.group_call([blk], atts, keys, [(1, br.INT4)], [(3, br.INT8)])
    assert (rows["n_match"][0], rows["n_bad"][0], rows["n_groups"][0], total) == (6, 3, 6, 6)
    assert recs["key"][:, 0].tolist() == [1, 4, 10, 13, 16, 19]
    plain = [(1, br.INT4, br.GT, 5)]
    assert np.array_equal(br.filter_call([blk], atts, plain)[1], fr.filter_call([blk], atts, plain)[1])
    assert np.array_equal(br.agg_call([blk], atts, plain, [(3, br.INT8)])[1], ar.agg_call([blk], atts, plain, [(3, br.INT8)])[1])


# ---- the descriptor ----
def test_descriptor_rules():
    for name, atts, keys, key_rsv, ok in bc.descriptors():
        assert br.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
    # the rules the filter had before stand as they are: the two rule sets coexist
    for name, atts, keys, flags, patch, ok in fc.descriptors():
        if patch is None:
            assert br.desc_ok(atts, keys, flags) == fr.desc_ok(atts, keys, flags) == ok, name
        elif patch[0] == "k":
            assert not br.desc_ok(atts, keys, flags, 0, [patch[3]]), name


def test_header_states_the_constants_and_keeps_the_key():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"typedef struct \{ uint16_t att; uint8_t type, op; uint32_t rsv; int64_t value; \} cryo_scan_key;", txt)
    assert re.search(r"CRYO_KEY_INT2 = 1, CRYO_KEY_INT4 = 2, CRYO_KEY_INT8 = 3", txt)
    assert re.search(r"\bCRYO_KEY_BYTES = 16\b", txt)
    assert re.search(r"^#define CRYO_KEY_BYTES_MAX 256u\b", txt, flags=re.M)
    assert re.search(r"^#define CRYO_FILTER_UNDECIDED 9u\b", txt, flags=re.M)
    assert re.search(r"^#define CRYO_FILTER_TUPLE 8u\b", txt, flags=re.M)
    assert len(re.findall(r"or are undecided|undecided\)", txt)) >= 2               # n_bad's wording in the aggregate and the grouping
    assert (codec.KEY_BYTES, codec.KEY_BYTES_MAX, codec.FILTER_UNDECIDED) == (br.BYTES, br.BYTES_MAX, br.UNDECIDED) == (16, 256, 9)


# ---- the wrapper's descriptors ----
def test_filter_desc_host_form():
    keys = [(3, codec.KEY_BYTES, codec.OP_GE, b"abc"), (1, codec.KEY_INT4, codec.OP_GT, 7), (3, codec.KEY_BYTES, codec.OP_LT, b"abd\xff"),
            (5, codec.KEY_BYTES, codec.OP_EQ, b"")]
    desc = codec.filter_desc(bc.ATTS, keys)
    assert len(desc) == 3                                                            # existing callers unpack three
    f, a, k = desc
    assert (f.natts, f.nkeys, f.keys) == (5, 4, k.ctypes.data) and k.dtype == codec.FILTER_KEY and k.itemsize == 16
    assert k["rsv"].tolist() == [3, 0, 4, 0] and k["type"].tolist() == [16, 2, 16, 16] and k["value"][1] == 7
    assert C.string_at(int(k["value"][0]), 3) == b"abc" and C.string_at(int(k["value"][2]), 4) == b"abd\xff"
    assert k["value"][3] == 0                                                        # an empty constant: no address needed
    base = f.consts.ctypes.data                                                      # the struct keeps the constants alive
    assert base <= int(k["value"][0]) < int(k["value"][2]) < base + f.consts.nbytes
    # integer keys alone: as before
    f, a, k = codec.filter_desc(bc.ATTS, [(1, codec.KEY_INT4, codec.OP_EQ, -5)])
    assert tuple(k[0]) == (1, 2, 3, 0, -5)


def test_filter_desc_device_form():
    keys = [(3, codec.KEY_BYTES, codec.OP_GE, b"abc"), (1, codec.KEY_INT4, codec.OP_GT, 7), (3, codec.KEY_BYTES, codec.OP_LT, b"abd\xff")]
    a, k, consts, rebase = codec.filter_desc_device(bc.ATTS, keys)
    assert bytes(consts[:7]) == b"abcabd\xff"                                       # back to back: the second at an odd address
    assert rebase(0x7F0000001001) is k
    assert k["value"].tolist() == [0x7F0000001001, 7, 0x7F0000001004] and k["rsv"].tolist() == [3, 0, 4]
    rebase(4096)                                                                     # again, from the offsets
    assert k["value"].tolist() == [4096, 7, 4099]
    assert a.dtype == codec.FILTER_ATT and a.size == 5


# ---- the host walks, through a codec double ----
ATTS3 = [(4, 4), (-1, 4), (8, 8)]                       # (rowid int4, tag text, x int8)
KEYS = [(2, br.BYTES, br.EQ, b"k1"), (1, br.INT4, br.GT, 10)]


def _tag(r):
    return Toast() if r % 7 == 0 else None if r % 5 == 0 else b"k" + bytes([48 + r % 3])


@pytest.fixture()
def HB():
    import bytes_key_double
    L = host.lib()
    dbl = bytes_key_double.BytesKeyDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_filter_ops(C.byref(dbl.filter_ops))
    L.cryo_host_set_agg_ops(C.byref(dbl.agg_ops))
    L.cryo_host_set_group_ops(C.byref(dbl.group_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_cache_shutdown()
    L.cryo_host_set_group_ops(None)
    L.cryo_host_set_agg_ops(None)
    L.cryo_host_set_filter_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


def _relation(L, oracle, nblocks=3):
    """nblocks chains of 40 tuples (rowid, tag, x = -3 rowid); tag: an external pointer when rowid % 7 == 0, else NULL when
    rowid % 5 == 0, else 'k0' / 'k1' / 'k2' by rowid % 3.  Even chains LZ4, odd ones zstd, xid 500 + k"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws, firsts = [], []
    for k in range(nblocks):
        raw = tc.build_block(B128, [tc.form_tuple(ATTS3, [r, _tag(r), -3 * r]) for r in range(40 * k + 1, 40 * k + 41)])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def test_filter_scan_reports_reason_9(HB, oracle):
    L, dbl, errors = HB
    mem, rel, raws, firsts = _relation(L, oracle)
    events, t = host.filter_scan(rel, ATTS3, KEYS)
    want_rows = [r for r in range(11, 121) if r % 3 == 1 and r % 7 and r % 5]
    want_und = [r for r in range(11, 121) if r % 7 == 0]
    assert want_rows[:7] == [13, 16, 19, 22, 31, 34, 37] and want_und[:4] == [14, 21, 28, 35]
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == want_rows
    assert [e for e in events if e[0] == "report"] == [("report", firsts[(r - 1) // 40], br.UNDECIDED, (r - 1) % 40 + 1) for r in want_und]
    at = events.index(("report", firsts[0], br.UNDECIDED, 14))                       # in position order, between the tuples
    assert events[at - 1][:3] == ("tuple", firsts[0], 13) and events[at + 1][:3] == ("tuple", firsts[0], 16)
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"]) == (3, 120, len(want_rows), len(want_und), len(want_und))
    assert t["bytes_back"] == 32 * 3 + 8 * (len(want_rows) + len(want_und)) + sum(fr.maxalign(len(e[4])) for e in events if e[0] == "tuple")
    # COUNT_ONLY: counted, not reported
    events, c = host.filter_scan(rel, ATTS3, KEYS, fr.COUNT_ONLY)
    assert events == [] and (c["matches"], c["bad"], c["reports"]) == (len(want_rows), len(want_und), 0)
    # an integer key that is false makes the undecided tuple a silent no match
    events, t = host.filter_scan(rel, ATTS3, [KEYS[0], (1, br.INT4, br.LT, 14)])
    assert [e[:3] for e in events] == [("tuple", firsts[0], 1), ("tuple", firsts[0], 4), ("report", firsts[0], br.UNDECIDED),
                                       ("tuple", firsts[0], 13)] and events[2][3] == 7 and (t["bad"], t["reports"]) == (1, 1)
    # a descriptor the codec refuses: a byte-string key on the int8 column
    with pytest.raises(host.FilterScanError) as e:
        host.filter_scan(rel, ATTS3, [(3, br.BYTES, br.EQ, b"k1")])
    assert e.value.code == E_ARG
    assert [c[0] for c in dbl.calls] and not errors
    L.cryo_memrel_destroy(mem)


def test_aggregate_scan_counts_undecided_as_bad(HB, oracle):
    L, dbl, errors = HB
    mem, rel, raws, firsts = _relation(L, oracle)
    events, t = host.aggregate_scan(rel, ATTS3, KEYS, [(3, br.INT8)])
    blocks = [e for e in events if e[0] == "block"]
    want = [br.agg_call([raw], ATTS3, KEYS, [(3, br.INT8)]) for raw in raws]
    assert [(e[3], e[4], e[5]) for e in blocks] == [(40, int(w[0]["n_match"][0]), int(w[0]["n_bad"][0])) for w in want]
    assert [(e[4], e[5]) for e in blocks][0] == (7, 4)                               # 13 16 19 22 31 34 37; 14 21 28 35
    rows = [r for r in range(11, 121) if r % 3 == 1 and r % 7 and r % 5]
    assert t["cells"][0] == (len(rows), -3 * rows[-1], -3 * rows[0], -3 * sum(rows))
    assert (t["matches"], t["bad"], t["reports"]) == (len(rows), len([r for r in range(11, 121) if r % 7 == 0]), 0)
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_group_scan_counts_undecided_as_bad(HB, oracle):
    L, dbl, errors = HB
    mem, rel, raws, firsts = _relation(L, oracle)
    events, t = host.group_scan(rel, ATTS3, KEYS, [(1, br.INT4)], [(3, br.INT8)])
    blocks = [e for e in events if e[0] == "block"]
    assert [(e[3], e[4], e[5]) for e in blocks][0] == (40, 7, 4)
    assert [g[0] for g in blocks[0][6]] == [(r,) for r in (13, 16, 19, 22, 31, 34, 37)]  # an undecided tuple is in no group
    rows = [r for r in range(11, 121) if r % 3 == 1 and r % 7 and r % 5]
    assert (t["matches"], t["groups"], t["bad"]) == (len(rows), len(rows), len([r for r in range(11, 121) if r % 7 == 0]))
    assert not errors
    L.cryo_memrel_destroy(mem)
