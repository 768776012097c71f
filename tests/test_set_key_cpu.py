"""CPU tests of the set scan keys (CRYO_OP_IN, CRYO_OP_NOT_IN): tests/set_key_ref.py against the hand-written expectations of
tests/set_key_cases.py and against the older references (IN of one member is =, IN of a set is the union of one = call per
member, NOT IN its complement among the non-NULL values), the descriptor rules with the older refusals, the header's text, the
Python wrapper's descriptors in host and device form, the four host walks through a codec double that reads the list from the
address the ABI carries, and the coverage conditions of the seeded generator the GPU property test uses."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import bytes_key_cases as bc
import fetch_walk
import filter_cases as fc
import filter_ref as fr
import set_key_cases as sc
import set_key_ref as sr
import tuple_craft as tc
from pg_cryogen_amd import codec, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B128 = 131072
E_ARG = -1


# ---- the reference against the hand-written expectations ----
def test_reference_gives_the_hand_written_positions():
    names = set()
    for name, B, atts, blk, keys, matches, bad in sc.cases():
        status, n, recs = sr.filter_block(blk, atts, keys)
        assert status == sr.OK, name
        assert [r[0] for r in recs if r[1] == sr.OK] == matches, name
        assert {r[0]: r[1] for r in recs if r[1] != sr.OK} == bad, name
        table = sr.filter_call([blk], atts, keys, sr.COUNT_ONLY)[0]
        assert (table["n_match"][0], table["n_bad"][0]) == (len(matches), len(bad)), name
        names.add(name)
    assert len(names) == len(sc.cases()) >= 2 * len(sc.SIZES) + 18
    assert {sc.LINEAR, sc.LINEAR + 1, 1, 2, 3, 63, 64, 65, 1023, 1024} == set(sc.SIZES)
    for turn in range(5):                                                    # the 290-item block: hits and misses in every turn
        inside = [p for p in range(64 * turn + 1, min(64 * turn + 64, 290) + 1)]
        assert set(inside) & set(sc.BIG_MATCHES) and set(inside) - set(sc.BIG_MATCHES), turn


def _positions(ref, blk, atts, keys):
    return [r[0] for r in ref.filter_block(blk, atts, keys)[2] if r[1] == sr.OK]


def test_in_is_the_union_of_equalities_and_not_in_its_complement():
    """through the older filter_ref, one = call per member; a member outside the type's range has no = call to make"""
    checked = 0
    for name, B, atts, blk, keys, matches, bad in sc.cases():
        if len(keys) != 1 or bad:
            continue
        att, typ, op, value = keys[0]
        size = sr.KEY_SIZE[typ]
        fit = sorted({m for m in value if -(1 << (8 * size - 1)) <= m < (1 << (8 * size - 1))})
        union = sorted(set().union(*[_positions(fr, blk, atts, [(att, typ, sr.EQ, m)]) for m in fit]))
        notnull = _positions(fr, blk, atts, [(att, typ, sr.NOTNULL, 0)])
        got = _positions(sr, blk, atts, keys)
        assert got == (union if op == sr.IN else [p for p in notnull if p not in union]), name
        if len(set(value)) == 1:
            assert _positions(sr, blk, atts, [(att, typ, sr.IN, value)]) == _positions(fr, blk, atts, [(att, typ, sr.EQ, value[0])]), name
            assert _positions(sr, blk, atts, [(att, typ, sr.NOT_IN, value)]) == _positions(fr, blk, atts, [(att, typ, sr.NE, value[0])]), name
        checked += 1
    assert checked >= 20


def test_without_a_set_key_the_references_agree():
    for name, B, atts, blk, keys, matches, bad in bc.cases()[::7]:
        assert np.array_equal(sr.filter_call([blk], atts, keys)[1], sr.br.filter_call([blk], atts, keys)[1]), name
    atts, blk = sc.big_block()
    plain = [(2, sr.INT4, sr.GE, 0)]
    for a, b in zip(sr.agg_call([blk], atts, plain, [(1, sr.INT4)]), sr.br.agg_call([blk], atts, plain, [(1, sr.INT4)])):
        assert np.array_equal(a, b)
    for a, b in zip(sr.project_call([blk, None], atts, plain, [2, 1]), sr.pr.project_call([blk, None], atts, plain, [2, 1])):
        assert np.array_equal(a, b)
    for a, b in zip(sr.group_call([blk], atts, plain, [(2, sr.INT4)], [(1, sr.INT4)]), sr.br.group_call([blk], atts, plain, [(2, sr.INT4)], [(1, sr.INT4)])):
        assert np.array_equal(a, b)


def test_aggregate_group_and_projection_see_the_set():
    atts, blk = sc.big_block()
    rows, cells = sr.agg_call([blk, None], atts, sc.BIG_KEYS, [(1, sr.INT4), (2, sr.INT4)])
    ids = sc.BIG_MATCHES
    assert tuple(rows[0]) == (sr.OK, 290, len(ids), 0) and tuple(rows[1]) == (sr.STREAM, 0, 0, 0)
    assert tuple(cells[0, 0])[:4] == (len(ids), ids[0], ids[-1], sum(ids)) and tuple(cells[0, 1])[:3] == (len(ids), -5, 3)
    rows, recs, cells, total = sr.group_call([blk], atts, sc.BIG_KEYS, [(2, sr.INT4)], [(1, sr.INT4)])
    assert total == 3 and recs["key"][:, 0].tolist() == [-5, 0, 3] and int(recs["n_rows"].sum()) == len(ids)
    table, recs, out, (tw, tr) = sr.project_call([blk], atts, sc.BIG_KEYS, [2, 1])
    assert (tw, tr) == (len(ids), len(ids)) and recs["pos"].tolist() == ids
    assert [struct.unpack("<ii", bytes(r)) for r in out] == [(i % 11 - 5, i) for i in ids]


# ---- the descriptor ----
def test_descriptor_rules():
    for name, atts, keys, key_rsv, ok in sc.descriptors():
        assert sr.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
    # the rules the filter and the byte-string keys had before stand as they are
    for name, atts, keys, key_rsv, ok in bc.descriptors():
        assert sr.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
    for name, atts, keys, flags, patch, ok in fc.descriptors():
        if patch is None:
            assert sr.desc_ok(atts, keys, flags) == fr.desc_ok(atts, keys, flags) == ok, name
        elif patch[0] == "k":
            assert not sr.desc_ok(atts, keys, flags, 0, [patch[3]]), name


def test_header_states_the_ops_and_the_limit():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"typedef struct \{ uint16_t att; uint8_t type, op; uint32_t rsv; int64_t value; \} cryo_scan_key;", txt)
    assert re.search(r"CRYO_OP_LT = 1, CRYO_OP_LE, CRYO_OP_EQ, CRYO_OP_GE, CRYO_OP_GT, CRYO_OP_NE, CRYO_OP_ISNULL, CRYO_OP_NOTNULL,", txt)
    assert re.search(r"\bCRYO_OP_IN = 9, CRYO_OP_NOT_IN = 10\b", txt)
    assert re.search(r"^#define CRYO_KEY_SET_MAX 1024u\b", txt, flags=re.M)
    assert re.search(r"^#define CRYO_KEY_BYTES_MAX 256u\b", txt, flags=re.M) and re.search(r"^#define CRYO_FILTER_MAX_KEYS 4u\b", txt, flags=re.M)
    assert (codec.OP_IN, codec.OP_NOT_IN, codec.KEY_SET_MAX) == (sr.IN, sr.NOT_IN, sr.SET_MAX) == (9, 10, 1024)
    walk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "filter_walk.h")).read()
    assert re.search(r"kSetLinear = %du\b" % sc.LINEAR, walk)                # the cases stand on both sides of the kernels' threshold


# ---- the wrapper's descriptors ----
def _list_at(address, n):
    return np.frombuffer(C.string_at(address, 8 * n), "<i8").tolist()


def test_filter_desc_host_form():
    keys = [(2, codec.KEY_BYTES, codec.OP_GE, b"abc"), (5, codec.KEY_INT4, codec.OP_IN, [7, -1, 7, 1 << 40]), (1, codec.KEY_INT4, codec.OP_GT, 7),
            (3, codec.KEY_INT8, codec.OP_NOT_IN, (sc.I64_MIN, sc.I64_MAX))]
    f, a, k = codec.filter_desc(sc.ATTS, keys)
    assert (f.natts, f.nkeys, f.keys) == (5, 4, k.ctypes.data)
    assert k["rsv"].tolist() == [3, 4, 0, 2] and k["op"].tolist() == [4, 9, 5, 10] and k["type"].tolist() == [16, 2, 2, 3] and k["value"][2] == 7
    base = f.consts.ctypes.data                                              # the struct keeps constants and lists alive
    assert [int(v) - base for v in k["value"][[0, 1, 3]]] == [0, 3, 35]      # back to back: the first list at an odd offset
    assert C.string_at(int(k["value"][0]), 3) == b"abc"
    assert _list_at(int(k["value"][1]), 4) == [7, -1, 7, 1 << 40] and _list_at(int(k["value"][3]), 2) == [sc.I64_MIN, sc.I64_MAX]
    assert f.consts.nbytes >= 3 + 32 + 16
    # no member: no address; integer keys alone: as before
    f, a, k = codec.filter_desc(sc.ATTS, [(5, codec.KEY_INT4, codec.OP_IN, [])])
    assert tuple(k[0]) == (5, 2, 9, 0, 0)
    f, a, k = codec.filter_desc(sc.ATTS, [(1, codec.KEY_INT4, codec.OP_EQ, -5)])
    assert tuple(k[0]) == (1, 2, 3, 0, -5)


def test_filter_desc_device_form():
    keys = [(2, codec.KEY_BYTES, codec.OP_EQ, b"abcde"), (5, codec.KEY_INT4, codec.OP_IN, [3, -3]), (4, codec.KEY_INT2, codec.OP_NOT_IN, [9]),
            (1, codec.KEY_INT4, codec.OP_GT, 7)]
    a, k, consts, rebase = codec.filter_desc_device(sc.ATTS, keys)
    assert bytes(consts[:5]) == b"abcde" and bytes(consts[5:29]) == struct.pack("<qqq", 3, -3, 9)
    assert rebase(0x7F0000001001) is k
    assert k["value"].tolist() == [0x7F0000001001, 0x7F0000001006, 0x7F0000001016, 7] and k["rsv"].tolist() == [5, 2, 1, 0]
    rebase(4096)                                                             # again, from the offsets
    assert k["value"].tolist() == [4096, 4101, 4117, 7]
    assert a.dtype == codec.FILTER_ATT and a.size == 5


# ---- the seeded generator of the GPU property test ----
def test_seeded_generator_meets_its_coverage_conditions():
    blocks, key_sets = sc.random_blocks(), sc.random_key_sets()
    assert len(blocks) == 64 and len(key_sets) == sc.TURNS
    for keys in key_sets:
        assert 1 <= len(keys) <= 4 and any(sr.is_set_key(k) for k in keys) and sr.desc_ok(sc.ATTS, keys), keys
    seen, matches, rejected = sc.coverage(blocks, key_sets)
    print(seen, matches, rejected)
    for n in sc.SIZES:
        assert seen.get(n, [0, 0])[0] > 0 and seen[n][1] > 0, (n, seen)     # a match and a non-match on a non-NULL value
    assert matches > 500 and rejected > 500, (matches, rejected)
    assert len({len(k) for k in key_sets}) == 4                             # one, two, three and four keys occur


# ---- the host walks, through a codec double ----
ATTS3 = [(4, 4), (-1, 4), (8, 8)]                       # (rowid int4, tag text, x int8)
WANTED = [12, 17, 17, 33, 40, 41, 80, 81, 119, 500, -4, 1 << 33]
KEYS = [(1, sr.INT4, sr.IN, WANTED), (3, sr.INT8, sr.NOT_IN, [-3 * 40, -3 * 80])]


@pytest.fixture()
def HS():
    import set_key_double
    L = host.lib()
    dbl = set_key_double.SetKeyDouble()
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


def _relation(L, oracle, nblocks=3):
    """nblocks chains of 40 tuples (rowid, tag, x = -3 rowid), rowid from 1 on; even chains LZ4, odd ones zstd, xid 500 + k"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4242, C.byref(rel))
    raws, firsts = [], []
    for k in range(nblocks):
        raw = tc.build_block(B128, [tc.form_tuple(ATTS3, [r, None if r % 5 == 0 else b"k" + bytes([48 + r % 3]), -3 * r])
                                    for r in range(40 * k + 1, 40 * k + 41)])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


ROWS = [12, 17, 33, 41, 81, 119]                        # WANTED within 1 .. 120, less rows 40 and 80, whose x the second key names


def test_the_four_host_walks_carry_the_list(HS, oracle):
    L, dbl, errors = HS
    mem, rel, raws, firsts = _relation(L, oracle)
    events, t = host.filter_scan(rel, ATTS3, KEYS)
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == ROWS
    assert (t["blocks"], t["items"], t["matches"], t["bad"]) == (3, 120, len(ROWS), 0)
    events, c = host.filter_scan(rel, ATTS3, KEYS, fr.COUNT_ONLY)
    assert events == [] and c["matches"] == len(ROWS)
    events, t = host.aggregate_scan(rel, ATTS3, KEYS, [(3, sr.INT8), (1, sr.INT4)])
    assert t["cells"][0] == (len(ROWS), -3 * ROWS[-1], -3 * ROWS[0], -3 * sum(ROWS)) and t["cells"][1] == (len(ROWS), 12, 119, sum(ROWS))
    assert [(e[3], e[4], e[5]) for e in events if e[0] == "block"] == [(40, 3, 0), (40, 1, 0), (40, 2, 0)]
    events, t = host.group_scan(rel, ATTS3, KEYS, [(1, sr.INT4)], [(3, sr.INT8)])
    assert (t["matches"], t["groups"], t["bad"]) == (len(ROWS), len(ROWS), 0)
    assert [g[0] for e in events if e[0] == "block" for g in e[6]] == [(r,) for r in ROWS]
    events, t = host.project_scan(rel, ATTS3, KEYS, [3, 1])
    assert [(e[0], e[1], e[2], e[4]) for e in events] == [("row", firsts[(r - 1) // 40], (r - 1) % 40 + 1, 0) for r in ROWS]
    assert [struct.unpack("<qi4x", e[5]) for e in events] == [(-3 * r, r) for r in ROWS]
    # every call saw the caller's lists, in the caller's order, through the address in the key
    assert {c[0] for c in dbl.calls} == {"filter", "agg", "group", "project"}
    assert all(keys == KEYS for keys in dbl.keys_seen), dbl.keys_seen[0]
    # a descriptor the codec refuses: a set key on the text column, and a list of 1 025 members
    for bad in ([(2, sr.INT4, sr.IN, [1])], [(1, sr.INT4, sr.IN, list(range(1025)))]):
        with pytest.raises(host.FilterScanError) as e:
            host.filter_scan(rel, ATTS3, bad)
        assert e.value.code == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)
