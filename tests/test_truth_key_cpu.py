"""CPU tests of the truth table over scan keys (CRYO_FILTER_TRUTH): tests/truth_key_ref.py against the hand-written expectations of
tests/truth_key_cases.py and against the older references (the AND table is the flag-less rule, a table from truth_dnf the union
of its terms' ANDed calls), an independent three-valued evaluator of expression trees against the table rule, the count of
monotone tables, truth_dnf in Python and in C against brute force, the descriptor rules with the older refusals, the header's
text, the Python wrapper's descriptors in host and device form, the four host walks through a codec double that checks flags
and rsv arrive as given, and the coverage conditions of the seeded generator the GPU property test uses."""
import ctypes as C
import itertools
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import bytes_key_cases as bc
import fetch_walk
import filter_cases as fc
import set_key_cases as sc
import set_key_ref as sr
import truth_key_cases as tk
import truth_key_ref as tr
import tuple_craft as tc
from pg_cryogen_amd import codec, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B128 = 131072
E_ARG = -1


# ---- the reference against the hand-written expectations ----
def test_reference_gives_the_hand_written_positions():
    names = set()
    for name, B, atts, blk, keys, W, matches, bad in tk.cases():
        assert tr.desc_ok(atts, keys, tr.TRUTH, W), name
        status, n, recs = tr.filter_block(blk, atts, keys, W)
        assert status == tr.OK, name
        assert [r[0] for r in recs if r[1] == tr.OK] == matches, name
        assert {r[0]: r[1] for r in recs if r[1] != tr.OK} == bad, name
        table = tr.filter_call([blk], atts, keys, tr.COUNT_ONLY, W)[0]
        assert (table["n_match"][0], table["n_bad"][0]) == (len(matches), len(bad)), name
        names.add(name)
    assert len(names) == len(tk.cases()) >= 14
    for turn in range(5):                                                    # the 290-item block: hits and misses in every turn
        inside = set(range(64 * turn + 1, min(64 * turn + 64, 290) + 1))
        assert inside & set(tk.BIG_MATCHES) and inside - set(tk.BIG_MATCHES), turn


def test_state_block_realises_every_combination():
    blk, states = tk.state_block()
    assert len(states) == 290 and len({tuple(s) for s in states}) == 3 * 3 * 2 * 2       # a NULL is F to these keys
    status, n, items = sr.br._items(blk)
    assert (status, n) == (tr.OK, 290)
    got = [tr.key_states(blk[off:off + ln].tobytes(), tk.STATE_ATTS, tk.STATE_KEYS) for pos, bad, off, ln in items]
    assert got == states                                                     # the reference reads the states the block was made from
    for turn in range(5):
        seen = {tuple(s) for s in states[64 * turn:64 * turn + 64]}
        assert any(tr.U in s for s in seen) and any(tr.U not in s for s in seen), turn
    for W in (tr.dnf([0b0011, 0b1100], 4), tr.dnf([1, 2, 4, 8], 4), tr.and_table(4), 0xFFFF):
        matches, und = tk.state_expect(states, W)
        recs = tr.filter_block(blk, tk.STATE_ATTS, tk.STATE_KEYS, W)[2]
        assert [r[0] for r in recs if r[1] == tr.OK] == matches and {r[0]: r[1] for r in recs if r[1] != tr.OK} == und
        assert (W == 0xFFFF) == (len(matches) == 290) and (und != {}) == (W != 0xFFFF)


# ---- the reference against the older references ----
def test_the_and_table_is_the_rule_without_the_flag():
    """on every case of the set keys and the byte-string keys, undecided ones included: records, bytes and totals"""
    checked = undecided = 0
    for name, B, atts, blk, keys, matches, bad in sc.cases() + bc.cases():
        if not keys:
            continue
        W = tr.and_table(len(keys))
        want, got = sr.filter_call([blk], atts, keys), tr.filter_call([blk], atts, keys, 0, W)
        for a, b in zip(want[:3], got[:3]):
            assert np.array_equal(a, b), name
        assert want[3] == got[3], name
        undecided += sr.UNDECIDED in bad.values()
        checked += 1
    assert checked >= 60 and undecided >= 3
    atts, blk = sc.big_block()
    keys, W = sc.BIG_KEYS + [(1, sr.INT4, sr.GE, 100)], tr.and_table(2)
    for a, b in zip(tr.agg_call([blk], atts, keys, [(1, sr.INT4)], W), sr.agg_call([blk], atts, keys, [(1, sr.INT4)])):
        assert np.array_equal(a, b)
    for a, b in zip(tr.group_call([blk], atts, keys, [(2, sr.INT4)], [(1, sr.INT4)], W), sr.group_call([blk], atts, keys, [(2, sr.INT4)], [(1, sr.INT4)])):
        assert np.array_equal(a, b)
    for a, b in zip(tr.project_call([blk, None], atts, keys, [2, 1], W), sr.project_call([blk, None], atts, keys, [2, 1])):
        assert np.array_equal(a, b)


def _positions(recs):
    return [r[0] for r in recs if r[1] == tr.OK]


def test_a_dnf_table_is_the_union_of_its_terms():
    """on blocks without undecided values: the matches under truth_dnf(terms) are the union over terms of the older reference's
    ANDed call on that term's keys"""
    rng = random.Random(7)
    checked = 0
    for name, B, atts, blk, keys, W, matches, bad in tk.cases():
        if tr.UNDECIDED in bad.values() or any(k[1] == tr.BYTES for k in keys):
            continue
        n = len(keys)
        for _ in range(6):
            terms = [rng.randrange(1, 1 << n) for _ in range(rng.randint(1, 3))]
            table = codec.truth_dnf(terms, n)
            union = set()
            for t in terms:
                union |= set(_positions(sr.filter_block(blk, atts, [k for i, k in enumerate(keys) if t >> i & 1])[2]))
            got = tr.filter_block(blk, atts, keys, table)[2]
            # a term's own call walks to its own highest column only: compare the matches among the tuples the full walk accepts
            walked = {r[0] for r in got if r[1] == tr.TUPLE}
            assert _positions(got) == sorted(union - walked), (name, terms)
            checked += 1
    assert checked >= 40


# ---- the table rule against three-valued logic ----
def _tree_dnf(W, n):
    """an OR of ANDs of leaves: one AND per minimal true point of W"""
    true = [m for m in range(1 << n) if W >> m & 1]
    minimal = [m for m in true if not any(o != m and o & m == o for o in true)]
    return ("or", [("and", [("leaf", k) for k in range(n) if m >> k & 1]) for m in minimal])


def _tree_cnf(W, n):
    """an AND of ORs of leaves: one OR per maximal false point of W, over the leaves that point lacks"""
    false = [m for m in range(1 << n) if not W >> m & 1]
    maximal = [m for m in false if not any(o != m and o & m == m for o in false)]
    return ("and", [("or", [("leaf", k) for k in range(n) if not m >> k & 1]) for m in maximal])


def _kleene(tree, leaves):
    """True, False or None (unknown), by Kleene's strong three-valued logic; an empty AND is true, an empty OR false"""
    kind, arg = tree
    if kind == "leaf":
        return leaves[arg]
    vals = [_kleene(t, leaves) for t in arg]
    if kind == "and":
        return False if any(v is False for v in vals) else None if any(v is None for v in vals) else True
    return True if any(v is True for v in vals) else None if any(v is None for v in vals) else False


def test_three_valued_logic_agrees_with_the_table_rule():
    """every monotone table of 1 .. 4 keys as two differently shaped trees of AND and OR, every one of the 3^n leaf states: the
    tree's Kleene value is TRUE / FALSE / UNKNOWN exactly where the table rule says match / no match / UNDECIDED, and TRUE exactly
    where the table has a 1 with every unknown leaf taken as false -- which is why leaves that are false on NULL lose nothing"""
    state = {True: tr.T, False: tr.F, None: tr.U}
    verdict = {True: tr.OK, False: tr.NOMATCH, None: tr.UNDECIDED}
    checked = 0
    for n in range(1, 5):
        for W in tr.monotone_tables(n):
            trees = (_tree_dnf(W, n), _tree_cnf(W, n))
            for leaves in itertools.product((True, False, None), repeat=n):
                t = sum(1 << k for k, v in enumerate(leaves) if v is True)
                for tree in trees:
                    k = _kleene(tree, leaves)
                    assert verdict[k] == tr.verdict_of([state[v] for v in leaves], W), (n, W, leaves, tree)
                    assert (k is True) == bool(W >> t & 1), (n, W, leaves)
                checked += 1
    assert checked == 2 * 3 + 5 * 9 + 19 * 27 + 167 * 81


def test_a_table_that_is_not_monotone_has_no_tree():
    """the other direction, for two keys: XOR, NOR and A AND NOT B are no value of any tree of AND and OR over the leaves"""
    reach = {0b1010, 0b1100}                                                 # the leaves A and B as tables
    for _ in range(3):
        reach |= {a & b for a in reach for b in reach} | {a | b for a in reach for b in reach}
    assert reach == {0b1010, 0b1100, 0b1000, 0b1110}
    assert all(tr.monotone(W, 2) for W in reach) and not any(tr.monotone(W, 2) for W in (0b0110, 0b0001, 0b0010))


def test_the_monotone_tables_are_counted_by_dedekind():
    assert [len(tr.monotone_tables(n)) for n in range(1, 5)] == [2, 5, 19, 167]
    for n in range(1, 5):
        tables = tr.monotone_tables(n)
        assert tr.and_table(n) in tables and (1 << (1 << n)) - 1 in tables and all(tr.table_ok(W, n) for W in tables)
    assert tr.and_table(2) == 0b1000 and tr.and_table(4) == 1 << 15


# ---- truth_dnf ----
def _dnf_queries():
    rng = random.Random(11)
    q = [(n, [rng.randrange(1, 1 << n) for _ in range(rng.randint(1, 5))]) for n in range(1, 5) for _ in range(40)]
    q += [(n, [t]) for n in range(1, 5) for t in range(1, 1 << n)]
    return q


BAD_DNF = [(2, []), (2, [0]), (2, [1, 0]), (2, [4]), (3, [1, 8]), (0, [1]), (5, [1]), (4, [16]), (1, [2])]


def test_truth_dnf_against_brute_force():
    for n, terms in _dnf_queries():
        W = codec.truth_dnf(terms, n)
        assert W == tr.dnf(terms, n) and tr.table_ok(W, n), (n, terms)
    assert codec.truth_dnf([0b0111, 0b1011], 4) == 0b1000100010000000         # A AND B AND (C OR D): masks 7, 11, 15
    assert codec.truth_dnf([1, 2], 2) == 0b1110 and codec.truth_dnf([3], 2) == tr.and_table(2)
    for n, terms in BAD_DNF:
        assert codec.truth_dnf(terms, n) == 0, (n, terms)
    # every valid table is the dnf of its minimal true points
    for n in range(1, 5):
        for W in tr.monotone_tables(n):
            if W & 1:
                continue                                                     # constant true has the empty term, which dnf refuses
            true = [m for m in range(1 << n) if W >> m & 1]
            assert codec.truth_dnf([m for m in true if not any(o != m and o & m == o for o in true)], n) == W


def test_the_c_helper_agrees(tmp_path):
    """cryo_filter_truth_dnf of host/filter.h in a small program of its own"""
    src = tmp_path / "dnf.c"
    src.write_text("""
#include "filter.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
int main(void)
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        uint32_t terms[16], n = 0, nkeys;
        char *tok = strtok(line, " \\n");
        nkeys = (uint32_t)strtoul(tok, 0, 0);
        while ((tok = strtok(0, " \\n")) && n < 16) terms[n++] = (uint32_t)strtoul(tok, 0, 0);
        printf("%u\\n", cryo_filter_truth_dnf(terms, n, nkeys));
    }
    printf("%u\\n", cryo_filter_truth_dnf(0, 1, 2));
    return 0;
}
""")
    exe = tmp_path / "dnf"
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pg_cryogen_amd", "host"),
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    queries = _dnf_queries() + BAD_DNF
    text = "".join("%d %s\n" % (n, " ".join(str(t) for t in terms)) for n, terms in queries)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True, timeout=60).stdout.split()
    assert len(out) == len(queries) + 1 and out[-1] == "0"                   # a null array
    for (n, terms), got in zip(queries, out):
        assert int(got) == codec.truth_dnf(terms, n), (n, terms, got)


# ---- the descriptor ----
def test_descriptor_rules():
    for name, atts, keys, flags, rsv, ok in tk.descriptors():
        assert tr.desc_ok(atts, keys, flags, rsv) == ok, name
        assert (tr.desc_ok(atts, keys, flags, rsv) and tr.reduce_flags_ok(flags)) == (ok and not flags & tr.COUNT_ONLY), name
    # the rules the filter, the byte-string keys and the set keys had before stand as they are, with and without a valid table
    for name, atts, keys, key_rsv, ok in sc.descriptors() + bc.descriptors():
        assert tr.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
        n = len(keys)
        assert tr.desc_ok(atts, keys, tr.TRUTH, (1 << (1 << min(n, 4))) - 1, key_rsv) == (ok and n >= 1), name
    for name, atts, keys, flags, patch, ok in fc.descriptors():
        if patch is None:
            assert tr.desc_ok(atts, keys, flags) == ok, name
    for W in range(16):                                                      # two keys: exactly the five monotone tables pass
        assert tr.desc_ok(sc.ATTS, [(5, tr.INT4, tr.GE, 1), (3, tr.INT8, tr.LT, 9)], tr.TRUTH, W) == (W in (0b1000, 0b1010, 0b1100, 0b1110, 0b1111))


def test_header_states_the_rule():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"^#define CRYO_FILTER_TRUTH 4u\b", txt, flags=re.M) and re.search(r"^#define CRYO_FILTER_COUNT_ONLY 1u\b", txt, flags=re.M)
    assert re.search(r"^#define CRYO_FILTER_MAX_KEYS 4u\b", txt, flags=re.M)
    assert re.search(r"uint32_t natts, nkeys, flags, rsv;", txt)
    flat = " ".join(txt.replace("\n *", " ").split())
    for phrase in ("Truth table.", "W is monotone when W[m] implies W[m | 1 << k] for every k < nkeys", "a match if W[t]",
                   "no match if not W[t | u]", "W = 1 << (2^nkeys - 1)", "Kleene", "cryo_filter_truth_dnf"):
        assert phrase in flat, phrase
    assert (codec.FILTER_TRUTH, codec.FILTER_COUNT_ONLY, codec.FILTER_MAX_KEYS) == (tr.TRUTH, tr.COUNT_ONLY, tr.MAX_KEYS) == (4, 1, 4)
    helper = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "filter.h")).read()
    assert "static inline uint32_t cryo_filter_truth_dnf(const uint32_t *terms, uint32_t nterms, uint32_t nkeys)" in helper


# ---- the wrapper's descriptors ----
def test_filter_desc_host_and_device_form():
    keys = [(2, codec.KEY_BYTES, codec.OP_EQ, b"de"), (5, codec.KEY_INT4, codec.OP_IN, [3, 4])]
    f, a, k = codec.filter_desc(sc.ATTS, keys, truth=0b1110)
    assert (f.natts, f.nkeys, f.flags, f.rsv) == (5, 2, codec.FILTER_TRUTH, 0b1110)
    f, a, k = codec.filter_desc(sc.ATTS, keys, codec.FILTER_COUNT_ONLY, codec.truth_dnf([1, 2], 2))
    assert (f.flags, f.rsv) == (codec.FILTER_TRUTH | codec.FILTER_COUNT_ONLY, 0b1110)
    assert C.string_at(int(k["value"][0]), 2) == b"de" and k["rsv"].tolist() == [2, 2]
    f, a, k = codec.filter_desc(sc.ATTS, keys, codec.FILTER_COUNT_ONLY)          # without a table: as before
    assert (f.flags, f.rsv) == (codec.FILTER_COUNT_ONLY, 0)
    assert (codec.filter_desc(sc.ATTS, keys)[0].flags, codec.filter_desc(sc.ATTS, keys, truth=0)[0].flags) == (0, codec.FILTER_TRUTH)
    a, k, consts, rebase = codec.filter_desc_device(sc.ATTS, keys, truth=0b1000)
    assert (rebase.flags, rebase.rsv) == (codec.FILTER_TRUTH, 0b1000) and bytes(consts[:2]) == b"de"
    assert rebase(4096) is k and k["value"].tolist() == [4096, 4098]
    a, k, consts, rebase = codec.filter_desc_device(sc.ATTS, keys)
    assert (rebase.flags, rebase.rsv) == (0, 0)
    assert codec.truth_flags(1, None) == (1, 0) and codec.truth_flags(1, 0xFFFF) == (5, 0xFFFF)


# ---- the seeded generator of the GPU property test ----
def test_seeded_generator_meets_its_coverage_conditions():
    descs = tk.property_descriptors()
    assert len(descs) == len(tk.PROPERTY_CASES) * tk.DESCS_PER_CASE
    for name, keys, W in descs:
        assert tr.desc_ok(tk.wg.case(name).call_atts, keys, tr.TRUTH, W), (name, keys, W)
    undecided, or_decided, matches, sizes = tk.property_coverage(descs)
    print(undecided, or_decided, matches, sizes)
    assert undecided >= len(descs) // 4 and or_decided >= len(descs) // 2 and matches > 500 and sizes == {1, 2, 3, 4}
    kinds = {("set" if sr.is_set_key(k) else "bytes" if k[1] == tr.BYTES else "null" if k[2] in (tr.ISNULL, tr.NOTNULL) else "int")
             for _, keys, _ in descs for k in keys}
    assert kinds == {"set", "bytes", "null", "int"}


# ---- the host walks, through a codec double ----
ATTS3 = [(4, 4), (-1, 4), (8, 8)]                       # (rowid int4, tag text, x int8)
KEYS = [(1, tr.INT4, tr.IN, [12, 17, 500]), (3, tr.INT8, tr.LE, -3 * 118), (2, tr.BYTES, tr.EQ, b"k1")]
TABLE = 0b11101110                                      # keys[0] OR keys[1]; the tag is evaluated and ignored
ROWS = [12, 17, 118, 119, 120]


@pytest.fixture()
def HS():
    import truth_key_double
    L = host.lib()
    dbl = truth_key_double.TruthKeyDouble()
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
    firsts = []
    for k in range(nblocks):
        raw = tc.build_block(B128, [tc.form_tuple(ATTS3, [r, None if r % 5 == 0 else b"k" + bytes([48 + r % 3]), -3 * r])
                                    for r in range(40 * k + 1, 40 * k + 41)])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
    return mem, rel, firsts


def test_the_four_host_walks_carry_flags_and_table(HS, oracle):
    L, dbl, errors = HS
    assert tr.table_ok(TABLE, 3) and TABLE == codec.truth_dnf([0b001, 0b010], 3)
    mem, rel, firsts = _relation(L, oracle)
    events, t = host.filter_scan(rel, ATTS3, KEYS, truth=TABLE)
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == ROWS
    assert (t["blocks"], t["items"], t["matches"], t["bad"]) == (3, 120, len(ROWS), 0)
    events, c = host.filter_scan(rel, ATTS3, KEYS, tr.COUNT_ONLY, TABLE)     # host/filter.c reads COUNT_ONLY beside the other bit
    assert events == [] and c["matches"] == len(ROWS)
    events, t = host.filter_scan(rel, ATTS3, KEYS)                           # no table: ANDed, nothing passes all three
    assert [e for e in events if e[0] == "tuple"] == [] and t["matches"] == 0
    events, t = host.aggregate_scan(rel, ATTS3, KEYS, [(1, tr.INT4)], truth=TABLE)
    assert t["cells"][0] == (len(ROWS), 12, 120, sum(ROWS))
    events, t = host.group_scan(rel, ATTS3, KEYS, [(1, tr.INT4)], [(3, tr.INT8)], truth=TABLE)
    assert (t["matches"], t["groups"], t["bad"]) == (len(ROWS), len(ROWS), 0)
    events, t = host.project_scan(rel, ATTS3, KEYS, [3, 1], truth=TABLE)
    assert [struct.unpack("<qi4x", e[5]) for e in events] == [(-3 * r, r) for r in ROWS]
    # flags and rsv arrived as the caller set them, in every codec call of every walk
    T4 = tr.TRUTH
    seen = {w for w in dbl.words_seen}
    assert seen == {("filter", T4, TABLE), ("filter", T4 | tr.COUNT_ONLY, TABLE), ("filter", 0, 0), ("agg", T4, TABLE), ("group", T4, TABLE),
                    ("project", T4, TABLE)}
    assert all(keys == KEYS for keys in dbl.keys_seen)
    # descriptors the codec refuses: XOR, a table of 0, a bit beyond 2^3; and COUNT_ONLY stays refused by the aggregate
    for bad in (0b00000110, 0, 1 << 8):
        assert not tr.table_ok(bad, 3)
        with pytest.raises(host.FilterScanError) as e:
            host.filter_scan(rel, ATTS3, KEYS, truth=bad)
        assert e.value.code == E_ARG
    with pytest.raises(host.FilterScanError) as e:
        host.filter_scan(rel, ATTS3, KEYS[:2], truth=0b0110)
    assert e.value.code == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)
