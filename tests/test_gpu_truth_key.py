"""GPU tests of the truth table over scan keys (CRYO_FILTER_TRUTH) in cryo_codec_filter_batch / _agg_batch / _group_batch /
_project_batch, their host-buffer forms and cryo_multi_*_blocks.

Every row, record, cell and byte is compared with tests/truth_key_ref.py, the plain-Python statement of the rules in
include/cryo_codec.h, applied to the blocks the ORACLE encoded; the hand-made blocks of tests/truth_key_cases.py also carry their
expectations written out by hand, and the block of all key states its expectations by construction.  Outputs are filled with a
sentinel before every call, and after every device-resident call the caller's key array is read back: the library must not have
written it."""
import ctypes as C

import numpy as np
import pytest

import scan_calls
import set_key_ref as sr
import truth_calls as tcall
import truth_key_cases as tk
import truth_key_ref as tr
import tuple_craft as tc
import walk_gen as wg
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import (REC_SENTINEL, SENTINEL, Encoder, multi_call, same_agg, same_fields, same_filter, same_group, same_project)

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def columns(atts):
    """(aggregate columns, group columns, projected columns) of a descriptor of the cases"""
    if len(atts) == 2:
        return [(2, tr.INT4), (1, tr.INT4)], [(2, tr.INT4)], [2, 1]
    return [(5, tr.INT4), (3, tr.INT8), (4, tr.INT2)], [(5, tr.INT4)], [5, 3, 1, 4]


def other_block(B, atts):
    if len(atts) == 2:
        return tc.build_block(B, [tc.form_tuple(atts, [i, i % 7 - 3]) for i in range(1, 40)])
    return tc.build_block(B, [tk.T(i, tc.Toast() if i % 6 == 0 else b"de" if i % 2 else b"r" * (i % 5), 7 * (i % 9) - 21, i % 4 - 1,
                                   None if i % 13 == 0 else i % 11) for i in range(1, 31)])


def batch(idx, blk, B, atts, sizes=(1, 4, 5, 9)):
    """a lone wave, a full workgroup, one over, two over (the group: two waves per workgroup), alternating with other tuples"""
    return [blk if j % 2 == 0 else other_block(B, atts) for j in range(sizes[idx % len(sizes)])]


# ---- all tables ----
def test_all_167_tables_on_every_combination_of_key_states(dev, enc):
    """one block of 290 items whose tuples realise every combination of states of four keys -- two byte-string keys (T, F, U,
    NULL), an integer comparison and a set key (T, F, NULL) --, every valid table of four keys, with records and COUNT_ONLY"""
    blk, states = tk.state_block()
    atts, keys, B = tk.STATE_ATTS, tk.STATE_KEYS, tk.STATE_B
    status, n, items = sr.br._items(blk)
    assert (status, n) == (tr.OK, 290) and not any(bad for _, bad, _, _ in items)
    tables = tr.monotone_tables(4)
    assert len(tables) == 167
    comps = [enc(METHOD_LZ4, blk)]
    n_und = 0
    with scan_calls.Device(dev, comps, atts, keys) as d:
        dst, rec, tab, tot = d.alloc(B + 64), d.alloc(8 * 290 + 64), d.alloc(32 + 64), d.alloc(16)
        for i, W in enumerate(tables):
            matches, und = tk.state_expect(states, W)                       # by construction
            n_und += bool(und)
            hit = set(matches)
            recs = np.array([(pos, 0, ln) if pos in hit else (pos, tr.UNDECIDED, 0) for pos, _, off, ln in items if pos in hit or pos in und],
                            cc.FILTER_REC)
            parts = []
            for pos, _, off, ln in items:
                if pos in hit:
                    t = np.zeros(tc.maxalign(ln), np.uint8)
                    t[:ln] = blk[off:off + ln]
                    parts.append(t)
            packed = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
            want = (np.array([(0, 290, len(matches), len(und), 0, 0)], cc.FILTER_BLOCK), recs, packed, (packed.size, recs.size))
            if i % 40 == 0:                                                  # the construction and the reference say the same
                ref = tr.filter_call([blk], atts, keys, 0, W)
                assert np.array_equal(ref[0], want[0]) and np.array_equal(ref[1], want[1]) and np.array_equal(ref[2], want[2])
            for flags in (0, tr.COUNT_ONLY):
                for b in (dst, rec, tab):
                    b.memset(SENTINEL)
                tot.memset(0xEE)
                dev.filter_batch(METHOD_LZ4, d.src, d.off, d.sz, B, 1, d.natts, d.atts, d.nkeys, d.keys, flags, dst, B, rec, 290, tab, tot,
                                 truth=W)
                dev.sync()
                got_tab, got_rec, got_dst = tab.download(), rec.download(), dst.download()
                total = tuple(int(v) for v in tot.download(dtype=np.uint64)[:2])
                assert (got_tab[32:] == SENTINEL).all(), (W, "a byte beyond the block table was written")
                got = (got_tab[:32].view(cc.FILTER_BLOCK).copy(), got_rec[:8 * 290].view(cc.FILTER_REC).copy(), got_dst, total)
                if flags:
                    empty = (want[0], np.zeros(0, cc.FILTER_REC), np.zeros(0, np.uint8), (0, 0))
                    same_filter(got, empty, (bin(W), "count only"))
                    assert (got_rec == SENTINEL).all()
                else:
                    same_filter(got, want, bin(W))
                    assert (got_rec[8 * recs.size:] == SENTINEL).all()
        d.keys_untouched()
    assert n_und > 100                                                       # most tables leave some tuple undecided


# ---- four calls, three forms ----
def test_crafted_blocks_filter(dev, enc):
    """every hand-made block in batches of 1, 4, 5 and 9 blocks, both methods: device buffers, host buffers, COUNT_ONLY in both"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(tk.cases()):
        blocks = batch(idx, blk, B, atts)
        want = tr.filter_call(blocks, atts, keys, 0, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name       # block 0's, as written by hand
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        cwant = tr.filter_call(blocks, atts, keys, tr.COUNT_ONLY, W)
        for method in METHODS:
            comps = [enc(method, b) for b in blocks]
            got = tcall.filter_batch(dev, method, comps, B, atts, keys, 0, W)
            same_filter(got, want, (name, method))
            first = got[1][:len(matches) + len(bad)]
            assert {int(r["pos"]): int(r["status"]) for r in first if r["status"]} == bad, name
            same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, 0, W), want, (name, method, "host buffers"))
            same_filter(tcall.filter_batch(dev, method, comps, B, atts, keys, tr.COUNT_ONLY, W), cwant, (name, method, "count only"))
            same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, tr.COUNT_ONLY, W), cwant, (name, method, "count only, host"))


def test_crafted_blocks_agg_group_and_project(dev, enc):
    """the same blocks through the aggregate and the projection (1, 4, 5, 9 blocks) and the grouped scan (1, 2, 3 blocks), device
    buffers and host buffers, the methods alternating"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(tk.cases()):
        method = METHODS[idx % 2]
        cols, by, pcols = columns(atts)
        blocks = batch(idx, blk, B, atts)
        comps = [enc(method, b) for b in blocks]
        want = tr.agg_call(blocks, atts, keys, cols, W)
        assert want[0]["n_match"][0] == len(matches), name
        same_agg(tcall.agg_batch(dev, method, comps, B, atts, keys, cols, W), want, name)
        same_agg(tcall.agg_host(dev, method, comps, B, atts, keys, cols, W), want, (name, "host"))
        want = tr.project_call(blocks, atts, keys, pcols, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name
        same_project(tcall.project_batch(dev, method, comps, B, atts, keys, pcols, W), want, name)
        same_project(tcall.project_host(dev, method, comps, B, atts, keys, pcols, W), want, (name, "host"))
        blocks = batch(idx, blk, B, atts, (1, 2, 3))
        comps = [enc(method, b) for b in blocks]
        want = tr.group_call(blocks, atts, keys, by, cols[1:], W)
        same_group(tcall.group_batch(dev, method, comps, B, atts, keys, by, cols[1:], W), want, name)
        same_group(tcall.group_host(dev, method, comps, B, atts, keys, by, cols[1:], W), want, (name, "host"))


def _raw(result):
    return [np.asarray(x).tobytes() if isinstance(x, np.ndarray) else x for x in result]


def test_the_and_table_is_the_call_without_the_flag(dev, enc):
    """byte for byte in all four calls and both buffer forms, on keys that run <false> without the flag (integers alone) and on
    keys that run <true> either way (a byte-string key with undecided values, a set key)"""
    blk = tc.build_block(tk.B, tk.mix() + [tk.T(i, b"de" if i % 3 else tc.Toast(), i % 4 + 3, i % 3, i % 5 + 1) for i in range(7, 40)])
    blocks = [blk, other_block(tk.B, tk.ATTS), blk]
    cols, by, pcols = columns(tk.ATTS)
    for keys in ([(5, tr.INT4, tr.GE, 3), (3, tr.INT8, tr.LE, 5)],
                 [(2, tr.BYTES, tr.EQ, b"de"), (5, tr.INT4, tr.EQ, 3), (3, tr.INT8, tr.IN, [5, 6])],
                 [(4, 0, tr.NOTNULL, 0)]):
        W = tr.and_table(len(keys))
        want = sr.filter_call(blocks, tk.ATTS, keys)
        assert want[0]["n_match"].sum() > 0
        for method in METHODS:
            comps = [enc(method, b) for b in blocks]
            for flags in (0, tr.COUNT_ONLY):
                a, b = tcall.filter_batch(dev, method, comps, tk.B, tk.ATTS, keys, flags, W), tcall.filter_batch(dev, method, comps, tk.B, tk.ATTS, keys, flags)
                assert _raw(a) == _raw(b)
                a, b = tcall.filter_host(dev, method, comps, tk.B, tk.ATTS, keys, flags, W), tcall.filter_host(dev, method, comps, tk.B, tk.ATTS, keys, flags)
                assert _raw(a) == _raw(b)
            same_filter(tcall.filter_batch(dev, method, comps, tk.B, tk.ATTS, keys, 0, W), want, keys)
            for call, args in ((tcall.agg_batch, (cols,)), (tcall.agg_host, (cols,)), (tcall.group_batch, (by, cols[1:])),
                               (tcall.group_host, (by, cols[1:])), (tcall.project_batch, (pcols,)), (tcall.project_host, (pcols,))):
                a, b = call(dev, method, comps, tk.B, tk.ATTS, keys, *args, W), call(dev, method, comps, tk.B, tk.ATTS, keys, *args)
                assert _raw(a) == _raw(b), (call.__name__, keys)


def test_multi_handles(dev, enc):
    """cryo_multi_*_blocks with one handle and with two on one device (two devices where the machine has them): a handful of
    tables -- OR of two, both nested shapes, OR over an undecided value, constant true, the AND table"""
    picked = {"OR of two integer keys", "(A AND B) OR C", "A AND (B OR C)", "undecided OR a key: a true key decides",
              "constant true: keys that nothing passes", "undecided AND a key: a false key decides"}
    cases = [c for c in tk.cases() if c[0] in picked]
    assert len(cases) == len(picked)
    for devices in [(0,), (0, 0)] + ([(0, 1)] if cc.device_count() > 1 else []):
        G = len(devices)
        for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(cases):
            method = METHODS[idx % 2]
            blocks = batch(2, blk, B, atts)                                  # five blocks
            comps = [enc(method, b) for b in blocks]
            n = len(comps)
            cols, by, pcols = columns(atts)
            rb = sr.pr.row_layout(atts, pcols)[1]
            rows = np.full((290 * n, rb), SENTINEL, np.uint8)
            rec = np.full(8 * 290 * n, SENTINEL, np.uint8).view(cc.PROJECT_REC)

            def five(L, h, chk):                                             # one handle serves the case's five calls
                return (cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W),
                                              np.full(n * B, SENTINEL, np.uint8), np.full(n * 290, REC_SENTINEL, cc.FILTER_REC)),
                        cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, tr.COUNT_ONLY, W))[0],
                        cc.agg_blocks_call(L.cryo_multi_agg_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W), cc.agg_desc(cols)),
                        cc.group_blocks_call(L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W),
                                             cc.group_desc(by), cc.agg_desc(cols[1:])),
                        cc.project_blocks_call(L.cryo_multi_project_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, 0, W),
                                               cc.project_desc(pcols), rb, rows, rec))
            (table, recs, dst, total), ctab, agg, grp, (ptab, prec, prows, (tw, trec)) = multi_call(devices, five)
            if G == 1:
                same_filter((table, recs, dst, total), tr.filter_call(blocks, atts, keys, 0, W), (name, devices))
            else:
                etable, regions, etotal = tr.multi_filter_call(blocks, atts, keys, G, B, 0, W)
                same_fields(table, etable, (name, devices))
                assert total == etotal
                wb, wr = np.zeros(dst.size, bool), np.zeros(recs.size, bool)
                for b0, packed, r0, rs in regions:
                    assert np.array_equal(dst[b0:b0 + packed.size], packed) and np.array_equal(recs[r0:r0 + rs.size], rs)
                    wb[b0:b0 + packed.size] = True
                    wr[r0:r0 + rs.size] = True
                assert (dst[~wb] == SENTINEL).all() and (recs[~wr].view(np.uint8) == SENTINEL).all()
            same_fields(ctab, tr.filter_call(blocks, atts, keys, tr.COUNT_ONLY, W)[0], (name, devices, "count only"))
            same_agg(agg, tr.agg_call(blocks, atts, keys, cols, W), (name, devices))
            same_group(grp, tr.group_call(blocks, atts, keys, by, cols[1:], W), (name, devices))
            if G == 1:
                same_project((ptab, prec[:trec], prows[:tw], (tw, trec)), tr.project_call(blocks, atts, keys, pcols, W), (name, devices))
            else:
                etable, regions, etotal = tr.multi_project_call(blocks, atts, keys, pcols, G, W)
                same_fields(ptab, etable, (name, devices))
                assert (tw, trec) == etotal
                ww, wr = np.zeros(len(prows), bool), np.zeros(prec.size, bool)
                for first, erows, erecs in regions:
                    assert np.array_equal(prows[first:first + len(erows)], erows) and np.array_equal(prec[first:first + erecs.size], erecs)
                    ww[first:first + len(erows)] = True
                    wr[first:first + erecs.size] = True
                assert (prows[~ww] == SENTINEL).all() and (prec[~wr].view(np.uint8) == SENTINEL).all()


# ---- bad blocks ----
def test_rejected_streams_between_good_neighbours(dev, enc):
    """a stream that does not decode and a block with a bad header between good ones: STREAM and HEADER whatever the table says,
    and the blocks behind them placed as if they held nothing"""
    name, B, atts, good, keys, W, matches, bad = next(c for c in tk.cases() if c[0] == "undecided OR a key: a true key decides")
    header = good.copy()
    header[0:4] = np.frombuffer((12).to_bytes(4, "little"), np.uint8)         # lower = 12: not 8 + 8 n
    blocks = [good, None, header, good, None, good]
    cols, by, pcols = columns(atts)
    for W in (W, 0b1111):                                                   # the case's OR, and constant true
        want = tr.filter_call(blocks, atts, keys, 0, W)
        assert want[0]["status"].tolist() == [0, tr.STREAM, tr.HEADER, 0, tr.STREAM, 0]
        for method in METHODS:
            comps = [enc(method, good if b is None else b) for b in blocks]
            comps[1] = comps[1][:len(comps[1]) - 7]
            comps[4] = comps[4][:len(comps[4]) // 2]
            assert [sr.decode(enc.oracle, method, c, B) is None for c in comps] == [b is None for b in blocks]
            same_filter(tcall.filter_batch(dev, method, comps, B, atts, keys, 0, W), want, method)
            same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, 0, W), want, (method, "host"))
            same_filter(tcall.filter_batch(dev, method, comps, B, atts, keys, tr.COUNT_ONLY, W), tr.filter_call(blocks, atts, keys, tr.COUNT_ONLY, W), method)
            same_agg(tcall.agg_batch(dev, method, comps, B, atts, keys, cols, W), tr.agg_call(blocks, atts, keys, cols, W), method)
            same_group(tcall.group_host(dev, method, comps, B, atts, keys, by, cols[1:], W), tr.group_call(blocks, atts, keys, by, cols[1:], W), method)
            same_project(tcall.project_batch(dev, method, comps, B, atts, keys, pcols, W), tr.project_call(blocks, atts, keys, pcols, W), method)


# ---- a seeded property test ----
def test_random_keys_and_tables_on_wide_random_tuples(dev, enc):
    """the wide random tuples of tests/walk_gen.py, 1 .. 4 random keys of every kind, random valid tables, a fixed seed: the four
    calls against the reference.  That enough descriptors meet an undecided tuple and a tuple an OR decided is asserted here on
    the reference's side, so the test cannot pass on descriptors that say nothing"""
    descs = tk.property_descriptors()
    undecided, or_decided, matches, sizes = tk.property_coverage(descs)
    assert undecided >= len(descs) // 4 and or_decided >= len(descs) // 2 and matches > 500 and sizes == {1, 2, 3, 4}
    for turn, (name, keys, W) in enumerate(descs):
        case = wg.case(name)
        atts, B, plan = case.call_atts, case.B, case.plan
        blocks = [b.data for b in case.blocks]
        method = METHODS[turn % 2]
        comps = [enc(method, b) for b in blocks]
        what = (name, keys, bin(W))
        want = tr.filter_call(blocks, atts, keys, 0, W)
        same_filter(tcall.filter_batch(dev, method, comps, B, atts, keys, 0, W), want, what)
        same_filter(tcall.filter_host(dev, method, comps, B, atts, keys, 0, W), want, (what, "host"))
        same_agg((tcall.agg_host if turn % 3 == 0 else tcall.agg_batch)(dev, method, comps, B, atts, keys, plan.agg_cols, W),
                 tr.agg_call(blocks, atts, keys, plan.agg_cols, W), what)
        same_group((tcall.group_host if turn % 3 == 1 else tcall.group_batch)(dev, method, comps, B, atts, keys, plan.by, plan.group_cols, W),
                   tr.group_call(blocks, atts, keys, plan.by, plan.group_cols, W), what)
        same_project((tcall.project_host if turn % 3 == 2 else tcall.project_batch)(dev, method, comps, B, atts, keys, plan.project_cols, W),
                     tr.project_call(blocks, atts, keys, plan.project_cols, W), what)


# ---- arguments ----
def test_descriptor_rules(dev, enc):
    """the rules of the flag and the table -- and the older refusals beside them -- on host arrays and, through the
    device-resident call, on device arrays; the aggregate, the grouping and the projection take the flag and refuse COUNT_ONLY"""
    B = tk.B
    blk = tc.build_block(B, [tk.T(1, b"p", 2, 3, 4)])
    comp = np.ascontiguousarray(enc(METHOD_LZ4, blk))
    L = dev.L
    src, szs = (C.c_void_p * 1)(comp.ctypes.data), (C.c_uint32 * 1)(comp.nbytes)
    dst, rec, table, tot = np.zeros(B, np.uint8), np.zeros(290, cc.FILTER_REC), np.zeros(1, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
    names = set()
    for name, atts, keys, flags, rsv, ok in tk.descriptors():
        assert tr.desc_ok(atts, keys, flags, rsv) == ok, name
        names.add(name)
        f, a, k = cc.filter_desc(atts, keys)
        f.flags, f.rsv = flags, rsv
        rc = L.cryo_codec_filter_blocks(dev.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), dst.ctypes.data, dst.nbytes, rec.ctypes.data,
                                        rec.size, table.ctypes.data, tot)
        assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
        if len(keys) > 4:
            keys = keys[:4]                                                  # Device stages what fits; nkeys below says five
        with scan_calls.Device(dev, [comp], atts, keys) as d:
            d_dst, d_rec, d_tab, d_tot = d.alloc(B), d.alloc(8 * 290), d.alloc(32), d.alloc(16)
            nkeys = 5 if "five keys" in name else len(keys)
            g = cc.CryoFilter(len(atts), nkeys, flags, rsv, d.atts.ptr, d.keys.ptr if nkeys else None)
            rc = L.cryo_codec_filter_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(g), d_dst.ptr, B, d_rec.ptr,
                                           290, d_tab.ptr, d_tot.ptr)
            dev.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    assert {"no key", "table 0", "a bit beyond 2^nkeys", "XOR", "NOR", "A AND NOT B", "rsv 1 without the flag", "flags 2"} <= names
    comps, atts = [comp], tk.ATTS
    keys = [(5, tr.INT4, tr.GE, 1), (3, tr.INT8, tr.LT, 9)]
    # the aggregate, the grouping and the projection take the flag ...
    assert tcall.agg_batch(dev, METHOD_LZ4, comps, B, atts, keys, [(1, tr.INT4)], 0b1110)[0]["n_match"][0] == 1
    assert tcall.agg_host(dev, METHOD_LZ4, comps, B, atts, keys, [(1, tr.INT4)], 0b1110)[0]["n_match"][0] == 1
    # ... refuse a bad table as the filter does, and refuse COUNT_ONLY with the flag as without it
    for truth in (0b0110, 0, 0b10000):
        for call in (lambda: tcall.agg_batch(dev, METHOD_LZ4, comps, B, atts, keys, [(1, tr.INT4)], truth),
                     lambda: tcall.group_batch(dev, METHOD_LZ4, comps, B, atts, keys, [(1, tr.INT4)], [], truth),
                     lambda: tcall.project_batch(dev, METHOD_LZ4, comps, B, atts, keys, [1], truth),
                     lambda: tcall.agg_host(dev, METHOD_LZ4, comps, B, atts, keys, [(1, tr.INT4)], truth),
                     lambda: tcall.group_host(dev, METHOD_LZ4, comps, B, atts, keys, [(1, tr.INT4)], [], truth),
                     lambda: tcall.project_host(dev, METHOD_LZ4, comps, B, atts, keys, [1], truth)):
            with pytest.raises(CryoError) as e:
                call()
            assert e.value.code == cc.E_ARG
    for flags in (tr.TRUTH | tr.COUNT_ONLY, tr.COUNT_ONLY):
        f, a, k = cc.filter_desc(atts, keys, flags & tr.COUNT_ONLY, 0b1110 if flags & tr.TRUTH else None)
        assert f.flags == flags
        with pytest.raises(CryoError) as e:
            dev.agg_blocks(METHOD_LZ4, comps, B, (f, a, k), cc.agg_desc([(1, tr.INT4)]))
        assert e.value.code == cc.E_ARG
        with pytest.raises(CryoError) as e:
            dev.project_blocks(METHOD_LZ4, comps, B, (f, a, k), cc.project_desc([1]), 8)
        assert e.value.code == cc.E_ARG
        with scan_calls.Device(dev, comps, atts, keys) as d:
            cols, rows, cells = d.put(cc.agg_desc([(1, tr.INT4)])[1]), d.alloc(16), d.alloc(40)
            g = cc.CryoFilter(len(atts), 2, flags, f.rsv, d.atts.ptr, d.keys.ptr)
            ag = cc.CryoAgg(1, 0, cols.ptr)
            rc = L.cryo_codec_agg_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(g), C.byref(ag), rows.ptr, cells.ptr)
            dev.sync()
            assert rc == cc.E_ARG, flags
