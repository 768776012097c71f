"""GPU: the four scan calls (filter, aggregate, group, project) and the fetch on blocks and tuples above 1 MiB -- the cases of
tests/large_scan_cases.py, whose expectations tests/test_large_scan_cpu.py pins by hand.

Every comparison is exact and made against the references applied to the blocks the ORACLE encoded (its decode of every stream
is compared with the block first), for both methods: a block of 256 and of 257 item ids on one tuple of 16 MiB, whose matches sum
to 2^32 and to 2^32 + 2^24 bytes (OVERLAP; a sum kept in 32 bits would say "fits"), that tuple once, a block of tuples with
varlenas of up to 2.5 MiB in front of their key columns, and the generator's block at 1 MiB + 8 and 4 MiB + 24; alone and between
neighbours, through the device-resident and the host-buffer calls, in chunks of one block, over 260 blocks whose running totals
pass 2^32, and through two handles.  Outputs are filled with a sentinel before every call."""
import time

import numpy as np
import pytest

import fetch_ref
import filter_ref
import large_scan_cases as ls
import layout_ref
import scan_calls
import truth_calls as tcall
from large_scan_cases import TWO24
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc
from scan_calls import REC_SENTINEL, SENTINEL, same_agg, same_filter, same_group, same_project

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
_streams = {}


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


def stream(oracle, method, c):
    """the oracle's stream of a case's block, made once; its decode by the oracle is the block"""
    key = (method, c.name)
    if key not in _streams:
        s = oracle.lz4_compress(c.block, 1) if method == METHOD_LZ4 else oracle.zstd_compress(c.block, 1)
        assert np.array_equal(layout_ref.decode(oracle, method, s, c.B), c.block), (c.name, "the oracle's own round trip")
        _streams[key] = s
    return _streams[key]


def batches(oracle, c):
    nb = ls.neighbour(oracle, c)
    return [[c], [c, nb, c]]


def run_device(dev, method, comps, c, keyset, call):
    keys, W = c.keysets[keyset]
    if call in ("filter", "count"):
        return tcall.filter_batch(dev, method, comps, c.B, c.atts, keys, fl_flags(call), W)
    if call == "agg":
        return tcall.agg_batch(dev, method, comps, c.B, c.atts, keys, c.agg_cols, W)
    if call == "group":
        return tcall.group_batch(dev, method, comps, c.B, c.atts, keys, c.group_by, c.agg_cols, W)
    return tcall.project_batch(dev, method, comps, c.B, c.atts, keys, c.project_cols, W)


def run_host(dev, method, comps, c, keyset, call):
    keys, W = c.keysets[keyset]
    if call in ("filter", "count"):
        return tcall.filter_host(dev, method, comps, c.B, c.atts, keys, fl_flags(call), W)
    if call == "agg":
        return tcall.agg_host(dev, method, comps, c.B, c.atts, keys, c.agg_cols, W)
    if call == "group":
        return tcall.group_host(dev, method, comps, c.B, c.atts, keys, c.group_by, c.agg_cols, W)
    return tcall.project_host(dev, method, comps, c.B, c.atts, keys, c.project_cols, W)


def fl_flags(call):
    return filter_ref.COUNT_ONLY if call == "count" else 0


SAME = {"filter": same_filter, "count": same_filter, "agg": same_agg, "group": same_group, "project": same_project}
CALLS = ["filter", "count", "agg", "group", "project"]


# ---- all four scans, device-resident ----
@pytest.mark.parametrize("name", ls.NAMES)
def test_all_four_scans(dev, oracle, name):
    """every case alone and between two blocks (case, neighbour, case), both methods, every key set the case has: the filter, the
    filter under COUNT_ONLY, the aggregate of k, x and g, the grouping by g and the projection of k, g, x and id.  The blocks of
    256 and 257 aliases go through the filter under a set key and under a float key as well: the kernel's other two
    instantiations.  Behind an OVERLAP block the neighbour's row starts at 0 and its bytes are the call's first"""
    c = ls.case(oracle, name)
    for method in METHODS:
        for turn, keyset in enumerate(ls.CASE_KEYSETS[name]):
            for cases in batches(oracle, c)[0 if turn == 0 else 1:]:      # one block: with the case's first key set
                comps = [stream(oracle, method, x) for x in cases]
                for call in CALLS:
                    want = ls.call_of(cases, keyset, call)
                    SAME[call](run_device(dev, method, comps, c, keyset, call), want, (name, method, keyset, len(cases), call))
        for keyset in ls.FILTER_ONLY.get(name, []):                       # the kernels of set keys and of float keys
            cases = batches(oracle, c)[1]
            comps = [stream(oracle, method, x) for x in cases]
            for call in ("filter", "count"):
                SAME[call](run_device(dev, method, comps, c, keyset, call), ls.call_of(cases, keyset, call), (name, method, keyset, call))
    if name in ("aliased256", "aliased257"):
        n = int(name[7:])
        table = ls.call_of(batches(oracle, c)[1], "int", "filter")[0]
        assert table["status"].tolist() == [7, 0, 7] and table["n_match"].tolist() == [0, 2, 0] and table["off"][1] == 0
        assert ls.call_of([c], "int", "agg")[0]["n_match"][0] == n == ls.call_of([c], "int", "project")[3][0]


# ---- the host-buffer forms ----
@pytest.mark.parametrize("name", ["aliased1", "aliased257", "mixed"])
def test_host_buffer_forms(dev, oracle, name):
    """cryo_codec_filter_blocks / _agg_blocks / _group_blocks / _project_blocks on (case, neighbour, case): bytes, records and the
    transfer counters; the match of 16 MiB comes back through the staging row whole"""
    c = ls.case(oracle, name)
    cases = batches(oracle, c)[1]
    n = len(cases)
    keysets = ls.CASE_KEYSETS[name]
    for method in METHODS:
        comps = [stream(oracle, method, x) for x in cases]
        for keyset in sorted({keysets[0], keysets[-1]}):
            d2h = {}
            for call in CALLS:
                want = ls.call_of(cases, keyset, call)
                before = dev.transfer_counters()["d2h_bytes"]
                got = run_host(dev, method, comps, c, keyset, call)
                d2h[call] = dev.transfer_counters()["d2h_bytes"] - before
                SAME[call](got, want, (name, method, keyset, call, "host buffers"))
            total = ls.call_of(cases, keyset, "filter")[3]
            assert d2h["filter"] == 32 * n + 8 * total[1] + total[0] and d2h["count"] == 32 * n, (name, method, keyset, d2h)
            nc = len(c.agg_cols)
            groups = ls.call_of(cases, keyset, "group")[3]
            rows, recs = ls.call_of(cases, keyset, "project")[3]
            assert d2h["agg"] == (16 + 40 * nc) * n and d2h["group"] == 32 * n + (24 + 40 * nc) * groups, (name, method, keyset, d2h)
            assert d2h["project"] == 32 * n + 8 * recs + 32 * rows, (name, method, keyset, d2h)
    if name == "aliased1":
        assert ls.call_of(cases, "int", "filter")[3][0] == 2 * TWO24 + ls.expected(cases[1], "int", "filter")[3][0]


# ---- fetch and check ----
@pytest.mark.parametrize("method", METHODS)
def test_fetch_and_check(dev, oracle, method):
    """the fetch of every position of the aliased blocks (OVERLAP for each request, nothing packed) and of the first, a middle
    and the last position of mixed(); the stored-block check on every block of this file"""
    for n in (256, 257):
        c = ls.case(oracle, "aliased%d" % n)
        reqs = [list(range(1, n + 1))]
        erec, epacked, etotal = fetch_ref.fetch_call([c.block], reqs)
        assert etotal == 0 and (erec["status"] == fetch_ref.OVERLAP).all()
        rec, dst, total = dev.fetch_blocks(method, [stream(oracle, method, c)], c.B, reqs, dst=np.full(c.B, SENTINEL, np.uint8))
        assert total == 0 and np.array_equal(rec, erec) and (dst == SENTINEL).all(), n
    c, one = ls.case(oracle, "mixed"), ls.case(oracle, "aliased1")
    for x, reqs in ((c, [[1, 8, 15]]), (one, [[1]])):
        erec, epacked, etotal = fetch_ref.fetch_call([x.block], reqs)
        rec, dst, total = dev.fetch_blocks(method, [stream(oracle, method, x)], x.B, reqs, dst=np.full(x.B, SENTINEL, np.uint8))
        assert total == etotal and np.array_equal(rec, erec) and np.array_equal(dst[:total], epacked) and (dst[total:] == SENTINEL).all()
    assert [int(s) for s in fetch_ref.fetch_call([c.block], [[1, 8, 15]])[0]["status"]] == [0, 0, fetch_ref.ITEM]
    by_size = {}
    for name in ls.NAMES:
        x = ls.case(oracle, name)
        by_size.setdefault(x.B, []).extend([x, ls.neighbour(oracle, x)])
    for B, cases in by_size.items():
        got = dev.check_blocks(method, [stream(oracle, method, x) for x in cases], B)
        assert [tuple(int(v) for v in r) for r in got] == [layout_ref.check_block(x.block) for x in cases], B


# ---- chunks of one block ----
@pytest.mark.parametrize("name,budget", [("aliased1", 8 << 20), ("aliased257", 8 << 20), ("mixed", 2 << 20)])
def test_chunks_below_one_block(dev, oracle, name, budget):
    """CRYO_OPT_WORKSPACE_MAX_BYTES below what one block needs: every block is a chunk of its own, the totals run on in device
    memory, and the device-resident filter and projection and the host-buffer filter return what they return in one chunk"""
    c = ls.case(oracle, name)
    cases = batches(oracle, c)[1]
    keyset = ls.CASE_KEYSETS[name][-1]
    for method in METHODS:
        comps = [stream(oracle, method, x) for x in cases]
        whole = {}
        for budget_now in (0, budget):
            dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget_now)
            for call, run in (("filter", run_device), ("project", run_device), ("host filter", run_host)):
                got = run(dev, method, comps, c, keyset, call.split()[-1])
                SAME[call.split()[-1]](got, ls.call_of(cases, keyset, call.split()[-1]), (name, method, call, budget_now))
                if budget_now == 0:
                    whole[call] = got
                else:
                    for a, b in zip(got[:3], whole[call][:3]):
                        assert np.array_equal(a, b), (name, method, call, "differs from the default budget's")
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- running totals above 2^32 ----
def test_running_totals_pass_2_32(dev, oracle):
    """one device-resident filter call over 260 copies of the aliased(1) stream (about 4.1 GiB decoded): block i's tuple starts at
    i * 2^24, so the byte total passes 2^32 in block 256.  The destination takes two tuples; the records and the table are whole.
    The expectation comes from the one-block reference"""
    c = ls.case(oracle, "aliased1")
    n = 260
    keys, _ = c.keysets["int"]
    etable, erecs, epacked, etotal = ls.expected(c, "int", "filter")
    assert etotal == (TWO24, 1) and erecs.size == 1
    comps = [stream(oracle, METHOD_LZ4, c)] * n
    cap = 2 * TWO24 + 64
    t0 = time.time()
    with scan_calls.Device(dev, comps, c.atts, keys) as d:
        dst, rec = d.alloc(cap, SENTINEL), d.alloc(8 * n + 64, SENTINEL)
        tab, tot = d.alloc(32 * n, 0xEE), d.alloc(16, 0xEE)
        dev.sync()
        t1 = time.time()
        dev.filter_batch(METHOD_LZ4, d.src, d.off, d.sz, c.B, n, d.natts, d.atts, d.nkeys, d.keys, 0, dst, cap, rec, n, tab, tot)
        dev.sync()
        t2 = time.time()
        d.keys_untouched()
        total = tuple(int(v) for v in tot.download(dtype=np.uint64))
        table = tab.download(dtype=np.uint8).view(cc.FILTER_BLOCK).copy()
        recs = rec.download(dtype=np.uint8).view(cc.FILTER_REC).copy()
        out = dst.download()
    print("filter_batch over %d blocks of %d bytes: %.2f s the call, %.2f s with upload and download" % (n, c.B, t2 - t1, time.time() - t0))
    assert total == (n * TWO24, n) and total[0] > 1 << 32
    i = np.arange(n, dtype=np.uint64)
    assert (table["off"] == i * np.uint64(TWO24)).all() and (table["rec_first"] == i).all()
    for f in ("status", "n_items", "n_match", "n_bad"):
        assert (table[f] == etable[f][0]).all(), f
    assert (recs[:n] == erecs[0]).all() and (recs[n:].view(np.uint8) == SENTINEL).all()
    assert np.array_equal(out[:TWO24], epacked) and np.array_equal(out[TWO24:2 * TWO24], epacked), "the first two tuples"
    assert (out[2 * TWO24:] == SENTINEL).all(), "a byte of a tuple that ends beyond dst_cap was written"


# ---- two handles ----
@pytest.mark.parametrize("method", METHODS)
def test_multi_filter_blocks(dev, oracle, method):
    """cryo_multi_filter_blocks with two handles on GPU 0 over (aliased(1), small, mixed in a block of the same size): handle 0
    places blocks 0 and 2 in its region, handle 1 block 1 in the next"""
    one = ls.case(oracle, "aliased1")
    B = one.B
    cases = [one, ls.neighbour(oracle, one), ls.case(oracle, "mixed@%d" % B)]
    keys, _ = one.keysets["int"]
    blocks = [x.block for x in cases]
    comps = [stream(oracle, method, x) for x in cases]
    n = len(cases)
    etable, regions, etotal = filter_ref.multi_call(blocks, ls.ATTS, keys, 2, B)
    assert etable["n_match"].tolist() == [1, 2, ls.MIXED_VERDICTS["int"].count("M")] and etable["n_bad"][2] == 3
    table, recs, dst, total = scan_calls.multi_call(
        (0, 0), lambda L, h, chk: cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(ls.ATTS, keys),
                                                        np.full(n * B, SENTINEL, np.uint8), np.full(n * 290, REC_SENTINEL, cc.FILTER_REC)))
    scan_calls.same_fields(table, etable, "two handles")
    assert total == etotal
    wb, wr = np.zeros(dst.size, bool), np.zeros(recs.size, bool)
    for b0, packed, r0, rs in regions:
        assert np.array_equal(dst[b0:b0 + packed.size], packed) and np.array_equal(recs[r0:r0 + rs.size], rs)
        wb[b0:b0 + packed.size] = True
        wr[r0:r0 + rs.size] = True
    assert (dst[~wb] == SENTINEL).all() and (recs[~wr].view(np.uint8) == SENTINEL).all()
