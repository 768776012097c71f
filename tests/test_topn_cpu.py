"""CPU tests of the ordered scan: the reference (tests/topn_ref.py) against the hand-made expectations of tests/topn_cases.py, its
descriptor rules, the three merges -- host/topn.c's, codec.topn_merge and the reference's -- against a plain sort of all rows,
cryo_topn_scan (host/topn.c) walking a mini-AM relation through the test build with a codec double (tests/topn_double.py), and
tests/topn_merge_check.c, a program of its own that runs the C merge under the host sanitizers."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fetch_walk
import filter_ref as fr
import topn_cases as tcs
import topn_ref as tr
import tuple_craft as tc
from pg_cryogen_amd import codec as cc, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MERGES = (tr.merge, cc.topn_merge, host.topn_merge)


@pytest.mark.parametrize("case", tcs.cases(), ids=lambda c: c[0])
def test_reference_against_hand_made_orders(case):
    name, B, atts, block, keys, by, cols, order, keys_at = case
    for limit in (1, 2, len(order), 290, 1000):
        table, recs, rows, total = tr.topn_call([block], atts, keys, by, limit, cols)
        kept = order[:limit]
        assert total == len(kept) and int(table["n_rows"][0]) == len(kept) and int(table["n_match"][0]) == len(order)
        assert recs["pos"].tolist() == kept, (name, limit)
        for r, w in zip(recs, rows):
            p = int(r["pos"])
            if p in keys_at:
                assert (int(r["key"][0]), int(r["key"][1]), int(r["key_nulls"])) == keys_at[p], (name, p)


def test_reference_rows_are_the_projection_rows():
    import project_ref as pr
    for name, B, atts, block, keys, by, cols, order, _ in tcs.cases():
        if any(k[1] >= 8 or k[2] >= 9 for k in keys):
            continue                                                     # project_ref knows neither float nor set keys
        table, recs, rows, _ = tr.topn_call([block], atts, keys, by, 1000, cols)
        pt, prec, prows, _ = pr.project_call([block], atts, keys, cols)
        by_pos = {int(r["pos"]): (int(r["nulls"]), bytes(w)) for r, w in zip(prec[prec["status"] == 0], prows)}
        assert [(int(r["nulls"]), bytes(w)) for r, w in zip(recs, rows)] == [by_pos[int(r["pos"])] for r in recs], name


def test_reference_truth_table_undecided_and_bad_items():
    keys, truth, order = tcs.truth_case()
    by = [(tcs.K, fr.INT8, tcs.DESC)]
    t, recs, _, _ = tr.topn_call([tcs.named_block()], tcs.ATTS, keys, by, 10, tcs.COLS, truth)
    assert recs["pos"].tolist() == order
    bkey = [(tcs.NAME, tr.br.BYTES, tr.fl.GE, b"c")]
    t, recs, _, _ = tr.topn_call([tcs.named_block(True)], tcs.ATTS, bkey, by, 10, tcs.COLS)
    assert recs["pos"].tolist() == [6, 4, 5] and (int(t["n_match"][0]), int(t["n_bad"][0])) == (3, 1)
    t, recs, _, _ = tr.topn_call([tcs.bad_items_block()], tcs.ATTS, [], [(tcs.K, fr.INT8, 0)], 3, tcs.COLS)
    assert recs["pos"].tolist() == [5, 3, 1] and (int(t["n_match"][0]), int(t["n_bad"][0]), int(t["n_rows"][0])) == (4, 2, 3)


def test_reference_call_carries_row_first_across_blocks_without_an_answer():
    good = tcs.cases()[1][3]
    by = [(tcs.K, fr.INT8, 0)]
    t, recs, rows, total = tr.topn_call([good, None, tcs.header_block(), good], tcs.ATTS, [], by, 2, tcs.COLS)
    assert t["status"].tolist() == [0, tr.STREAM, tr.HEADER, 0] and t["row_first"].tolist() == [0, 2, 2, 2] and total == 4
    table, regions, end = tr.multi_call([good] * 5, tcs.ATTS, [], by, 2, tcs.COLS, 2)
    assert table["row_first"].tolist() == [0, 6, 2, 8, 4] and [r[0] for r in regions] == [0, 6] and end == 10


@pytest.mark.parametrize("d", tcs.descriptors(), ids=lambda d: d[0])
def test_reference_descriptor_rules(d):
    name, atts, keys, by, limit, cols, patch, ok = d
    assert tcs.ref_ok(tr, atts, keys, by, limit, cols, patch) == ok, name


def test_image_is_the_float_order():
    f8 = tcs.f8
    vals = [float("-inf"), -1e300, -1.5, -5e-324, 0.0, 5e-324, 1.0, 1e300, float("inf")]
    imgs = [tr.image(f8(v), tr.FLOAT8) for v in vals]
    assert imgs == sorted(imgs) and len(set(imgs)) == len(imgs)
    assert tr.image(f8(-0.0), tr.FLOAT8) == tr.image(f8(0.0), tr.FLOAT8) == 0
    assert tr.image(tcs.s64(0xFFF8000000000000), tr.FLOAT8) == tr.image(0x7FF0000000000001, tr.FLOAT8) == tr.INT64_MAX > imgs[-1]
    assert tr.image(1, tr.FLOAT4) == f8(2.0 ** -149) and tr.image(tcs.s32(0xFF800000), tr.FLOAT4) == tr.image(f8(float("-inf")), tr.FLOAT8)
    assert tr.image(-7, tr.INT2) == -7


# ---- the merge ----
def random_blocks(seed, n_blocks, by, per):
    """blocks of up to `per` records whose keys repeat across blocks, each in its own order, with rows that name (block, rank)"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n_blocks):
        m = int(rng.integers(0, per + 1))
        recs = np.zeros(m, tr.REC)
        recs["key"][:, 0] = rng.integers(-3, 4, m)
        if len(by) > 1:
            recs["key"][:, 1] = rng.integers(-2, 3, m)
        nulls = rng.integers(0, 8, m) == 0
        recs["key_nulls"] = nulls
        recs["key"][nulls, 0] = 0
        recs["pos"] = np.arange(1, m + 1)
        order = sorted(range(m), key=lambda r: (tr.sort_key(by, [int(k) for k in recs[r]["key"]], int(recs[r]["key_nulls"])), r))
        recs = recs[order]
        rows = np.zeros((m, 8), np.uint8)
        rows[:, 0], rows[:, 1], rows[:, 2] = b, np.arange(m) & 0xFF, np.arange(m) >> 8
        out.append((recs, rows))
    return out


def plain_sort(by, limit, blocks):
    """every row of every block in one list, sorted by (key tuple, block, rank) and cut"""
    flat = [(tr.sort_key(by, [int(k) for k in r["key"]], int(r["key_nulls"])), b, i) for b, (recs, _) in enumerate(blocks) for i, r in enumerate(recs)]
    return [(b, i) for _, b, i in sorted(flat)[:limit]]


@pytest.mark.parametrize("limit", [1, 290, 291, 1000])
@pytest.mark.parametrize("by", [[(1, 3, 0)], [(1, 3, tcs.DESC | tcs.NULLS_FIRST), (2, 3, tcs.DESC)]], ids=["one", "two"])
def test_merges_against_a_plain_sort(by, limit):
    blocks = random_blocks(5, 9, by, 290)
    visible = [blk for i, blk in enumerate(blocks) if i % 3 != 1]       # blocks skipped as invisible
    want = plain_sort(by, limit, visible)
    assert len(want) == min(limit, sum(len(r) for r, _ in visible))      # limit 1 000 with fewer rows than that comes too
    for merge in MERGES:
        recs, rows = merge(by, limit, visible)
        assert [(int(w[0]), int(w[1]) | int(w[2]) << 8) for w in rows] == [(([i for i in range(9) if i % 3 != 1][b]), r) for b, r in want]
        assert [r.tobytes() for r in recs] == [visible[b][0][r].tobytes() for b, r in want]


def test_merge_ties_go_to_the_block_added_earlier():
    by = [(1, 3, 0)]
    recs = np.zeros(3, tr.REC)
    recs["key"][:, 0] = 5
    recs["pos"] = [1, 2, 3]
    a = (recs, np.full((3, 8), 1, np.uint8))
    b = (recs.copy(), np.full((3, 8), 2, np.uint8))
    for merge in MERGES:
        r, w = merge(by, 4, [b, a])
        assert w[:, 0].tolist() == [2, 2, 2, 1] and r["pos"].tolist() == [1, 2, 3, 1]
        r, w = merge(by, 10, [a])
        assert len(r) == 3                                                # fewer rows than the limit
        r, w = merge(by, 10, [])
        assert len(r) == 0


# ---- the C merge under the host sanitizers: a program of its own ----
HOST = os.path.join(ROOT, "pg_cryogen_amd", "host")
SOURCES = [os.path.join(ROOT, "tests", "topn_merge_check.c")] + [os.path.join(HOST, f) for f in
                                                                 ("topn.c", "walk.c", "staging.c", "storage.c", "scan_iterator.c")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def test_the_c_merge_under_the_sanitizers(tmp_path):
    src = tmp_path / "trivial.c"
    src.write_text("int main(void) { return 0; }\n")
    if subprocess.run(["gcc"] + SANITIZE + [str(src), "-o", str(tmp_path / "trivial")], capture_output=True, timeout=120).returncode != 0:
        pytest.skip("this gcc cannot link a program with -fsanitize=address")
    exe = tmp_path / "topn_merge_check"
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DCRYO_HOST_TEST_HOOKS"] + SANITIZE
                   + ["-I" + HOST, "-I" + os.path.join(ROOT, "include")] + SOURCES + ["-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in r.stderr:
        # the leak check cannot start where the process is traced: the rest of the checks without it
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "topn merge check ok", r.stderr[-4000:]


# ---- the walk, through a codec double ----
B128 = 131072
E_UNSUPPORTED, E_ARG, E_DSTSIZE = -6, -1, -5
ATTS4 = [(4, 4), (-1, 4), (2, 2), (8, 8)]                 # (rowid int4, pad text, g int2, ts int8)
COLS = [4, 1]                                             # widths 8, 4: offsets 0, 8; 16 bytes
KEYS = [(1, fr.INT4, fr.GE, 30), (1, fr.INT4, fr.LT, 250)]
BY = [(3, fr.INT2, tcs.NULLS_FIRST), (4, fr.INT8, tcs.DESC)]


@pytest.fixture()
def HT():
    import topn_double
    L = host.lib()
    dbl = topn_double.OrderingDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_topn_ops(C.byref(dbl.topn_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_topn_set_window(0, 0)
    L.cryo_cache_shutdown()
    L.cryo_host_set_topn_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


def _relation(L, oracle, nblocks=9):
    """nblocks chains of 40 tuples (rowid, "t" x (rowid % 7), g = rowid % 3 or NULL when rowid % 10 == 0, ts = (rowid * 7919) %
    1000, so timestamps repeat across blocks): even ones LZ4, odd ones zstd, xid 500 + k.  Returns (mem, rel, decoded blocks,
    first pages)"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4343, C.byref(rel))
    raws, firsts = [], []
    for k in range(nblocks):
        ids = [40 * k + i for i in range(1, 41)]
        raw = tc.build_block(B128, [tc.form_tuple(ATTS4, [r, b"t" * (r % 7), None if r % 10 == 0 else r % 3, (r * 7919) % 1000]) for r in ids])
        comp = oracle.zstd_compress(raw, 1) if k % 2 else oracle.lz4_compress(raw, 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
        raws.append(raw)
    return mem, rel, raws, firsts


def _want_block(first, xid, raw, limit, keys=KEYS):
    t, recs, rows, _ = tr.topn_call([raw], ATTS4, keys, BY, limit, COLS)
    return ("block", first, xid, (int(t["n_items"][0]), int(t["n_match"][0]), int(t["n_bad"][0])), recs.tobytes(), rows.tobytes())


def _flat(events):
    return [e[:4] + (e[4].tobytes(), e[5].tobytes()) if e[0] == "block" else e for e in events]


def test_topn_scan_walk_through_a_double(HT, oracle):
    L, dbl, errors = HT
    mem, rel, raws, firsts = _relation(L, oracle)
    # behind the nine good chains: a chain that cannot be read, a stream the decoders reject, a block with a bad item, a good chain
    short_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 904, oracle.lz4_compress(raws[0], 1))
    dead_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 906, oracle.lz4_compress(raws[3], 1))
    dented = raws[1].copy()
    dented[8 + 8 * 4 + 4:8 + 8 * 4 + 8] = 0                                 # item 5 (rowid 45): len 0
    dent_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 908, oracle.zstd_compress(dented, 1))
    tail_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 907, oracle.zstd_compress(raws[0], 1))
    page = L.cryo_memrel_page(mem, short_first)
    csize = struct.unpack_from("<I", C.string_at(page, 64), 40)[0]
    C.memmove(page + 40, struct.pack("<I", csize + 100000), 4)
    C.memset(L.cryo_memrel_page(mem, dead_first) + 48, 0xFF, 64)

    limit = 7
    events, t = host.topn_scan(rel, ATTS4, KEYS, BY, limit, COLS)
    want = [_want_block(firsts[k], 500 + k, raws[k], limit) for k in range(9)]
    want += [("report", short_first, fetch_walk.CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED), ("report", dead_first, fr.STREAM, 0)]
    want += [_want_block(dent_first, 908, dented, limit), _want_block(tail_first, 907, raws[0], limit)]
    assert _flat(events) == want                                          # blocks in block order, reports between them
    blocks = [e for e in events if e[0] == "block"]
    assert [e[3] for e in blocks][:2] == [(40, 11, 0), (40, 40, 0)] and blocks[9][3] == (40, 39, 1)       # n_bad > 0 comes with the block
    # rowids 30 .. 249: seven blocks have matches, two have none; every block keeps at most 7
    assert [len(e[4]) for e in blocks] == [7] * 7 + [0, 0, 7, 7]
    assert dbl.calls == [(host.COMP_LZ4, 6, 6 * limit), (host.COMP_ZSTD, 6, 6 * limit)]   # one call per method, min(limit, 290) rows per block of room
    kept = sum(len(e[4]) for e in blocks)
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"], t["rows"]) == (13, 40 * 11, 220 + 39 + 11, 1, 2, 2, kept)
    assert t["bytes_back"] == 12 * 32 + kept * (24 + 16)                  # a table row for the rejected stream too
    # the merge of the blocks a snapshot sees (here: the xids below 505 and the frozen one) is the plain sort of their rows
    L.cryo_memrel_set_frozen(mem, firsts[6], True)
    events, _ = host.topn_scan(rel, ATTS4, KEYS, BY, limit, COLS)
    assert [e[2] for e in events if e[0] == "block"][:9] == [500, 501, 502, 503, 504, 505, 2, 507, 508]
    seen = [(e[4], e[5]) for e in events if e[0] == "block" and (e[2] < 505 or e[2] == 2)]
    every = [tr.topn_call([raws[k]], ATTS4, KEYS, BY, 290, COLS) for k in (0, 1, 2, 3, 4, 6)]
    flat = sorted(((tr.sort_key(BY, [int(x) for x in r["key"]], int(r["key_nulls"])), b, i), bytes(w))
                  for b, (_, recs, rows, _) in enumerate(every) for i, (r, w) in enumerate(zip(recs, rows)))
    for merge in MERGES:
        recs, rows = merge(BY, limit, seen)
        assert [bytes(w) for w in rows] == [w for _, w in flat[:limit]] and len(rows) == limit
    # descriptors the codec refuses; null arguments
    for by, lim, cols in ((BY, 0, COLS), ([], 5, COLS), ([(2, fr.INT4, 0)], 5, COLS), (BY, 5, [2])):
        with pytest.raises(host.TopnScanError) as e:
            host.topn_scan(rel, ATTS4, KEYS, by, lim, cols)
        assert e.value.code == E_ARG and e.value.events == [], (by, lim, cols)
    f, o, p = cc.filter_desc(ATTS4, KEYS), cc.order_desc(BY, 5), cc.project_desc(COLS)
    nb, nr = host.TOPN_BLOCK_FN(0), host.FETCH_REPORT_FN(0)
    assert L.cryo_topn_scan(C.byref(rel), None, C.byref(o[0]), C.byref(p[0]), nb, nr, None, None) == E_ARG
    assert L.cryo_topn_scan(C.byref(rel), C.byref(f[0]), None, C.byref(p[0]), nb, nr, None, None) == E_ARG
    assert L.cryo_topn_scan(C.byref(rel), C.byref(f[0]), C.byref(o[0]), None, nb, nr, None, None) == E_ARG
    assert L.cryo_topn_scan(None, C.byref(f[0]), C.byref(o[0]), C.byref(p[0]), nb, nr, None, None) == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_topn_scan_windows(HT, oracle):
    """the window lowered to 4 chains (three windows), then to the compressed bytes of about three: several codec calls, the same
    delivery; a limit above 290 asks for 290 rows per block; a call the double refuses stops the walk and what was delivered stands"""
    L, dbl, _ = HT
    mem, rel, raws, firsts = _relation(L, oracle)
    whole, t0 = host.topn_scan(rel, ATTS4, KEYS, BY, 1000, COLS)
    assert dbl.calls == [(host.COMP_LZ4, 5, 5 * 290), (host.COMP_ZSTD, 4, 4 * 290)] and t0["codec_calls"] == 2 and t0["rows"] == 220
    dbl.calls.clear()
    L.cryo_topn_set_window(4, 0)
    got, t = host.topn_scan(rel, ATTS4, KEYS, BY, 1000, COLS)
    assert _flat(got) == _flat(whole)
    assert [c[:2] for c in dbl.calls] == [(host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 1)]
    assert {k: v for k, v in t.items() if k != "codec_calls"} == {k: v for k, v in t0.items() if k != "codec_calls"}
    dbl.calls.clear()
    # with rowid >= 100 and limit 5 the first window's calls keep 0 + 5 rows each, the second window's first call 5 + 5: refused.  The
    # first window's blocks stand, the totals say how far the walk got
    dbl.row_cap_limit = 9
    with pytest.raises(host.TopnScanError) as e:
        host.topn_scan(rel, ATTS4, [(1, fr.INT4, fr.GE, 100)], BY, 5, COLS)
    assert e.value.code == E_DSTSIZE and [ev[1] for ev in e.value.events] == firsts[:4]
    assert [len(ev[4]) for ev in e.value.events] == [0, 0, 5, 5]
    assert e.value.totals["codec_calls"] == 3 and e.value.totals["rows"] == 10 and e.value.totals["blocks"] == 8
    assert [c[:2] for c in dbl.calls] == [(host.COMP_LZ4, 2), (host.COMP_ZSTD, 2), (host.COMP_LZ4, 2)]   # no call after the refused one
    dbl.row_cap_limit = None
    dbl.calls.clear()
    csize = len(oracle.lz4_compress(raws[0], 1))
    L.cryo_topn_set_window(0, 3 * csize + csize // 2)
    got, t = host.topn_scan(rel, ATTS4, KEYS, BY, 1000, COLS)
    assert _flat(got) == _flat(whole) and t["codec_calls"] == len(dbl.calls) >= 3 and t["rows"] == t0["rows"]
    L.cryo_memrel_destroy(mem)


def test_without_a_topn_table_the_scan_is_unsupported(HT, oracle):
    L, dbl, _ = HT
    mem, rel, raws, firsts = _relation(L, oracle, nblocks=2)
    L.cryo_host_set_topn_ops(None)
    with pytest.raises(host.TopnScanError) as e:
        host.topn_scan(rel, ATTS4, [], BY, 5, COLS)
    assert e.value.code == E_UNSUPPORTED and e.value.events == [] and e.value.totals["blocks"] == 0
    L.cryo_memrel_destroy(mem)
