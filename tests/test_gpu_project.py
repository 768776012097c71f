"""GPU tests of the projecting scan (cryo_codec_project_batch, cryo_codec_project_blocks).

Every row of the block table, every record and every row byte is compared with tests/project_ref.py, the numpy statement of the
rules in include/cryo_codec.h, applied to the ORACLE's decode of each stream.  The device buffers are filled with a sentinel
before every call: nothing at or beyond the totals or the caps may be written."""
import ctypes as C
import struct

import numpy as np
import pytest

import agg_ref as ar
import filter_ref as fr
import project_cases as pc
import project_ref as pr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import pack_streams, project_batch, project_host as host_call, same_project as same

pytestmark = pytest.mark.gpu

SYNTH_ATTS = [(4, 4), (-1, 4)]
METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def prj(codec):
    yield codec
    for opt, v in ((cc.OPT_WORKSPACE_MAX_BYTES, 0), (cc.OPT_POOL_BYTES, 0)):
        codec.set_option(opt, v)


def oracle_encode(oracle, method, raw):
    return oracle.lz4_compress(raw, 1) if method == METHOD_LZ4 else oracle.zstd_compress(raw, 1)


def both(codec, oracle, blocks, B, atts, keys, cols, what, methods=METHODS):
    """device buffers and host buffers, on the oracle's streams of `blocks`, against project_ref; returns the expectation"""
    want = pr.project_call(blocks, atts, keys, cols)
    for method in methods:
        comps = [oracle_encode(oracle, method, b) for b in blocks]
        same(project_batch(codec, method, comps, B, atts, keys, cols), want, (what, method))
        same(host_call(codec, method, comps, B, atts, keys, cols), want, (what, method, "host buffers"))
    return want


# ---- the crafted blocks: widths, pads, duplicates, key columns, floats, NULLs, bad items, byte-string keys ----
@pytest.fixture(scope="module")
def crafted(oracle):
    """(cases, {(block bytes, method): stream}): every crafted block and the block of other tuples, encoded once"""
    cases = pc.cases()
    enc = {}
    for blk in [c[3] for c in cases] + [pc.other_block()]:
        for method in METHODS:
            enc[(blk.tobytes(), method)] = oracle_encode(oracle, method, blk)
    return cases, enc


@pytest.mark.parametrize("nb", [1, 4, 5, 9])
def test_crafted_blocks(prj, crafted, nb):
    """a lone wave, a full workgroup, one over, two over; crafted blocks alternate with a block of other tuples"""
    cases, enc = crafted
    other = pc.other_block()
    for name, B, atts, block, keys, cols, expected in cases:
        blocks = [block if i % 2 == 0 else other for i in range(nb)]
        want = pr.project_call(blocks, atts, keys, cols)
        # the hand-made expectation of the crafted block, wherever it stands in the batch
        for i in range(0, nb, 2):
            assert pr.rows_of(*want[:3], i) == [(p, nulls, row) for p, st, nulls, row in expected if st == 0], name
            assert (want[0]["n_match"][i], want[0]["n_bad"][i]) == (sum(e[1] == 0 for e in expected), sum(e[1] != 0 for e in expected))
        for method in METHODS:
            comps = [enc[(b.tobytes(), method)] for b in blocks]
            same(project_batch(prj, method, comps, B, atts, keys, cols), want, (name, nb, method))
            same(host_call(prj, method, comps, B, atts, keys, cols), want, (name, nb, method, "host buffers"))


def test_byte_string_key_and_the_integer_instantiation(prj, crafted):
    """one byte-string key: the compressed in-line and the external value are status 9, counted in n_bad, a record and no row; the
    same tuples under an integer key alone run the other instantiation and all match"""
    cases, enc = crafted
    by = {c[0]: c for c in cases}
    for name, n_match, n_bad in (("byte-string key", 2, 2), ("the same tuples, integer key", 5, 0)):
        _, B, atts, block, keys, cols, expected = by[name]
        for method in METHODS:
            table, rec, rows, (tw, tr) = project_batch(prj, method, [enc[(block.tobytes(), method)]], B, atts, keys, cols)
            assert (int(table["n_match"][0]), int(table["n_bad"][0]), tw, tr) == (n_match, n_bad, n_match, n_match + n_bad), name
            assert [(int(r["pos"]), int(r["status"]), int(r["nulls"])) for r in rec] == [e[:3] for e in expected], name
            assert [bytes(r) for r in rows] == [e[3] for e in expected if e[1] == 0], name


# ---- the turns of a wave: 64 items each ----
def test_turn_boundaries(prj, oracle):
    """0, 1, 63, 64, 65, 128, 129 and 290 items per block: every item matching, none, every other one"""
    blocks = [pc.turn_block(n) for n in pc.TURN_SIZES]
    sizes = list(pc.TURN_SIZES)
    t, _, rows, tot = both(prj, oracle, blocks, pc.TURN_B, pc.TURN_ATTS, pc.TURN_KEYS["all"], pc.TURN_COLS, "all")
    assert t["n_items"].tolist() == sizes and t["n_match"].tolist() == sizes and tot == (sum(sizes), sum(sizes))
    assert bytes(rows[-1]) == struct.pack("<b3xi", 290 % 251 - 125, 290)
    t, _, _, tot = both(prj, oracle, blocks, pc.TURN_B, pc.TURN_ATTS, pc.TURN_KEYS["none"], pc.TURN_COLS, "none")
    assert t["n_items"].tolist() == sizes and not t["n_match"].any() and tot == (0, 0)
    blocks = [pc.turn_block_alternating(n) for n in pc.TURN_SIZES]
    t, rec, _, tot = both(prj, oracle, blocks, pc.TURN_B, pc.TURN_ATTS, pc.ALTERNATING_KEYS, pc.TURN_COLS, "every other")
    assert t["n_match"].tolist() == [(n + 1) // 2 for n in sizes] and (rec["pos"] % 2 == 1).all()


# ---- blocks without an answer in the middle of a batch ----
def test_stream_and_header_blocks(prj, oracle):
    _, B, atts, good, keys, cols, expected = [c for c in pc.cases() if c[0] == "width mix, range on id"][0]
    blocks = [good, None, pc.header_block(), good, None, good]
    want = pr.project_call(blocks, atts, keys, cols)
    assert want[0]["status"].tolist() == [0, fr.STREAM, fr.HEADER, 0, fr.STREAM, 0]
    assert want[0]["row_first"].tolist() == [0, 3, 3, 3, 6, 6] and want[0]["rec_first"].tolist() == [0, 3, 3, 3, 6, 6]
    for method in METHODS:
        comps = [oracle_encode(oracle, method, good if b is None else b) for b in blocks]
        comps[1] = comps[1][:len(comps[1]) - 7]                            # truncated streams
        comps[4] = comps[4][:len(comps[4]) // 2]
        assert [ar.decode(oracle, method, c, B) is None for c in comps] == [b is None for b in blocks]
        same(project_batch(prj, method, comps, B, atts, keys, cols), want, method)
        same(host_call(prj, method, comps, B, atts, keys, cols), want, (method, "host"))


# ---- more than 256 blocks in one call, and the same call in several chunks ----
TILE_B, TILE_N, TILE_CUT = 4096, 330, 262


@pytest.fixture(scope="module")
def two_tiles(oracle):
    """ten generator blocks of 4 KiB, repeated to 330 (some hold bad items only, some tuples of which the keys pass a part, some
    none); block 262 stands for a stream the decoders reject.  (raws, keys, cols, the reference's result: one for both methods)"""
    raws = [oracle.synth(77, k, TILE_B, k % 5) for k in range(10)]
    keys = [(1, fr.INT4, fr.GE, 311), (1, fr.INT4, fr.LT, 650)]
    blocks = [None if i == TILE_CUT else raws[i % 10] for i in range(TILE_N)]
    return raws, keys, [1], pr.project_call(blocks, SYNTH_ATTS, keys, [1])


@pytest.mark.parametrize("method", METHODS)
def test_330_blocks_whole_and_in_chunks(prj, oracle, two_tiles, method):
    """330 blocks are one chunk under the default budget, so k_project_offsets runs two tiles of 256 and 74 rows.  Under a budget of
    1 MiB a chunk holds at most 83 blocks (a block takes 4 096 decoded bytes and 290 x 16 bytes of side area; the loop halves 330 to
    165, which needs 1.4 MiB, then to 83): four chunks or more, the running totals carried in device memory between them.  Both
    equal the reference and each other"""
    raws, keys, cols, want = two_tiles
    enc = [oracle_encode(oracle, method, r) for r in raws]
    comps = [enc[i % 10] for i in range(TILE_N)]
    comps[TILE_CUT] = comps[TILE_CUT][:len(comps[TILE_CUT]) - 9]
    assert ar.decode(oracle, method, comps[TILE_CUT], TILE_B) is None
    t = want[0]
    assert t["status"][TILE_CUT] == fr.STREAM and t["row_first"][256] > 0 and t["n_bad"].max() == 290 and want[3][0] > 0
    whole = project_batch(prj, method, comps, TILE_B, SYNTH_ATTS, keys, cols)
    same(whole, want, (method, "one chunk"))
    same(host_call(prj, method, comps, TILE_B, SYNTH_ATTS, keys, cols), want, (method, "host buffers"))
    g = whole[0]
    assert (g["row_first"][1:] == g["row_first"][:-1] + g["n_match"][:-1]).all()
    assert (g["rec_first"][1:] == g["rec_first"][:-1] + g["n_match"][:-1] + g["n_bad"][:-1]).all()
    prj.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 1 << 20)
    got = project_batch(prj, method, comps, TILE_B, SYNTH_ATTS, keys, cols)
    same(got, want, (method, "small budget"))
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], whole[:3])) and got[3] == whole[3]
    same(host_call(prj, method, comps, TILE_B, SYNTH_ATTS, keys, cols), want, (method, "host buffers, small budget"))
    prj.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- caps ----
def test_caps(prj, oracle):
    """row_cap and rec_cap each cut in the middle of a block, and at 0: the totals are counted in full, nothing at or beyond a cap
    is written (project_batch checks the sentinel), and the host-buffer call answers CRYO_E_DSTSIZE"""
    blocks = [pc.turn_block_alternating(65), pc.turn_block(64), pc.turn_block_alternating(129)]
    atts, keys, cols = pc.TURN_ATTS, pc.ALTERNATING_KEYS, pc.TURN_COLS
    want = pr.project_call(blocks, atts, keys, cols)
    need = want[3]
    assert need == (33 + 64 + 65, 33 + 64 + 65)
    for method in METHODS:
        comps = [oracle_encode(oracle, method, b) for b in blocks]
        same(host_call(prj, method, comps, pc.TURN_B, atts, keys, cols, need[0], need[1]), want, "exactly the need")
        for wcap, rcap in ((need[0] - 1, need[1]), (need[0], need[1] - 1), (50, 290 * 3), (290 * 3, 100), (0, 290 * 3), (290 * 3, 0), (0, 0)):
            with pytest.raises(CryoError) as e:
                host_call(prj, method, comps, pc.TURN_B, atts, keys, cols, wcap, rcap)
            assert e.value.code == cc.E_DSTSIZE, (wcap, rcap)
            table, rec, rows, total = project_batch(prj, method, comps, pc.TURN_B, atts, keys, cols, wcap, rcap)
            assert total == need and rows.shape[0] == min(wcap, need[0]) and rec.shape[0] == min(rcap, need[1])
            same((table, rec, rows, need), (want[0], want[1][:rcap], want[2][:wcap], need), ("cut at", wcap, rcap))


# ---- consistency with the filter ----
def filter_batch(codec, method, comps, B, atts, keys):
    """cryo_codec_filter_batch on device copies: (table, records, packed bytes)"""
    n = len(comps)
    packed, offs, sizes = pack_streams(comps)
    _, a, k = cc.filter_desc(atts, keys)
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(a.nbytes), codec.alloc(k.nbytes),
            codec.alloc(32 * n), codec.alloc(8 * 290 * n), codec.alloc(n * B), codec.alloc(16)]
    d_src, d_off, d_sz, d_atts, d_keys, d_table, d_rec, d_dst, d_total = bufs
    try:
        for d, h in ((d_src, packed), (d_off, offs), (d_sz, sizes), (d_atts, a), (d_keys, k)):
            d.upload(h)
        codec.filter_batch(method, d_src, d_off, d_sz, B, n, len(atts), d_atts, len(keys), d_keys if keys else None, 0, d_dst, n * B,
                           d_rec, 290 * n, d_table, d_total)
        codec.sync()
        tb, tr = (int(v) for v in d_total.download()[:16].view("<u8"))
        return d_table.download().view(cc.FILTER_BLOCK).copy(), d_rec.download()[:8 * tr].view(cc.FILTER_REC).copy(), d_dst.download()[:tb].copy()
    finally:
        for x in bufs:
            x.free()


@pytest.mark.parametrize("dist", [cc.DIST_NARROW, cc.DIST_WIDE])
def test_consistent_with_the_filter(prj, oracle, dist):
    """16 generator blocks of 128 KiB: the (block, pos) list of the projection's matches is the filter's under the same keys, and
    each row's column bytes are the bytes the reference walk finds in the tuple the filter returned"""
    B, n = 131072, 16
    raws = [oracle.synth(91, k, B, dist) for k in range(n)]
    ids = np.sort(pr.project_call(raws, SYNTH_ATTS, [], [1])[2][:, :4].copy().view("<i4").ravel())
    assert ids.size > 200
    keys = [(1, fr.INT4, fr.GE, int(ids[ids.size // 4])), (1, fr.INT4, fr.LT, int(ids[3 * ids.size // 4]))]
    comps = [oracle_encode(oracle, METHOD_LZ4, r) for r in raws]
    ftable, frec, fdst = filter_batch(prj, METHOD_LZ4, comps, B, SYNTH_ATTS, keys)
    table, rec, rows, (tw, tr) = project_batch(prj, METHOD_LZ4, comps, B, SYNTH_ATTS, keys, [1, 1])
    same((table, rec, rows, (tw, tr)), pr.project_call(raws, SYNTH_ATTS, keys, [1, 1]), dist)
    assert tw > 0 and (ftable["status"] == 0).all()
    for f in ("n_items", "n_match", "n_bad", "rec_first"):
        assert (table[f] == ftable[f]).all(), f
    for i in range(n):
        mine = pr.rows_of(table, rec, rows, i)
        theirs = fr.tuples_of(ftable, frec, fdst, i)
        assert [m[0] for m in mine] == [t[0] for t in theirs], i            # the same positions
        for (pos, nulls, row), (_, tup) in zip(mine, theirs):
            (isnull, at), = ar.walk(tup, SYNTH_ATTS, 1)
            assert not isnull and nulls == 0 and row == tup[at:at + 4] * 2, (i, pos)


# ---- arguments ----
def test_descriptor_rules(prj, oracle):
    """every argument rule of the two descriptors, on host arrays (refused before a device is touched: the transfer counters
    stand still) and on device arrays"""
    B = pc.B
    arr = np.ascontiguousarray(oracle.lz4_compress(pc.other_block(), 1))
    L = prj.L
    src, szs = (C.c_void_p * 1)(arr.ctypes.data), (C.c_uint32 * 1)(arr.nbytes)
    rows, rec, table = np.zeros((290, 64), np.uint8), np.zeros(290, cc.PROJECT_REC), np.zeros(1, cc.PROJECT_BLOCK)
    total = (C.c_uint64 * 2)()
    bufs = [prj.alloc(6416), prj.alloc(96), prj.alloc(128), prj.alloc(4096), prj.alloc(8), prj.alloc(4), prj.alloc(32),
            prj.alloc(8 * 290), prj.alloc(64 * 290), prj.alloc(16), prj.alloc(64)]
    d_atts, d_keys, d_cols, d_src, d_off, d_sz, d_table, d_rec, d_rows, d_total, d_consts = bufs
    try:
        d_src.upload(np.concatenate([arr, np.zeros(4096 - arr.nbytes, np.uint8)]))
        d_off.upload(np.zeros(1, np.uint64))
        d_sz.upload(np.array([arr.nbytes], np.uint32))
        for name, atts, keys, cols, flags, patch, ok in pc.descriptors():
            f, a, k = cc.filter_desc(atts, keys, flags)
            p, c = cc.project_desc(cols)
            if patch:
                which, field, index, value = patch
                if which in "fp":
                    {"f": f, "p": p}[which].rsv = value
                else:
                    {"a": a, "k": k, "c": c}[which][field][index] = value
            before = prj.transfer_counters()
            rc = L.cryo_codec_project_blocks(prj.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), C.byref(p), rows.ctypes.data, 290,
                                             rec.ctypes.data, 290, table.ctypes.data, total)
            assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
            if not ok:
                assert prj.transfer_counters() == before, name
            da, dk, consts, rebase = cc.filter_desc_device(atts, keys)
            dk = rebase(d_consts.ptr)
            if patch and patch[0] in "ak":
                {"a": da, "k": dk}[patch[0]][patch[1]][patch[2]] = patch[3]
            if len(atts):
                d_atts.upload(da)
            d_keys.upload(dk)
            d_consts.upload(consts)
            d_cols.upload(c)
            fd = cc.CryoFilter(f.natts, f.nkeys, f.flags, f.rsv, d_atts.ptr, d_keys.ptr if len(keys) else None)
            pd = cc.CryoProject(p.ncols, p.rsv, d_cols.ptr)
            rc = L.cryo_codec_project_batch(prj.h, METHOD_LZ4, d_src.ptr, d_off.ptr, d_sz.ptr, B, 1, C.byref(fd), C.byref(pd),
                                            d_rows.ptr, 290, d_rec.ptr, 290, d_table.ptr, d_total.ptr)
            prj.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    finally:
        for x in bufs:
            x.free()


def test_arguments(prj, oracle):
    comp = oracle.lz4_compress(pc.other_block(), 1)
    d = [prj.alloc(1024) for _ in range(10)]
    try:
        _, a, k = cc.filter_desc(pc.ATTS, [(1, fr.INT4, fr.GE, 1), (1, fr.INT4, fr.LT, 5)])
        _, p = cc.project_desc([1, 5])
        d[3].upload(a)
        d[4].upload(k)
        d[5].upload(p)

        class Shifted:                                                    # a device pointer that breaks the alignment rule
            def __init__(self, buf, by):
                self.ptr = buf.ptr + by

        def call(method=METHOD_LZ4, B=4096, n=1, natts=8, nkeys=2, ncols=2, cols=d[5], rows=d[6], wcap=16, rec=d[7], rcap=16, table=d[8],
                 total=d[9]):
            prj.project_batch(method, d[0], d[1], d[2], B, n, natts, d[3], nkeys, d[4], ncols, cols, rows, wcap, rec, rcap, table, total)

        for kw in (dict(method=7), dict(B=4092), dict(B=8), dict(B=0), dict(natts=0), dict(natts=1601), dict(nkeys=5), dict(ncols=0),
                   dict(ncols=9), dict(cols=None), dict(rows=None), dict(rec=None), dict(table=None), dict(total=None),
                   dict(table=Shifted(d[8], 8)), dict(rec=Shifted(d[7], 4)), dict(rows=Shifted(d[6], 4)), dict(cols=Shifted(d[5], 4)),
                   dict(total=Shifted(d[9], 4))):
            with pytest.raises(CryoError) as e:
                call(**kw)
            assert e.value.code == cc.E_ARG, kw
        for x in (d[6], d[7], d[8]):
            x.memset(0xEE)
        call(n=0)                                                         # no block: the totals are 0 and nothing else is written
        prj.sync()
        assert all((x.download() == 0xEE).all() for x in (d[6], d[7], d[8])) and not d[9].download()[:16].any()
        bad = p.copy()
        bad["att"][1] = 3                                                 # a varlena column, found in the device copy
        d[5].upload(bad)
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
    finally:
        for x in d:
            x.free()
    fdesc, pdesc = cc.filter_desc(pc.ATTS, []), cc.project_desc([1, 5])
    with pytest.raises(CryoError) as e:
        prj.project_blocks(METHOD_ZSTD, [comp], 4100, fdesc, pdesc, 8)
    assert e.value.code == cc.E_ARG
    table, rec, rows, total = prj.project_blocks(METHOD_LZ4, [], 4096, fdesc, pdesc, 8)
    assert table.size == 0 and total == (0, 0)
    table, rec, rows, total = prj.project_blocks(METHOD_LZ4, [comp], 4096, fdesc, pdesc, 8)
    assert table["n_match"][0] == table["n_items"][0] == 7 and total == (7, 7)
    assert [bytes(r) for r in rows[:7]] == [struct.pack("<ih2x", 100 + i, -(100 + i)) for i in range(7)]
