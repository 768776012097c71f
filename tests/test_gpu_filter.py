"""GPU tests of the scan filter (cryo_codec_filter_batch, cryo_codec_filter_blocks, cryo_multi_filter_blocks).

Every row of the block table, every record and every byte is compared with tests/filter_ref.py, the numpy statement of the rules
in include/cryo_codec.h, applied to the ORACLE's decode of each stream.  The destination and the record buffer are filled with a
sentinel before every call: nothing at or beyond the totals may be written."""
import ctypes as C

import numpy as np
import pytest

import filter_cases as fc
import filter_ref as fr
import oracle_lib
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
REC_SENTINEL = np.frombuffer(bytes([SENTINEL] * 8), cc.FILTER_REC)[0]
SYNTH_ATTS = [(4, 4), (-1, 4)]


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def flt(codec):
    yield codec
    for opt, v in ((cc.OPT_ZSTD_CHECKSUM, 0), (cc.OPT_ENCODE_SEGMENT_BYTES, 0), (cc.OPT_WORKSPACE_MAX_BYTES, 0),
                   (cc.OPT_PIPE_MIN_BYTES, 64 << 20), (cc.OPT_POOL_BYTES, 0)):
        codec.set_option(opt, v)


def oracle_encode(oracle, method, raw):
    return oracle.lz4_compress(raw, 1) if method == METHOD_LZ4 else oracle.zstd_compress(raw, 1)


def filter_batch(codec, method, comps, B, atts, keys, flags=0, dst_cap=None, rec_cap=None):
    """cryo_codec_filter_batch on device copies of the streams and of the descriptor: (table, record buffer, dst bytes, totals);
    the destination and the record buffer are filled with SENTINEL before the call"""
    n = len(comps)
    sizes = np.array([len(c) for c in comps], np.uint32)
    offs = np.zeros(n, np.uint64)
    at = 0
    for i, c in enumerate(comps):
        offs[i] = at
        at += (len(c) + 15) & ~15
    packed = np.zeros(max(at, 16), np.uint8)
    for i, c in enumerate(comps):
        packed[int(offs[i]):int(offs[i]) + len(c)] = np.asarray(c, np.uint8)
    _, a, k = cc.filter_desc(atts, keys, flags)
    cap = n * B if dst_cap is None else dst_cap
    rcap = n * 290 if rec_cap is None else rec_cap
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(a.nbytes), codec.alloc(k.nbytes),
            codec.alloc(cap + 64), codec.alloc(8 * rcap + 64), codec.alloc(32 * n), codec.alloc(16)]
    d_src, d_off, d_sz, d_atts, d_keys, d_dst, d_rec, d_tab, d_tot = bufs
    try:
        d_src.upload(packed)
        d_off.upload(offs)
        d_sz.upload(sizes)
        d_atts.upload(a)
        d_keys.upload(k)
        d_dst.memset(SENTINEL)
        d_rec.memset(SENTINEL)
        d_tab.memset(0xEE)
        d_tot.memset(0xEE)
        codec.filter_batch(method, d_src, d_off, d_sz, B, n, len(atts), d_atts, len(keys), d_keys if keys else None, flags,
                           d_dst, cap, d_rec, rcap, d_tab, d_tot)
        codec.sync()
        table = d_tab.download(dtype=np.uint8).view(cc.FILTER_BLOCK).copy()
        tot = d_tot.download(dtype=np.uint64)
        return table, d_rec.download(dtype=np.uint8).view(cc.FILTER_REC).copy(), d_dst.download(), (int(tot[0]), int(tot[1]))
    finally:
        for b in bufs:
            b.free()


def host_call(codec, method, comps, B, atts, keys, flags=0):
    n = max(len(comps), 1)
    return codec.filter_blocks(method, comps, B, cc.filter_desc(atts, keys, flags), dst=np.full(n * B, SENTINEL, np.uint8),
                               rec=np.full(n * 290, REC_SENTINEL, cc.FILTER_REC))


def same(got, want, what=""):
    table, recs, dst, total = got
    etable, erecs, packed, etotal = want
    assert table.size == etable.size, what
    for f in etable.dtype.names:
        bad = np.flatnonzero(table[f] != etable[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(table[i]), tuple(etable[i])) for i in bad[:5]])
    assert tuple(total) == tuple(etotal), (what, total, etotal)
    for f in erecs.dtype.names:
        bad = np.flatnonzero(recs[f][:erecs.size] != erecs[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(recs[i]), tuple(erecs[i])) for i in bad[:5]])
    assert (recs[erecs.size:].view(np.uint8) == SENTINEL).all(), (what, "a record at or beyond the total was written")
    diff = np.flatnonzero(dst[:packed.size] != packed)
    assert diff.size == 0, (what, "first differing byte", int(diff[0]))
    assert (dst[packed.size:] == SENTINEL).all(), (what, "a byte at or beyond the total was written")


def expect(oracle, method, comps, B, atts, keys, flags=0):
    return fr.filter_call([fr.decode(oracle, method, c, B) for c in comps], atts, keys, flags)


# ---- the hand-made vectors ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_crafted_blocks(flt, oracle, method):
    """every hand-made block of the CPU test in batches of 1, 4, 5 and 9 blocks (a lone wave, a full workgroup, one over, two
    over), alternating with a block of other tuples; device buffers, host buffers and COUNT_ONLY"""
    B = fc.B
    other = tc.build_block(B, [fc.T(i, 1000 + i, b"r", 10 * i, b"s", -i) for i in range(1, 31)])
    enc = {}

    def comp(b):
        key = b.tobytes()
        if key not in enc:
            enc[key] = oracle_encode(oracle, method, b)
        return enc[key]

    for idx, (name, blk, keys, matches, bad) in enumerate(fc.cases()):
        n = (1, 4, 5, 9)[idx % 4]
        blocks = [blk if j % 2 == 0 else other for j in range(n)]
        comps = [comp(b) for b in blocks]
        want = fr.filter_call(blocks, fc.ATTS, keys)
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        same(filter_batch(flt, method, comps, B, fc.ATTS, keys), want, name)
        if idx % 3 == 0:
            same(host_call(flt, method, comps, B, fc.ATTS, keys), want, (name, "host buffers"))
            cwant = fr.filter_call(blocks, fc.ATTS, keys, fr.COUNT_ONLY)
            same(filter_batch(flt, method, comps, B, fc.ATTS, keys, fr.COUNT_ONLY), cwant, (name, "count only"))


def test_all_ops_on_all_types(flt, oracle):
    B = fc.B
    blk = tc.build_block(B, fc.ops_block())
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, blk)] * 2
        for keys, att, op, value in fc.ops_keys()[method::2]:          # the two methods share the 120 keys between them
            got = filter_batch(flt, method, comps, B, fc.ATTS, keys)
            same(got, fr.filter_call([blk, blk], fc.ATTS, keys), keys)
            assert got[1]["pos"][:got[3][1] // 2].tolist() == fc.ops_expected(att, op, value), keys


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_none_and_all_alternate_and_overlap(flt, oracle, method):
    B = fc.B
    hit = tc.build_block(B, [fc.T(*fc.GOOD)] * 40)
    miss = tc.build_block(B, [fc.T(5, 100, b"abc", 8, b"xy", 900)] * 40)
    over = fc.overlap_block()
    for n in (1, 4, 5, 9):
        for first in (hit, miss):
            blocks = [first if j % 2 == 0 else (miss if first is hit else hit) for j in range(n)]
            want = fr.filter_call(blocks, fc.ATTS, fc.K4)
            assert set(want[0]["n_match"].tolist()) <= {0, 40}
            same(filter_batch(flt, method, [oracle_encode(oracle, method, b) for b in blocks], B, fc.ATTS, fc.K4), want, n)
    blocks = [hit, over, miss, over, hit]
    comps = [oracle_encode(oracle, method, b) for b in blocks]
    want = fr.filter_call(blocks, fc.ATTS, fc.K6)
    assert want[0]["status"].tolist() == [0, fr.OVERLAP, 0, fr.OVERLAP, 0] and want[0]["n_bad"].tolist() == [0, 1, 0, 1, 0]
    assert want[0]["n_match"].tolist() == [40, 0, 40, 0, 40] and want[1]["status"][40] == fr.ITEM
    same(filter_batch(flt, method, comps, B, fc.ATTS, fc.K6), want, "overlap")
    same(host_call(flt, method, comps, B, fc.ATTS, fc.K6), want, "overlap, host buffers")
    cwant = fr.filter_call(blocks, fc.ATTS, fc.K6, fr.COUNT_ONLY)                    # nothing is placed: no OVERLAP
    assert cwant[0]["status"].tolist() == [0] * 5 and cwant[0]["n_match"].tolist() == [40, 4, 40, 4, 40]
    same(filter_batch(flt, method, comps, B, fc.ATTS, fc.K6, fr.COUNT_ONLY), cwant, "overlap, count only")
    same(host_call(flt, method, comps, B, fc.ATTS, fc.K6, fr.COUNT_ONLY), cwant, "overlap, count only, host buffers")


# ---- the turns of a wave: 64 items each ----
def test_turn_boundaries(flt, oracle):
    B = 16384
    atts = [(4, 4)]
    blocks = []
    for n in (63, 64, 65, 128, 290):
        tuples = [tc.form_tuple(atts, [i + 1000 * (i % 2)]) for i in range(1, n + 1)]
        assert len(tuples[0]) == 28
        blocks.append((n, tc.build_block(B, tuples)))
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, b) for _, b in blocks]
        for what, keys in (("first", [(1, fr.INT4, fr.EQ, 1001)]), ("every second", [(1, fr.INT4, fr.GE, 1000)]),
                           ("all", [(1, fr.INT4, fr.GE, 0)]), ("none", [(1, fr.INT4, fr.LT, 0)])):
            want = fr.filter_call([b for _, b in blocks], atts, keys)
            if what == "every second":
                assert want[0]["n_match"].tolist() == [32, 32, 33, 64, 145]
            same(filter_batch(flt, method, comps, B, atts, keys), want, (method, what))
        for (n, b), c in zip(blocks, comps):                                       # only the last item of each
            keys = [(1, fr.INT4, fr.EQ, n + 1000 * (n % 2))]
            want = fr.filter_call([b], atts, keys)
            assert want[1]["pos"].tolist() == [n]
            same(filter_batch(flt, method, [c], B, atts, keys), want, (method, "last of", n))


# ---- the generator's blocks, whoever wrote the streams ----
def range_keys(lo, hi):
    return [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)]


@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_generator_blocks(flt, oracle, stock, B):
    dists = range(5) if B == 131072 else (1,)
    raws = [oracle.synth(31, d, B, d) for d in dists]
    first = dists[0] * 290
    keysets = [range_keys(first + 100, first + 700) if B == 131072 else range_keys(first + 3, first + 6), [(2, 0, fr.NOTNULL, 0)]]
    for method in (METHOD_LZ4, METHOD_ZSTD):
        sources = {"oracle": [oracle_encode(oracle, method, r) for r in raws], "gpu": flt.compress_blocks(method, 1, raws)}
        if method == METHOD_ZSTD:
            flt.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
            sources["gpu checksummed"] = flt.compress_blocks(method, 1, raws)
            flt.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
        flt.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
        sources["gpu segment"] = flt.compress_blocks(method, 1, raws)
        flt.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
        if method == METHOD_LZ4 and stock.lz4 is not None:
            sources["liblz4"] = [stock.lz4_compress(r, 1) for r in raws]
        if method == METHOD_ZSTD and stock.zstd is not None:
            sources["libzstd"] = [stock.zstd_compress(r, 1) for r in raws]
        for rot, (name, comps) in enumerate(sources.items()):
            decoded = [fr.decode(oracle, method, c, B) for c in comps]              # the oracle's decode of each stream
            assert all(np.array_equal(x, r) for x, r in zip(decoded, raws))
            keys = keysets[rot % 2] if name != "oracle" else keysets[0]
            want = fr.filter_call(decoded, SYNTH_ATTS, keys)
            same(filter_batch(flt, method, comps, B, SYNTH_ATTS, keys), want, (method, name))
            if name == "oracle":
                assert want[3][1] > 0
                same(host_call(flt, method, comps, B, SYNTH_ATTS, keys), want, (method, name, "host buffers"))
                want = fr.filter_call(decoded, SYNTH_ATTS, keysets[1])
                same(filter_batch(flt, method, comps, B, SYNTH_ATTS, keysets[1]), want, (method, name, "NOTNULL"))


# ---- damage ----
def test_rejected_streams_between_good_neighbours(flt, oracle):
    B = 131072
    raws = [oracle.synth(21, k, B, d) for k, d in enumerate((0, 1, 2, 3, 1, 2))]
    keys = range_keys(200, 1500)
    for method in (METHOD_LZ4, METHOD_ZSTD):
        good = [oracle_encode(oracle, method, r) for r in raws]
        hurt = list(good)
        hurt[1] = good[1][:len(good[1]) - 7]
        hurt[4] = good[4][:len(good[4]) // 2]
        want = expect(oracle, method, hurt, B, SYNTH_ATTS, keys)
        assert want[0]["status"].tolist()[1] == fr.STREAM and want[0]["status"].tolist()[4] == fr.STREAM
        assert want[0]["n_match"][0] == 91 and want[0]["n_match"][2] == 290
        same(filter_batch(flt, method, hurt, B, SYNTH_ATTS, keys), want, method)
        same(host_call(flt, method, hurt, B, SYNTH_ATTS, keys), want, (method, "host buffers"))
    # a zstd frame whose checksum trailer no longer matches its content
    flt.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    frames = flt.compress_blocks(METHOD_ZSTD, 1, raws)
    flt.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
    same(filter_batch(flt, METHOD_ZSTD, frames, B, SYNTH_ATTS, keys), fr.filter_call(raws, SYNTH_ATTS, keys))
    frames[2] = frames[2].copy()
    frames[2][-2] ^= 0x10
    want = fr.filter_call([r if i != 2 else None for i, r in enumerate(raws)], SYNTH_ATTS, keys)
    assert want[0]["status"].tolist() == [0, 0, fr.STREAM, 0, 0, 0]
    same(filter_batch(flt, METHOD_ZSTD, frames, B, SYNTH_ATTS, keys), want, "checksum mismatch")


# ---- chunks ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_chunks_give_the_same_results(flt, oracle, method):
    B = 131072
    raws = [oracle.synth(55, k, B, (1, 0, 2, 3, 4)[k % 5]) for k in range(40)]
    comps = [oracle_encode(oracle, method, r) for r in raws]
    comps[17] = comps[17][:len(comps[17]) - 9]
    keys = range_keys(1000, 9000)
    want = expect(oracle, method, comps, B, SYNTH_ATTS, keys)
    whole = filter_batch(flt, method, comps, B, SYNTH_ATTS, keys)
    same(whole, want, "one chunk")
    flt.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 2 << 20)               # at most 15 decoded blocks of 128 KiB fit: three chunks or more
    got = filter_batch(flt, method, comps, B, SYNTH_ATTS, keys)
    same(got, want, "small budget")
    for a, b in zip(got[:3], whole[:3]):
        assert np.array_equal(a, b)
    # the totals run on across the chunks: every block starts where the one before ended
    t = got[0]
    assert (t["rec_first"][1:] == t["rec_first"][:-1] + t["n_match"][:-1] + t["n_bad"][:-1]).all() and (np.diff(t["off"].astype(np.int64)) >= 0).all()
    same(host_call(flt, method, comps, B, SYNTH_ATTS, keys), want, "host buffers, small budget")
    same(host_call(flt, method, comps, B, SYNTH_ATTS, keys, fr.COUNT_ONLY), expect(oracle, method, comps, B, SYNTH_ATTS, keys, fr.COUNT_ONLY),
         "host buffers, small budget, count only")
    flt.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- more than 256 blocks in one chunk: the second tile of the offset scan ----
TILE_B, TILE_N, TILE_CUT = 4096, 330, 262


@pytest.fixture(scope="module")
def two_tiles(oracle):
    """ten generator blocks of 4 KiB, repeated to 330: at this size the WIDE and RANDOM blocks hold 290 bad items each (records
    without bytes), the others 56 and 102 tuples or none; the keys pass some tuples of blocks 1 and 2 and none of blocks 6 and 7.
    Block 262 stands for a stream the decoders reject.  (raws, keys, the reference's result: one for both methods)"""
    raws = [oracle.synth(77, k, TILE_B, k % 5) for k in range(10)]
    keys = range_keys(311, 650)
    blocks = [None if i == TILE_CUT else raws[i % 10] for i in range(TILE_N)]
    return raws, keys, fr.filter_call(blocks, SYNTH_ATTS, keys)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_second_tile_of_the_offset_scan(flt, oracle, two_tiles, method):
    """330 blocks are one chunk under the default budget, so k_filter_offsets runs two tiles of 256 and 74 rows: the running
    totals carried into the second tile and the sums inside it, with a rejected stream, a block without a match and partly
    matching blocks beyond row 256; device buffers and host buffers against the reference, nothing left out"""
    raws, keys, want = two_tiles
    enc = [oracle_encode(oracle, method, r) for r in raws]
    comps = [enc[i % 10] for i in range(TILE_N)]
    comps[TILE_CUT] = comps[TILE_CUT][:len(comps[TILE_CUT]) - 9]
    assert all(np.array_equal(fr.decode(oracle, method, c, TILE_B), r) for c, r in zip(enc, raws))
    assert fr.decode(oracle, method, comps[TILE_CUT], TILE_B) is None
    t = want[0]
    assert t["status"][TILE_CUT] == fr.STREAM and set(t["status"].tolist()) == {0, fr.STREAM}
    assert (t["n_items"][256], t["n_match"][256], t["n_bad"][256]) == (56, 0, 0)      # tuples, and none of them passes
    assert 0 < t["n_match"][261] < t["n_items"][261] and 0 < t["n_match"][272] < t["n_items"][272]
    assert t["n_bad"][255] == 290 and t["rec_first"][256] > 0 and t["off"][256] > 0
    for what, got in (("device buffers", filter_batch(flt, method, comps, TILE_B, SYNTH_ATTS, keys)),
                      ("host buffers", host_call(flt, method, comps, TILE_B, SYNTH_ATTS, keys))):
        same(got, want, (method, what))
        # every row starts where the one before ended, across row 256 as anywhere else
        g, recs = got[0], got[1][:got[3][1]]
        nrec = g["n_match"].astype(np.uint64) + g["n_bad"]
        assert (g["rec_first"][1:] == g["rec_first"][:-1] + nrec[:-1]).all(), (method, what)
        room = np.where(recs["status"] == 0, (recs["len"].astype(np.uint64) + 7) & ~np.uint64(7), 0)
        upto = np.concatenate([[0], np.cumsum(room, dtype=np.uint64)]).astype(np.uint64)
        assert (g["off"] == upto[g["rec_first"]]).all() and got[3][0] == upto[-1], (method, what)


# ---- the caps ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_caps(flt, oracle, method):
    B = 131072
    raws = [oracle.synth(8, k, B, d) for k, d in enumerate((1, 0, 2, 1))]
    comps = [oracle_encode(oracle, method, r) for r in raws]
    keys = range_keys(50, 1100)
    want = fr.filter_call(raws, SYNTH_ATTS, keys)
    tb, tr = want[3]
    assert tb > 0 and tr > 0
    same(filter_batch(flt, method, comps, B, SYNTH_ATTS, keys, dst_cap=tb, rec_cap=tr), want, "exactly the totals")
    desc = cc.filter_desc(SYNTH_ATTS, keys)
    dst, rec = np.full(tb + 32, SENTINEL, np.uint8), np.full(tr + 4, REC_SENTINEL, cc.FILTER_REC)
    table, _, _, tot = flt.filter_blocks(method, comps, B, desc, dst=dst[:tb], rec=rec[:tr])
    same((table, rec, dst, tot), want, "host, exactly the totals")
    # one unit short: the device call reports the full need and writes nothing past the caps
    table, recs, out, tot = filter_batch(flt, method, comps, B, SYNTH_ATTS, keys, dst_cap=tb - 8, rec_cap=tr - 1)
    assert tot == (tb, tr)
    for f in want[0].dtype.names:
        assert np.array_equal(table[f], want[0][f])
    last = tb - fr.maxalign(int(want[1]["len"][-1]))
    assert np.array_equal(out[:last], want[2][:last]) and (out[last:] == SENTINEL).all()
    assert np.array_equal(recs[:tr - 1], want[1][:tr - 1]) and (recs[tr - 1:].view(np.uint8) == SENTINEL).all()
    for budget in (0, 1 << 20):                                        # one chunk; one block per chunk
        flt.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
        for dcap, rcap in ((tb - 8, tr), (tb, tr - 1)):
            dst, rec = np.full(tb + 32, SENTINEL, np.uint8), np.full(tr + 4, REC_SENTINEL, cc.FILTER_REC)
            with pytest.raises(CryoError) as e:
                flt.filter_blocks(method, comps, B, desc, dst=dst[:dcap], rec=rec[:rcap])
            assert e.value.code == cc.E_DSTSIZE and (dst[dcap:] == SENTINEL).all() and (rec[rcap:].view(np.uint8) == SENTINEL).all()
    flt.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- counters ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_transfer_and_codec_counters(flt, oracle, method):
    B = 131072
    raws = [oracle.synth(13, k, B, k % 4) for k in range(40)]
    comps = [oracle_encode(oracle, method, r) for r in raws]
    keys = range_keys(2000, 2500)
    want = fr.filter_call(raws, SYNTH_ATTS, keys)
    flt.set_option(cc.OPT_POOL_BYTES, 8 * B)
    for budget in (0, 4 << 20):
        flt.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
        before_t, before_c = flt.transfer_counters(), flt.counters()
        got = host_call(flt, method, comps, B, SYNTH_ATTS, keys)
        after_t, after_c = flt.transfer_counters(), flt.counters()
        same(got, want)
        assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 32 * 40 + 8 * want[3][1] + want[3][0]
        for k in ("pool_hits", "pool_misses", "pool_blocks"):
            assert after_t[k] == before_t[k], k
        assert after_c == before_c
        before_t = flt.transfer_counters()
        host_call(flt, method, comps, B, SYNTH_ATTS, keys, fr.COUNT_ONLY)
        assert flt.transfer_counters()["d2h_bytes"] - before_t["d2h_bytes"] == 32 * 40
    flt.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
    flt.set_option(cc.OPT_POOL_BYTES, 0)


# ---- several handles ----
def multi_filter(method, comps, B, atts, keys, flags, devices):
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    try:
        def chk(rc, what):
            assert rc == 0, (what, rc, L.cryo_multi_last_error(h))
        n = len(comps)
        return cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, flags),
                                     np.full(n * B, SENTINEL, np.uint8), np.full(n * 290, REC_SENTINEL, cc.FILTER_REC))
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("devices", [(0,), (0, 0), (0, 1)])
def test_multi_filter_blocks(flt, oracle, devices):
    """one handle; two handles on one device; two devices"""
    if max(devices) >= cc.device_count():
        pytest.skip("one device visible")
    handles = len(devices)
    B = 131072
    raws = [oracle.synth(17, k, B, k % 5) for k in range(11)]
    keys = range_keys(300, 2000)
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, r) for r in raws]
        comps[2] = comps[2][:40]
        blocks = [r if i != 2 else None for i, r in enumerate(raws)]
        table, recs, dst, total = multi_filter(method, comps, B, SYNTH_ATTS, keys, 0, devices)
        if handles == 1:
            same((table, recs, dst, total), fr.filter_call(blocks, SYNTH_ATTS, keys), "G = 1")
            continue
        etable, regions, etotal = fr.multi_call(blocks, SYNTH_ATTS, keys, handles, B)
        for f in etable.dtype.names:
            assert np.array_equal(table[f], etable[f]), f
        assert total == etotal
        wb, wr = np.zeros(dst.size, bool), np.zeros(recs.size, bool)
        for b0, packed, r0, rs in regions:                                # regions disjoint, nothing else written
            assert np.array_equal(dst[b0:b0 + packed.size], packed) and np.array_equal(recs[r0:r0 + rs.size], rs)
            wb[b0:b0 + packed.size] = True
            wr[r0:r0 + rs.size] = True
        assert (dst[~wb] == SENTINEL).all() and (recs[~wr].view(np.uint8) == SENTINEL).all()
        one = fr.filter_call(blocks, SYNTH_ATTS, keys)
        for i in range(11):                                               # the block table finds everything
            assert fr.tuples_of(table, recs, dst, i) == fr.tuples_of(one[0], one[1], one[2], i)
        ctab, _, _, ctot = multi_filter(method, comps, B, SYNTH_ATTS, keys, fr.COUNT_ONLY, devices)
        assert ctot == (0, 0) and np.array_equal(ctab, fr.filter_call(blocks, SYNTH_ATTS, keys, fr.COUNT_ONLY)[0])


# ---- arguments ----
def test_descriptor_rules(flt, oracle):
    """every argument rule of the descriptor, on host arrays (refused before a device is touched) and on device arrays"""
    B = fc.B
    comp = oracle.lz4_compress(tc.build_block(B, [fc.T(*fc.GOOD)]), 1)
    L = flt.L
    arr = np.ascontiguousarray(comp)
    src, szs = (C.c_void_p * 1)(arr.ctypes.data), (C.c_uint32 * 1)(arr.nbytes)
    dst, rec, table, tot = np.zeros(B, np.uint8), np.zeros(290, cc.FILTER_REC), np.zeros(1, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
    bufs = [flt.alloc(6416), flt.alloc(96), flt.alloc(4096), flt.alloc(8), flt.alloc(4), flt.alloc(B), flt.alloc(8 * 290),
            flt.alloc(32), flt.alloc(16)]
    d_atts, d_keys, d_src, d_off, d_sz, d_dst, d_rec, d_tab, d_tot = bufs
    try:
        d_src.upload(np.concatenate([arr, np.zeros(4096 - arr.nbytes, np.uint8)]))
        d_off.upload(np.zeros(1, np.uint64))
        d_sz.upload(np.array([arr.nbytes], np.uint32))
        for name, atts, keys, flags, patch, ok in fc.descriptors():
            assert fr.desc_ok(atts, keys, flags) == (ok or patch is not None), name
            f, a, k = cc.filter_desc(atts, keys, flags)
            if patch:
                which, field, index, value = patch
                if which == "f":
                    f.rsv = value
                else:
                    (a if which == "a" else k)[field][index] = value
            rc = L.cryo_codec_filter_blocks(flt.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), dst.ctypes.data, dst.nbytes,
                                            rec.ctypes.data, rec.size, table.ctypes.data, tot)
            assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
            if len(atts):
                d_atts.upload(a)
            d_keys.upload(k)
            g = cc.CryoFilter(f.natts, f.nkeys, f.flags, f.rsv, d_atts.ptr, d_keys.ptr if len(keys) else None)
            rc = L.cryo_codec_filter_batch(flt.h, METHOD_LZ4, d_src.ptr, d_off.ptr, d_sz.ptr, B, 1, C.byref(g), d_dst.ptr, B, d_rec.ptr,
                                           290, d_tab.ptr, d_tot.ptr)
            flt.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    finally:
        for b in bufs:
            b.free()


def test_arguments(flt, oracle):
    comp = oracle.lz4_compress(oracle.synth(1, 0, 4096, 1), 1)
    d = [flt.alloc(256) for _ in range(9)]
    try:
        _, a, k = cc.filter_desc(SYNTH_ATTS, range_keys(1, 5))
        d[3].upload(a)
        d[4].upload(k)

        def call(method=METHOD_LZ4, B=4096, n=1, natts=2, nkeys=2, flags=0, dst=d[5], rec=d[6], tab=d[7], tot=d[8]):
            flt.filter_batch(method, d[0], d[1], d[2], B, n, natts, d[3], nkeys, d[4], flags, dst, 64, rec, 8, tab, tot)

        for kw in (dict(method=7), dict(B=4092), dict(B=8), dict(B=0), dict(natts=0), dict(natts=1601), dict(nkeys=5), dict(flags=2),
                   dict(tab=None), dict(tot=None), dict(dst=None), dict(rec=None)):
            with pytest.raises(CryoError) as e:
                call(**kw)
            assert e.value.code == cc.E_ARG, kw
        d[8].memset(0xEE)
        call(n=0)                                                         # no block: totals 0
        flt.sync()
        assert d[8].download(dtype=np.uint64)[:2].tolist() == [0, 0]
        bad = k.copy()
        bad["value"][0] = 1 << 31                                         # outside int4, found in the device copy
        d[4].upload(bad)
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
    finally:
        for b in d:
            b.free()
    with pytest.raises(CryoError) as e:
        flt.filter_blocks(METHOD_ZSTD, [comp], 4100, cc.filter_desc(SYNTH_ATTS, []))
    assert e.value.code == cc.E_ARG
    table, _, _, total = flt.filter_blocks(METHOD_LZ4, [], 4096, cc.filter_desc(SYNTH_ATTS, []))
    assert table.size == 0 and total == (0, 0)
    table, _, _, total = flt.filter_blocks(METHOD_LZ4, [comp], 4096, cc.filter_desc(SYNTH_ATTS, []))
    assert table["n_match"][0] == table["n_items"][0] > 0 and total[1] == table["n_items"][0]
