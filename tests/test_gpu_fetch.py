"""GPU tests of the tuple fetch (cryo_codec_fetch_batch, cryo_codec_fetch_blocks, cryo_multi_fetch_blocks).

Every record and every byte is compared with tests/fetch_ref.py, the numpy statement of the rules in include/cryo_codec.h,
applied to the ORACLE's decode of each stream."""
import ctypes as C
import struct

import numpy as np
import pytest

import fetch_ref as fr
import layout_ref
import oracle_lib
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def fch(codec):
    yield codec
    for opt, v in ((cc.OPT_ZSTD_CHECKSUM, 0), (cc.OPT_ENCODE_SEGMENT_BYTES, 0), (cc.OPT_WORKSPACE_MAX_BYTES, 0),
                   (cc.OPT_PIPE_MIN_BYTES, 64 << 20), (cc.OPT_POOL_BYTES, 0), (cc.OPT_LZ4_DECODE_PATH, 0),
                   (cc.OPT_ZSTD_DECODE_PATH, 0)):
        codec.set_option(opt, v)


def fetch_batch(codec, method, comps, B, requests, dst_cap=None):
    """cryo_codec_fetch_batch on device copies of the streams and of the request table: (records, dst bytes, total); the
    destination is filled with SENTINEL before the call"""
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
    first, pos = cc.request_table(requests)
    n_req = int(first[-1])
    cap = n * B if dst_cap is None else dst_cap
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(first.nbytes),
            codec.alloc(max(pos.nbytes, 16)), codec.alloc(cap + 64), codec.alloc(16 * max(n_req, 1)), codec.alloc(8)]
    d_src, d_off, d_sz, d_first, d_pos, d_dst, d_res, d_tot = bufs
    try:
        d_src.upload(packed)
        d_off.upload(offs)
        d_sz.upload(sizes)
        d_first.upload(first)
        if n_req:
            d_pos.upload(pos)
        d_dst.memset(SENTINEL)
        d_res.memset(0xEE)
        d_tot.memset(0xEE)
        codec.fetch_batch(method, d_src, d_off, d_sz, B, n, d_first, d_pos, n_req, d_dst, cap, d_res, d_tot)
        codec.sync()
        recs = d_res.download(dtype=np.uint8)[:16 * n_req].view(cc.FETCH_RESULT).copy()
        return recs, d_dst.download(), int(d_tot.download(dtype=np.uint64)[0])
    finally:
        for b in bufs:
            b.free()


def expect(oracle, method, comps, B, requests):
    return fr.fetch_call([fr.decode(oracle, method, c, B) for c in comps], requests)


def same(got, want, what=""):
    recs, dst, total = got
    erecs, packed, etotal = want
    assert recs.size == erecs.size, what
    for f in ("status", "len", "off"):
        bad = np.flatnonzero(recs[f] != erecs[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(recs[i]), tuple(erecs[i])) for i in bad[:5]])
    assert total == etotal, (what, total, etotal)
    diff = np.flatnonzero(dst[:etotal] != packed)
    assert diff.size == 0, (what, "first differing byte", int(diff[0]))
    assert (dst[etotal:] == SENTINEL).all(), (what, "a byte at or beyond the total was written")


def oracle_encode(oracle, method, raw):
    return oracle.lz4_compress(raw, 1) if method == METHOD_LZ4 else oracle.zstd_compress(raw, 1)


SHAPES = [[], [1], [290], [145], list(range(1, 291)), list(range(7, 291, 7)), [291], [65535], [1, 290, 291, 65535]]


# ---- valid streams, whoever wrote them ----
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_valid_streams(fch, oracle, stock, B):
    raws = [oracle.synth(31, d, B, d) for d in range(5)]
    for method in (METHOD_LZ4, METHOD_ZSTD):
        sources = {"oracle": [oracle_encode(oracle, method, r) for r in raws], "gpu": fch.compress_blocks(method, 1, raws)}
        if method == METHOD_ZSTD:
            fch.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
            sources["gpu checksummed"] = fch.compress_blocks(method, 1, raws)
            fch.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
        fch.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
        sources["gpu segment"] = fch.compress_blocks(method, 1, raws)
        fch.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
        if method == METHOD_LZ4 and stock.lz4 is not None:
            sources["liblz4"] = [stock.lz4_compress(r, 1) for r in raws]
        if method == METHOD_ZSTD and stock.zstd is not None:
            sources["libzstd"] = [stock.zstd_compress(r, 1) for r in raws]
        for rot, (name, comps) in enumerate(sources.items()):
            # every distribution meets every request shape; blocks with and without requests alternate
            streams = [comps[j % 5] for j in range(5 * len(SHAPES))]
            requests = [SHAPES[(j // 5 + j + rot) % len(SHAPES)] for j in range(len(streams))]
            decoded = [fr.decode(oracle, method, c, B) for c in comps]          # the oracle's decode of each stream
            assert all(np.array_equal(x, r) for x, r in zip(decoded, raws))
            want = fr.fetch_call([decoded[j % 5] for j in range(len(streams))], requests)
            same(fetch_batch(fch, method, streams, B, requests), want, (method, name))
            if name == "oracle":
                same(fetch_batch(fch, method, streams, B, [[] for _ in streams]), (np.zeros(0, fr.RESULT), np.zeros(0, np.uint8), 0),
                     "no request at all")
                recs, dst, total = fch.fetch_blocks(method, streams, B, requests, dst=np.full(len(streams) * B, SENTINEL, np.uint8))
                same((recs, dst, total), want, (method, name, "host buffers"))


def test_small_blocks(fch, oracle):
    """4 KiB blocks, and the smallest block there is (16 bytes: a header and nothing else)"""
    raws = [oracle.synth(5, d, 4096, d) for d in (1, 2, 4)]
    tiny = np.zeros(16, np.uint8)
    tiny[:8] = np.frombuffer(struct.pack("<II", 8, 16), np.uint8)
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, r) for r in raws]
        requests = [list(range(1, 120)), [2, 3, 50], [1]]
        same(fetch_batch(fch, method, comps, 4096, requests), fr.fetch_call(raws, requests))
        same(fetch_batch(fch, method, [oracle_encode(oracle, method, tiny)], 16, [[1, 2]]), fr.fetch_call([tiny], [[1, 2]]))


# ---- built blocks: tuple lengths around every word boundary, nonzero pads ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_built_blocks_pads_are_zero(fch, oracle, method):
    B = 131072
    lens = [1, 2, 3, 4, 5, 6, 7, 8, 9, 23, 24, 25, 4095, 4097]
    blocks = [fr.build_block(B, lens, pad=0xEE), fr.build_block(B, [B - 16], pad=0xEE), fr.build_block(B, [1] * 290, pad=0xEE),
              fr.build_block(B, lens[::-1], pad=0x01)]
    comps = [oracle_encode(oracle, method, b) for b in blocks]
    requests = [list(range(1, len(lens) + 1)), [1], list(range(1, 291)), [1, 2, 13, 14]]
    want = fr.fetch_call(blocks, requests)
    assert want[2] == sum(fr.maxalign(x) for x in lens) + (B - 16) + 290 * 8 + sum(fr.maxalign(x) for x in (4097, 4095, 2, 1))
    got = fetch_batch(fch, method, comps, B, requests)
    same(got, want)
    # said once more without the reference: the seven bytes behind each one-byte tuple are zero, the block's were 0xEE
    recs, dst, _ = got
    r = recs[len(lens) + 1]
    assert r["len"] == 1 and dst[int(r["off"])] != 0 and not dst[int(r["off"]) + 1:int(r["off"]) + 8].any()
    same(fch.fetch_blocks(method, comps, B, requests, dst=np.full(4 * B, SENTINEL, np.uint8)), want, "host buffers")


# ---- damage ----
def request_mix(rng, n):
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return list(range(1, 291))
    if kind == 1:
        return list(range(7, 291, 7))
    if kind == 2:
        return sorted(set(int(x) for x in rng.integers(1, 300, 12)))
    return [1, max(2, n // 2), 289, 290, 291]


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_layout_corruptions_match_reference(fch, oracle, method):
    B = 131072
    rng = np.random.default_rng(4000 + method)
    raws, requests = [], []
    for k in range(220):
        raws.append(layout_ref.corrupt(oracle.synth(77, k, B, int(rng.integers(0, 5))), rng))
        requests.append(request_mix(rng, 290))
    comps = [oracle_encode(oracle, method, r) for r in raws]
    want = fr.fetch_call(raws, requests)
    assert {fr.OK, fr.HEADER, fr.ITEM, fr.NOITEM} <= set(want[0]["status"].tolist())
    same(fetch_batch(fch, method, comps, B, requests), want)
    same(fch.fetch_blocks(method, comps, B, requests, dst=np.full(len(comps) * B, SENTINEL, np.uint8)), want, "host buffers")


def test_rejected_streams_between_good_neighbours(fch, oracle):
    B = 131072
    raws = [oracle.synth(21, k, B, d) for k, d in enumerate((0, 1, 2, 3, 1, 2))]
    requests = [[1, 2, 3], list(range(1, 291)), [5], [290], [7, 8], [100]]
    for method in (METHOD_LZ4, METHOD_ZSTD):
        good = [oracle_encode(oracle, method, r) for r in raws]
        base = fetch_batch(fch, method, good, B, requests)
        same(base, fr.fetch_call(raws, requests))
        hurt = list(good)
        hurt[1] = good[1][:len(good[1]) - 7]
        hurt[4] = good[4][:len(good[4]) // 2]
        want = expect(oracle, method, hurt, B, requests)
        assert want[0]["status"].tolist()[3:293] == [fr.STREAM] * 290
        got = fetch_batch(fch, method, hurt, B, requests)
        same(got, want)
        # the neighbours' records (but for their offsets) and bytes are what they were
        keep = np.r_[0:3, 293:295, 297:298]
        assert np.array_equal(got[0][["status", "len"]][keep], base[0][["status", "len"]][keep])
        for r in keep:
            a, b = got[0][r], base[0][r]
            assert np.array_equal(got[1][int(a["off"]):int(a["off"]) + int(a["len"])], base[1][int(b["off"]):int(b["off"]) + int(b["len"])])
    # a zstd frame whose checksum trailer no longer matches its content
    fch.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    frames = fch.compress_blocks(METHOD_ZSTD, 1, raws)
    fch.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
    same(fetch_batch(fch, METHOD_ZSTD, frames, B, requests), fr.fetch_call(raws, requests))
    frames[2] = frames[2].copy()
    frames[2][-2] ^= 0x10
    want = fr.fetch_call([r if i != 2 else None for i, r in enumerate(raws)], requests)
    same(fetch_batch(fch, METHOD_ZSTD, frames, B, requests), want)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_overlapping_items_and_bad_requests(fch, oracle, method):
    B = 131072
    big = B * 3 // 4
    o = np.zeros(B, np.uint8)                                   # 290 items that all claim the same three-quarter-block tuple
    o[B - big:] = (np.arange(big) % 253 + 1).astype(np.uint8)
    for i in range(290):
        o[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", B - big, big - 3), np.uint8)
    o[:8] = np.frombuffer(struct.pack("<II", 8 + 8 * 290, B - big), np.uint8)
    good = oracle.synth(3, 0, B, 1)
    blocks = [good, o, o, o, good, good, good, good, good]
    requests = [[1, 2], list(range(1, 291)), [17], [3, 4, 291], [2], [0, 1], [5, 5], [9, 8, 7], list(range(1, 100)) + [99]]
    want = fr.fetch_call(blocks, requests)
    st = want[0]["status"].tolist()
    assert st[2:292] == [fr.OVERLAP] * 290 and st[292] == fr.OK and st[293:296] == [fr.OVERLAP, fr.OVERLAP, fr.NOITEM]
    assert st[297:] == [fr.BADREQ] * (2 + 2 + 3 + 100) and want[2] < len(blocks) * B
    comps = [oracle_encode(oracle, method, b) for b in blocks]
    same(fetch_batch(fch, method, comps, B, requests), want)
    same(fch.fetch_blocks(method, comps, B, requests, dst=np.full(len(comps) * B, SENTINEL, np.uint8)), want, "host buffers")
    # 290 blocks that each return one overlapping tuple in full: the total is large but below n x B
    requests = [[1 + i] for i in range(290)]
    want = fr.fetch_call([o] * 290, requests)
    assert want[2] == 290 * big
    same(fetch_batch(fch, method, [comps[1]] * 290, B, requests), want)


# ---- decode routes, chunks ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_routes_and_chunks_give_the_same_records(fch, oracle, method):
    B = 131072
    rng = np.random.default_rng(9 + method)
    raws = [oracle.synth(55, k, B, k % 5) for k in range(10)]
    raws[3] = layout_ref.corrupt(raws[3], rng)
    base = [oracle_encode(oracle, method, r) for r in raws]
    n = 300
    comps = [base[j % 10] for j in range(n)]
    comps[41] = comps[41][:len(comps[41]) - 9]
    requests = [request_mix(rng, 290) if j % 4 else [] for j in range(n)]
    want = fr.fetch_call([raws[j % 10] if j != 41 else None for j in range(n)], requests)
    whole = fetch_batch(fch, method, comps, B, requests)                      # a few hundred blocks: the batch routes
    same(whole, want, "300 blocks")
    few = fetch_batch(fch, method, comps[:48], B, requests[:48])               # at most 64: the few-blocks routes
    same(few, fr.fetch_call([raws[j % 10] if j != 41 else None for j in range(48)], requests[:48]), "48 blocks")
    one = fetch_batch(fch, method, comps[5:6], B, [list(range(1, 291))])
    same(one, fr.fetch_call([raws[5]], [list(range(1, 291))]), "one block")
    # the handle's decode-path options do not change the routes the fetch takes
    fch.set_option(cc.OPT_LZ4_DECODE_PATH if method == METHOD_LZ4 else cc.OPT_ZSTD_DECODE_PATH, 1)
    same(fetch_batch(fch, method, comps, B, requests), want, "decode-path option set")
    fch.set_option(cc.OPT_LZ4_DECODE_PATH if method == METHOD_LZ4 else cc.OPT_ZSTD_DECODE_PATH, 0)
    # small workspace budgets: several chunks, and one block per chunk; the offsets run on across the chunks
    for budget in (6 << 20, 1 << 20):
        fch.set_option(cc.OPT_WORKSPACE_MAX_BYTES, budget)
        got = fetch_batch(fch, method, comps, B, requests)
        same(got, want, ("budget", budget))
        assert np.array_equal(got[0], whole[0])
        host = fch.fetch_blocks(method, comps[:80], B, requests[:80], dst=np.full(80 * B, SENTINEL, np.uint8))
        same(host, fr.fetch_call([raws[j % 10] if j != 41 else None for j in range(80)], requests[:80]), ("host, budget", budget))
    fch.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- the destination's capacity ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_destination_capacity(fch, oracle, method):
    B = 131072
    raws = [oracle.synth(8, k, B, d) for k, d in enumerate((1, 0, 2, 1))]
    comps = [oracle_encode(oracle, method, r) for r in raws]
    requests = [list(range(1, 291)), [1, 2, 3], list(range(10, 200, 3)), [290]]
    want = fr.fetch_call(raws, requests)
    total = want[2]
    same(fetch_batch(fch, method, comps, B, requests, dst_cap=total), want, "exactly the total")     # the 64 bytes behind survive
    exact = np.full(total + 32, SENTINEL, np.uint8)
    recs, dst, tot = fch.fetch_blocks(method, comps, B, requests, dst=exact[:total])
    same((recs, exact, tot), want, "host, exactly the total")
    # 8 bytes short: the device call says so in *d_total and writes every tuple that fits
    recs, dst, tot = fetch_batch(fch, method, comps, B, requests, dst_cap=total - 8)
    assert tot == total and tot > total - 8
    for f in ("status", "len", "off"):
        assert np.array_equal(recs[f], want[0][f])
    last = int(want[0]["off"][-1])
    assert np.array_equal(dst[:last], want[1][:last]) and (dst[last:] == SENTINEL).all()
    short = np.full(total + 32, SENTINEL, np.uint8)
    with pytest.raises(CryoError) as e:
        fch.fetch_blocks(method, comps, B, requests, dst=short[:total - 8])
    assert e.value.code == cc.E_DSTSIZE and (short[total - 8:] == SENTINEL).all()
    # several chunks: the call stops at the chunk that does not fit
    fch.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 1 << 20)
    with pytest.raises(CryoError) as e:
        fch.fetch_blocks(method, comps, B, requests, dst=short[:total - 8])
    assert e.value.code == cc.E_DSTSIZE and (short[total - 8:] == SENTINEL).all()
    recs, dst, tot = fch.fetch_blocks(method, comps, B, requests, dst=exact[:total])
    same((recs, exact, tot), want, "host, exactly the total, one block per chunk")
    fch.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- counters ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_transfer_and_codec_counters(fch, oracle, method):
    B = 131072
    rng = np.random.default_rng(12)
    raws = [oracle.synth(13, k, B, k % 4) for k in range(40)]
    comps = [oracle_encode(oracle, method, r) for r in raws]
    requests = [request_mix(rng, 290) if k % 5 else [] for k in range(40)]
    want = fr.fetch_call(raws, requests)
    n_req = want[0].size
    t0 = fch.transfer_counters()
    fch.check_blocks(method, comps, B)
    t1 = fch.transfer_counters()
    check_up = t1["h2d_bytes"] - t0["h2d_bytes"]
    fch.set_option(cc.OPT_POOL_BYTES, 8 * B)
    before_t, before_c = fch.transfer_counters(), fch.counters()
    got = fch.fetch_blocks(method, comps, B, requests, dst=np.full(40 * B, SENTINEL, np.uint8))
    after_t, after_c = fch.transfer_counters(), fch.counters()
    same(got, want)
    assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == want[2] + 16 * n_req
    table = ((8 * 41 + 15) & ~15) + ((2 * n_req + 15) & ~15)                 # as the header documents the padding
    assert after_t["h2d_bytes"] - before_t["h2d_bytes"] == check_up + table
    for k in ("pool_hits", "pool_misses", "pool_blocks"):
        assert after_t[k] == before_t[k], k
    assert after_c == before_c
    # several chunks: the same exact figures
    fch.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 4 << 20)
    before_t = fch.transfer_counters()
    same(fch.fetch_blocks(method, comps, B, requests, dst=np.full(40 * B, SENTINEL, np.uint8)), want)
    after_t = fch.transfer_counters()
    assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == want[2] + 16 * n_req
    assert after_t["h2d_bytes"] - before_t["h2d_bytes"] == check_up + table
    before_c = fch.counters()
    same(fetch_batch(fch, method, comps, B, requests), want)
    assert fch.counters() == before_c
    fch.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
    fch.set_option(cc.OPT_POOL_BYTES, 0)


# ---- several handles ----
def multi_fetch(method, comps, B, requests, devices, dst):
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    try:
        def chk(rc, what):
            assert rc == 0, (what, rc, L.cryo_multi_last_error(h))
        return cc.fetch_blocks_call(L.cryo_multi_fetch_blocks, h, chk, method, comps, B, requests, dst)
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_multi_fetch_blocks(fch, oracle, method):
    B = 131072
    rng = np.random.default_rng(3)
    raws = [oracle.synth(17, k, B, k % 5) for k in range(11)]
    raws[6] = layout_ref.corrupt(raws[6], rng)
    comps = [oracle_encode(oracle, method, r) for r in raws]
    comps[2] = comps[2][:40]
    blocks = [r if i != 2 else None for i, r in enumerate(raws)]
    requests = [request_mix(rng, 290) if k % 3 else [k + 1] for k in range(11)]
    one = fch.fetch_blocks(method, comps, B, requests, dst=np.full(11 * B, SENTINEL, np.uint8))
    same(one, fr.fetch_call(blocks, requests))
    same(multi_fetch(method, comps, B, requests, (0,), np.full(11 * B, SENTINEL, np.uint8)), fr.fetch_call(blocks, requests), "G = 1")
    for G in (2, 3):
        recs, dst, total = multi_fetch(method, comps, B, requests, (0,) * G, np.full(11 * B, SENTINEL, np.uint8))
        erecs, regions, etotal = fr.multi_call(blocks, requests, G, B)
        assert np.array_equal(recs["status"], one[0]["status"]) and np.array_equal(recs["len"], one[0]["len"])   # as one handle
        assert np.array_equal(recs["off"], erecs["off"]) and total == etotal
        for r, s in zip(recs, one[0]):                                        # the same bytes at each record's off
            if r["status"] == fr.OK:
                n8 = fr.maxalign(int(r["len"]))
                assert np.array_equal(dst[int(r["off"]):int(r["off"]) + n8], one[1][int(s["off"]):int(s["off"]) + n8])
        written = np.zeros(dst.size, bool)
        for g, (start, packed) in enumerate(regions):                         # regions disjoint, nothing else written
            assert np.array_equal(dst[start:start + packed.size], packed)
            assert not written[start:start + packed.size].any()
            written[start:start + packed.size] = True
        assert (dst[~written] == SENTINEL).all()


# ---- arguments ----
def test_arguments(fch, oracle):
    comp = oracle.lz4_compress(oracle.synth(1, 0, 4096, 1), 1)
    d = [fch.alloc(256) for _ in range(8)]
    L = fch.L
    try:
        for method, B in ((7, 4096), (METHOD_LZ4, 4092), (METHOD_LZ4, 8), (METHOD_LZ4, 0)):
            with pytest.raises(CryoError) as e:
                fch.fetch_batch(method, d[0], d[1], d[2], B, 1, d[3], d[4], 1, d[5], 64, d[6], d[7])
            assert e.value.code == cc.E_ARG
        p = [b.ptr for b in d]
        call = lambda *a: L.cryo_codec_fetch_batch(fch.h, METHOD_LZ4, *a)    # noqa: E731
        d[7].memset(0xEE)
        assert call(None, None, None, 4096, 0, None, None, 0, None, 0, None, p[7]) == cc.OK          # no block: total 0
        fch.sync()
        assert int(d[7].download(dtype=np.uint64)[0]) == 0
        assert call(p[0], p[1], p[2], 4096, 1, p[3], None, 1, p[5], 64, p[6], p[7]) == cc.E_ARG      # requests, no table
        assert call(p[0], p[1], p[2], 4096, 1, None, p[4], 1, p[5], 64, p[6], p[7]) == cc.E_ARG
        assert call(p[0], p[1], p[2], 4096, 1, p[3], p[4], 1, p[5] + 4, 64, p[6], p[7]) == cc.E_ARG  # d_dst not 8-byte aligned
        assert call(p[0], p[1], p[2], 4096, 1, p[3], p[4], 1, p[5], 64, p[6] + 8, p[7]) == cc.E_ARG  # d_result not 16-byte aligned
        assert call(p[0], p[1], p[2], 4096, 1, p[3], p[4], 1, p[5], 64, p[6], None) == cc.E_ARG
    finally:
        for b in d:
            b.free()
    with pytest.raises(CryoError) as e:
        fch.fetch_blocks(METHOD_ZSTD, [comp], 4100, [[1]])
    assert e.value.code == cc.E_ARG
    recs, _, total = fch.fetch_blocks(METHOD_LZ4, [], 4096, [])
    assert recs.size == 0 and total == 0
    # a request table that does not start at 0, or that decreases
    arr = np.ascontiguousarray(comp)
    src, szs = (C.c_void_p * 2)(arr.ctypes.data, arr.ctypes.data), (C.c_uint32 * 2)(arr.nbytes, arr.nbytes)
    pos, res, dst, tot = np.array([1, 2, 3], np.uint16), np.zeros(3, cc.FETCH_RESULT), np.zeros(8192, np.uint8), C.c_uint64()
    for first in ([1, 2, 3], [0, 2, 1]):
        f = np.array(first, np.uint64)
        assert L.cryo_codec_fetch_blocks(fch.h, METHOD_LZ4, src, szs, 2, 4096, f.ctypes.data, pos.ctypes.data, dst.ctypes.data,
                                         dst.nbytes, res.ctypes.data, C.byref(tot)) == cc.E_ARG
    f = np.array([0, 1, 3], np.uint64)
    assert L.cryo_codec_fetch_blocks(fch.h, METHOD_LZ4, src, szs, 2, 4096, f.ctypes.data, None, dst.ctypes.data, dst.nbytes,
                                     res.ctypes.data, C.byref(tot)) == cc.E_ARG
    assert L.cryo_codec_fetch_blocks(fch.h, METHOD_LZ4, src, szs, 2, 4096, f.ctypes.data, pos.ctypes.data, dst.ctypes.data,
                                     dst.nbytes, res.ctypes.data, C.byref(tot)) == cc.OK and tot.value > 0
