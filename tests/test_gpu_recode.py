"""GPU tests of recompression: cryo_codec_recode_batch, cryo_codec_recode_blocks, cryo_multi_recode_blocks and
cryo_recompress_relation through the shipped host library.

The main gate is equality without tolerance: recoding is defined as decompress followed by compress, both this project's
deterministic codecs, so every new stream must equal compress_blocks(decompress_blocks(streams)) byte for byte."""
import base64
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest

import oracle_lib
import recode_ref as rr
from mini_am import load_relation
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc, host

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TARGETS = [(METHOD_LZ4, 1), (METHOD_LZ4, 50), (METHOD_ZSTD, -5), (METHOD_ZSTD, 1), (METHOD_ZSTD, 3), (METHOD_ZSTD, 9),
           (METHOD_ZSTD, 19)]
ALL_ON = ((cc.OPT_ENCODE_SEGMENT_BYTES, 16384), (cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 6), (cc.OPT_ZSTD_CHECKSUM, 1),
          (cc.OPT_ENCODE_VERIFY, 1))
DEFAULTS = ((cc.OPT_ENCODE_SEGMENT_BYTES, 0), (cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 1), (cc.OPT_ZSTD_CHECKSUM, 0),
            (cc.OPT_ENCODE_VERIFY, 0), (cc.OPT_WORKSPACE_MAX_BYTES, 0))


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def rc(codec):
    for opt, v in DEFAULTS:
        codec.set_option(opt, v)
    yield codec
    for opt, v in DEFAULTS:
        codec.set_option(opt, v)


def note_missing(stock):
    """the comparisons with the live stock libraries run where they load; say so where one does not (the oracle, pinned to
    them by tests/test_oracle_golden.py, is compared at every level either way)"""
    for name, lib in (("liblz4.so.1", stock.lz4), ("libzstd.so.1", stock.zstd)):
        if lib is None:
            print("note: %s does not load here: compared with the oracle only" % name)


def oracle_encode(oracle, method, raw, param=1):
    return oracle.lz4_compress(raw, param) if method == METHOD_LZ4 else oracle.zstd_compress(raw, param)


def oracle_decode(oracle, method, comp, B):
    return (oracle.lz4_decompress if method == METHOD_LZ4 else oracle.zstd_decompress)(comp, B)


def golden_streams(method, B):
    name = "lz4" if method == METHOD_LZ4 else "zstd"
    return [np.frombuffer(base64.b64decode(s["data"]), np.uint8)
            for s in json.load(open(os.path.join(G, "streams.json")))["streams"] if s["method"] == name and s["B"] == B]


def sources(oracle, method, B):
    """streams of `method`: the five synthetic distributions (the CPU oracle's level-1 / acceleration-1 streams) and the
    stock-library streams of tests/golden/streams.json"""
    per = {4096: 1, 131072: 2}.get(B, 1)
    dists = (1, 2, 4) if B == 4096 else range(5)     # wide / random rows are degenerate at 4 KiB
    raws = [oracle.synth(31, per * d + k, B, d) for d in dists for k in range(per)]
    comps = [oracle_encode(oracle, method, r) for r in raws] + golden_streams(method, B)
    return comps


def expect_streams(codec, src_method, comps, B, dst_method, param):
    outs, st = codec.decompress_blocks(src_method, comps, B)
    assert (st == 0).all()
    return outs, codec.compress_blocks(dst_method, param, outs)


# ---- equality, the main gate ----
@pytest.mark.parametrize("opts", ["default", "all_on"])
@pytest.mark.parametrize("B", [4096, 131072, 1 << 20])
@pytest.mark.parametrize("src_method", [METHOD_LZ4, METHOD_ZSTD])
def test_recode_equals_decode_then_encode(rc, oracle, stock, src_method, B, opts):
    comps = sources(oracle, src_method, B)
    assert len(comps) >= (4 if B == 4096 else 10)
    if opts == "all_on":
        for opt, v in ALL_ON:
            rc.set_option(opt, v)
    else:
        note_missing(stock)
    for dst_method, param in TARGETS:
        raws, exp = expect_streams(rc, src_method, comps, B, dst_method, param)
        got, st, off, sz, _ = rc.recode_blocks(src_method, comps, B, dst_method, param)
        assert (st == 0).all(), (dst_method, param, st)
        for i, (g, e) in enumerate(zip(got, exp)):
            assert len(g) == len(e) and np.array_equal(g, e), (src_method, B, opts, dst_method, param, i, len(g), len(e))
        if opts == "default":
            # the byte-identical encoders: the libraries' own output (the oracle is pinned to them; the live libraries too)
            for i, (g, r) in enumerate(zip(got, raws)):
                if dst_method == METHOD_ZSTD and param == 19 and B > 131072 and i % 4:
                    continue                              # the CPU takes a second per such block
                assert np.array_equal(g, oracle_encode(oracle, dst_method, r, param)), (dst_method, param, i)
                if dst_method == METHOD_LZ4 and stock.lz4 is not None:
                    assert np.array_equal(g, stock.lz4_compress(r, param)), (param, i)
                if dst_method == METHOD_ZSTD and stock.zstd is not None and param in (-5, 1, 19):
                    assert np.array_equal(g, stock.zstd_compress(r, param)), (param, i)


# ---- the new streams are the stock libraries' to read ----
def test_new_streams_decode_with_stock_libraries(rc, oracle, stock):
    B = 131072
    raws = [oracle.synth(32, k, B, k % 5) for k in range(10)]
    flipped_content = 0
    note_missing(stock)
    for checksum in (0, 1):
        rc.set_option(cc.OPT_ZSTD_CHECKSUM, checksum)
        for src_method in (METHOD_LZ4, METHOD_ZSTD):
            comps = [oracle_encode(oracle, src_method, r) for r in raws]
            for dst_method, param in ((METHOD_LZ4, 1), (METHOD_ZSTD, 1), (METHOD_ZSTD, 9)):
                got, st, _, _, _ = rc.recode_blocks(src_method, comps, B, dst_method, param)
                assert (st == 0).all()
                for k, (g, r) in enumerate(zip(got, raws)):
                    n, out = oracle_decode(oracle, dst_method, g, B)
                    assert n == B and np.array_equal(out, r)
                    if dst_method == METHOD_LZ4 and stock.lz4 is not None:
                        n, out = stock.lz4_decompress(g, B)
                        assert n == B and np.array_equal(out, r)
                    if dst_method == METHOD_ZSTD and stock.zstd is not None:
                        n, out = stock.zstd_decompress(g, B)
                        assert n == B and np.array_equal(out, r)
                        if checksum:
                            assert g[4] & 4                         # the frame header's checksum flag
                            bent = g.copy()
                            bent[-1] ^= 0x01                        # the stored checksum no longer matches the content
                            assert stock.zstd_decompress(bent, B)[0] == -1
                            assert oracle_decode(oracle, dst_method, bent, B)[0] != B
                            if k % 5 == cc.DIST_RANDOM:
                                # `random` rows are stored as raw literals: a byte in the middle of the frame is content, and
                                # changing it leaves the framing alone; a checksum or a format error, stock libzstd says no
                                assert len(g) > B // 2
                                bent = g.copy()
                                bent[len(g) // 2] ^= 0x40
                                assert stock.zstd_decompress(bent, B)[0] == -1
                                assert oracle_decode(oracle, dst_method, bent, B)[0] != B
                                flipped_content += 1
    rc.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
    assert flipped_content > 0 or stock.zstd is None


# ---- packing ----
def test_packing_rule_and_untouched_tail(rc, oracle):
    B = 131072
    # zeros next to random: sizes a hundred and more times apart between neighbours
    raws = [oracle.synth(33, k, B, (4, 3)[k & 1]) for k in range(12)] + [oracle.synth(33, 20 + k, B, k % 5) for k in range(9)]
    comps = [oracle_encode(oracle, METHOD_LZ4, r) for r in raws]
    for dst_method, param in ((METHOD_ZSTD, 1), (METHOD_LZ4, 1)):
        cap = len(comps) * rr.align16(cc.bound(dst_method, B))
        dst = np.full(cap, 0xC7, np.uint8)
        got, st, off, sz, _ = rc.recode_blocks(METHOD_LZ4, comps, B, dst_method, param, dst=dst)
        assert (st == 0).all()
        assert max(sz[:12]) > 100 * min(sz[:12])
        _, exp = expect_streams(rc, METHOD_LZ4, comps, B, dst_method, param)
        want = np.full(cap, 0xC7, np.uint8)
        sizes, offs, total = rr.pack_buffer(exp, [0] * len(exp), want)
        assert [int(x) for x in sz] == sizes and [int(x) for x in off] == offs
        assert total < cap and np.array_equal(dst[:total], want[:total])      # streams and zero pads
        assert (dst[total:] == 0xC7).all()                                    # nothing beyond the packed total


# ---- transfers ----
def test_transfer_counters(rc, oracle):
    B = 131072
    raws = [oracle.synth(34, k, B, k % 5) for k in range(25)]
    for src_method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, src_method, r) for r in raws]
        t0 = rc.transfer_counters()
        rc.check_blocks(src_method, comps, B)
        t1 = rc.transfer_counters()
        c1 = rc.counters()
        got, st, off, sz, _ = rc.recode_blocks(src_method, comps, B, METHOD_ZSTD, 3)
        t2 = rc.transfer_counters()
        c2 = rc.counters()
        total = int(off[-1]) + rr.align16(sz[-1])
        assert t2["h2d_bytes"] - t1["h2d_bytes"] == t1["h2d_bytes"] - t0["h2d_bytes"]
        assert t2["d2h_bytes"] - t1["d2h_bytes"] == total + 8 * len(comps)
        for k in ("pool_hits", "pool_misses", "pool_blocks"):
            assert t2[k] == t1[k]
        # the internal decode counts nowhere, the encode as any compress
        assert c2["blocks_decompressed"] == c1["blocks_decompressed"] and c2["bytes_out"] == c1["bytes_out"]
        assert c2["blocks_compressed"] - c1["blocks_compressed"] == len(comps)
        assert c2["bytes_in"] - c1["bytes_in"] == len(comps) * B


def test_narrow_blocks_move_a_fraction_of_their_size(rc, oracle):
    """a `narrow` 1 MiB block has 290 item ids of 8 bytes and 290 tuple slots of 64 bytes: under 21 KiB that is not zero.
    Stored as literals, plus LZ4's length bytes for the 1 MiB zero run (about 4 KiB), it stays under 32 KiB: the bound of a
    quarter of the block size below is eight times that, and needs no measurement."""
    B, n = 1 << 20, 8
    raws = [oracle.synth(35, k, B, cc.DIST_NARROW) for k in range(n)]
    for src_method, dst_method, param in ((METHOD_LZ4, METHOD_ZSTD, 1), (METHOD_ZSTD, METHOD_LZ4, 1), (METHOD_LZ4, METHOD_ZSTD, 9)):
        comps = [oracle_encode(oracle, src_method, r) for r in raws]
        t0 = rc.transfer_counters()
        got, st, off, sz, _ = rc.recode_blocks(src_method, comps, B, dst_method, param)
        t1 = rc.transfer_counters()
        assert (st == 0).all()
        d2h = t1["d2h_bytes"] - t0["d2h_bytes"]
        print("narrow 1 MiB x %d, %d -> %d/%d: d2h %d bytes, h2d %d bytes" % (n, src_method, dst_method, param, d2h,
                                                                               t1["h2d_bytes"] - t0["h2d_bytes"]))
        assert d2h == int(off[-1]) + rr.align16(sz[-1]) + 8 * n
        assert d2h < n * B // 4
        assert t1["h2d_bytes"] - t0["h2d_bytes"] < n * B // 4


# ---- damaged sources ----
@pytest.mark.parametrize("src_method", [METHOD_LZ4, METHOD_ZSTD])
def test_damaged_sources_are_rejected_alone(rc, oracle, src_method):
    """streams of tests/golden/adversarial.json that the decode conformance tests already feed to the decoders and that they
    reject, mixed among good ones"""
    name = "lz4" if src_method == METHOD_LZ4 else "zstd"
    adv = [c for c in json.load(open(os.path.join(G, "adversarial.json")))["cases"]
           if c["method"] == name and len(c["data"]) > 0 and not c["ok"]]
    B = adv[0]["B"]
    bad = [np.frombuffer(base64.b64decode(c["data"]), np.uint8) for c in adv]
    bad = [b for b in bad if oracle_decode(oracle, src_method, b, B)[0] != B]
    assert len(bad) >= 20
    good = [oracle_encode(oracle, src_method, oracle.synth(36, k, B, (1, 2, 4)[k % 3])) for k in range(len(bad) + 5)]
    mixed, is_bad = [], []
    for k, g in enumerate(good):
        mixed.append(g); is_bad.append(False)
        if k < len(bad):
            mixed.append(bad[k]); is_bad.append(True)
    for dst_method, param in ((METHOD_ZSTD, 1), (METHOD_LZ4, 1)):
        clean, st0, _, _, _ = rc.recode_blocks(src_method, good, B, dst_method, param)
        assert (st0 == 0).all()
        got, st, off, sz, _ = rc.recode_blocks(src_method, mixed, B, dst_method, param)
        assert [int(s) for s in st] == [cc.E_CORRUPT if b else 0 for b in is_bad]
        assert all(int(sz[i]) == 0 for i in range(len(mixed)) if is_bad[i])
        sizes, offs, _ = rr.pack_offsets(sz, st)
        assert [int(x) for x in off] == offs
        kept = [g for g, b in zip(got, is_bad) if not b]
        assert len(kept) == len(clean) and all(np.array_equal(a, b) for a, b in zip(kept, clean))


# ---- chunking, edge calls ----
@pytest.mark.parametrize("verify", [0, 1])
def test_chunked_call_equals_one_chunk(rc, oracle, verify):
    B, n = 131072, 48
    raws = [oracle.synth(37, k, B, k % 5) for k in range(n)]
    rc.set_option(cc.OPT_ENCODE_VERIFY, verify)
    rc.set_option(cc.OPT_ZSTD_CHECKSUM, verify)
    for src_method, dst_method, param in ((METHOD_LZ4, METHOD_ZSTD, 3), (METHOD_ZSTD, METHOD_LZ4, 1), (METHOD_ZSTD, METHOD_ZSTD, 9)):
        comps = [oracle_encode(oracle, src_method, r) for r in raws]
        comps[7] = comps[7][:len(comps[7]) // 2]                    # a truncated stream: rejected, in whichever chunk it lands
        rc.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
        l0 = rc.counters()["launches"]
        one, st1, off1, sz1, _ = rc.recode_blocks(src_method, comps, B, dst_method, param)
        l1 = rc.counters()["launches"]
        rc.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 4 << 20)         # a chunk holds 128 KiB decoded + two slots per block
        t0 = rc.transfer_counters()
        many, st2, off2, sz2, _ = rc.recode_blocks(src_method, comps, B, dst_method, param)
        t1 = rc.transfer_counters()
        l2 = rc.counters()["launches"]
        rc.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)
        # launches rises once per decode and once per encode of a chunk: the limited call really ran in several chunks
        # (about 385 KiB per block against 4 MiB: at most 10 blocks per chunk, 5 chunks at least; 4 leaves room for a
        # chunk whose verification needs one edge decode less than the whole call's)
        assert l2 - l1 >= 4 * (l1 - l0) > 0, (l0, l1, l2)
        assert int(st1[7]) == cc.E_CORRUPT and (np.delete(st1, 7) == 0).all()
        assert np.array_equal(st1, st2) and np.array_equal(off1, off2) and np.array_equal(sz1, sz2)
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(one, many))
        assert t1["d2h_bytes"] - t0["d2h_bytes"] == int(off2[-1]) + rr.align16(sz2[-1]) + 8 * n


def test_edge_calls_leave_the_handle_usable(rc, oracle):
    B = 131072
    raws = [oracle.synth(38, k, B, 1 + k % 2) for k in range(5)]
    comps = [oracle_encode(oracle, METHOD_LZ4, r) for r in raws]
    _, exp = expect_streams(rc, METHOD_LZ4, comps, B, METHOD_ZSTD, 1)

    def usable():
        got, st, _, _, _ = rc.recode_blocks(METHOD_LZ4, comps, B, METHOD_ZSTD, 1)
        assert (st == 0).all() and all(np.array_equal(g, e) for g, e in zip(got, exp))

    usable()
    got, st, off, sz, _ = rc.recode_blocks(METHOD_LZ4, comps[:1], B, METHOD_ZSTD, 1)     # n = 1
    assert int(off[0]) == 0 and np.array_equal(got[0], exp[0])
    got, st, off, sz, _ = rc.recode_blocks(METHOD_LZ4, [], B, METHOD_ZSTD, 1)            # n = 0
    assert got == [] and len(st) == 0
    L = rc.L
    assert L.cryo_codec_recode_blocks(rc.h, METHOD_LZ4, None, None, 0, B, METHOD_ZSTD, 1, None, 0, None, None, None) == cc.OK
    # a capacity one byte short of the packed total, then exactly the total
    _, _, off, sz, _ = rc.recode_blocks(METHOD_LZ4, comps, B, METHOD_ZSTD, 1)
    total = int(off[-1]) + rr.align16(sz[-1])
    with pytest.raises(CryoError) as e:
        rc.recode_blocks(METHOD_LZ4, comps, B, METHOD_ZSTD, 1, dst=np.zeros(total - 1, np.uint8))
    assert e.value.code == cc.E_DSTSIZE
    usable()
    got, st, _, _, _ = rc.recode_blocks(METHOD_LZ4, comps, B, METHOD_ZSTD, 1, dst=np.zeros(total, np.uint8))
    assert (st == 0).all() and all(np.array_equal(g, x) for g, x in zip(got, exp))
    for args, code in (((7, comps, B, METHOD_ZSTD, 1), cc.E_ARG), ((METHOD_LZ4, comps, B, 7, 1), cc.E_ARG),
                       ((METHOD_LZ4, comps, 0, METHOD_ZSTD, 1), cc.E_ARG), ((METHOD_LZ4, comps, B, METHOD_ZSTD, 23), cc.E_UNSUPPORTED)):
        with pytest.raises(CryoError) as e:
            rc.recode_blocks(*args, dst=np.zeros(1 << 20, np.uint8))
        assert e.value.code == code, args[:1] + args[2:]
        usable()
    arr = np.zeros(64, np.uint8)
    assert L.cryo_codec_recode_blocks(rc.h, METHOD_LZ4, None, None, 3, B, METHOD_ZSTD, 1, arr.ctypes.data, 64, None, None, None) == cc.E_ARG
    usable()


# ---- the device-resident call ----
def test_recode_batch_with_a_larger_stride(rc, oracle):
    B = 131072
    raws = [oracle.synth(39, k, B, (k + 4) % 5) for k in range(11)]          # block 4: `random` rows
    for src_method, dst_method, param in ((METHOD_LZ4, METHOD_ZSTD, 1), (METHOD_ZSTD, METHOD_LZ4, 1)):
        comps = [oracle_encode(oracle, src_method, r) for r in raws]
        good = list(comps)
        comps[4] = comps[4][:len(comps[4]) // 2]
        n = len(comps)
        sizes = np.array([len(c) for c in comps], np.uint32)
        offs = np.zeros(n, np.uint64)
        pos = 0
        for i, c in enumerate(comps):
            offs[i] = pos
            pos += rr.align16(len(c))
        packed = np.zeros(pos, np.uint8)
        for i, c in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + len(c)] = c
        stride = cc.bound(dst_method, B) + 4096 + 8
        bufs = [rc.alloc(packed.nbytes), rc.alloc(8 * n), rc.alloc(4 * n), rc.alloc(n * stride), rc.alloc(4 * n), rc.alloc(4 * n)]
        d_src, d_off, d_sz, d_dst, d_osz, d_st = bufs
        try:
            d_src.upload(packed); d_off.upload(offs); d_sz.upload(sizes)
            d_dst.memset(0x3C)
            rc.recode_batch(src_method, d_src, d_off, d_sz, B, n, dst_method, param, d_dst, stride, d_osz, d_st)
            rc.sync()
            st, osz, raw = d_st.download(dtype=np.int32), d_osz.download(dtype=np.uint32), d_dst.download()
            with pytest.raises(CryoError) as e:
                rc.recode_batch(src_method, d_src, d_off, d_sz, B, n, dst_method, param, d_dst, cc.bound(dst_method, B) - 1, d_osz, d_st)
            assert e.value.code == cc.E_DSTSIZE
        finally:
            for b in bufs:
                b.free()
        _, exp = expect_streams(rc, src_method, good, B, dst_method, param)
        assert [int(s) for s in st] == [cc.E_CORRUPT if i == 4 else 0 for i in range(n)] and int(osz[4]) == 0
        for i in range(n):
            if i != 4:
                assert int(osz[i]) == len(exp[i]) and np.array_equal(raw[i * stride:i * stride + int(osz[i])], exp[i]), i


# ---- several handles ----
@pytest.mark.parametrize("handles", [2, 3])
def test_multi_recode_regions(rc, oracle, handles):
    B, n = 131072, 23
    raws = [oracle.synth(40, k, B, k % 5) for k in range(n)]
    comps = [oracle_encode(oracle, METHOD_LZ4, r) for r in raws]
    comps[5] = comps[5][:64]
    one, st1, _, sz1, _ = rc.recode_blocks(METHOD_LZ4, comps, B, METHOD_ZSTD, 3)
    L = cc.lib()
    m = C.c_void_p()
    assert L.cryo_multi_open((C.c_int * handles)(*([0] * handles)), handles, C.byref(m)) == 0

    def chk(code, what):
        if code != 0:
            raise CryoError(code, what)
    try:
        slot = rr.align16(cc.bound(METHOD_ZSTD, B))
        cap = handles * -(-n // handles) * slot
        dst = np.full(cap, 0x5D, np.uint8)
        got, st, off, sz, _ = cc.recode_blocks_call(L.cryo_multi_recode_blocks, m, chk, METHOD_LZ4, comps, B, METHOD_ZSTD, 3, dst=dst)
        assert np.array_equal(st, st1) and np.array_equal(sz, sz1) and int(st[5]) == cc.E_CORRUPT
        assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got, one))
        sizes, offs, region = rr.multi_offsets(sz, st, handles, cap)
        assert [int(x) for x in off] == offs and region % 16 == 0
        for g in range(handles):                               # zero pads, and nothing beyond each region's packed part
            idx = list(range(g, n, handles))
            end = offs[idx[-1]] + rr.align16(sizes[idx[-1]])
            assert (dst[end:(g + 1) * region] == 0x5D).all()
            for i in idx:
                assert (dst[offs[i] + sizes[i]:offs[i] + rr.align16(sizes[i])] == 0).all()
        with pytest.raises(CryoError) as e:
            cc.recode_blocks_call(L.cryo_multi_recode_blocks, m, chk, METHOD_LZ4, comps, B, METHOD_ZSTD, 3, dst=dst[:cap - 1])
        assert e.value.code == cc.E_DSTSIZE
        tc = cc.TransferCounters()
        assert L.cryo_multi_get_transfer_counters(m, C.byref(tc)) == 0
        assert tc.d2h_bytes == sum(rr.align16(s) for s in sizes) + 8 * n
    finally:
        L.cryo_multi_close(m)


# ---- the shipped host library, end to end ----
@pytest.fixture()
def HG():
    host.use(production=True)
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops")
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(131072)
    L.cryo_define_compression_gucs()
    L.cryo_cache_configure(16)
    yield L, errors
    host.set_int("cryo_gpu_zstd_checksum_guc", 0)
    L.cryo_cache_shutdown()
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)
    host.use(production=None)


def test_recompress_relation_production_library(HG, oracle, stock):
    """the 10 000-row mini-AM table loaded as LZ4, migrated to checksummed zstd: the stored-block check then covers the tuple
    bodies, a scan returns the same rows, and less than the relation's uncompressed size came back from the device"""
    L, errors = HG
    rows = [struct.pack("<i", i) for i in range(1, 10001)]
    mem, rel, blocks, firsts = load_relation(L, rows, 1, host.COMP_LZ4, batch=16)
    dmem = L.cryo_memrel_create()
    dst = host.CryoRel()
    L.cryo_memrel_bind(dmem, 4243, C.byref(dst))
    try:
        assert len(blocks) == 35 and not errors
        host.set_int("cryo_gpu_zstd_checksum_guc", 1)
        t0 = host.transfer_counters()
        moved, reports, totals = host.recompress_relation(rel, dst, host.COMP_ZSTD, 3)
        t1 = host.transfer_counters()
        assert reports == [] and not errors
        assert [m[0] for m in moved] == firsts and totals["blocks"] == 35 and totals["recoded"] == 35
        assert totals["verbatim"] == 0 and totals["skipped"] == 0 and totals["codec_calls"] == 1
        assert t1[1] - t0[1] < len(blocks) * host.get_block_size()                     # d2h below the uncompressed size
        assert t1[1] - t0[1] == sum(rr.align16(x) for x in _sizes(L, dst, moved)) + 8 * 35
        assert host.check_relation(dst)[0] == []
        # every first page: zstd, the source's xid, a checksummed frame that stock libzstd reads
        for (old, new, onp, nnp), raw in zip(moved, blocks):
            page = C.string_at(L.cryo_memrel_page(dmem, new), 8192)
            xid, method, csize, npages = struct.unpack_from("<IiIH", page, 32)
            assert (xid, method, npages) == (777, host.COMP_ZSTD, nnp) and nnp == L.cryo_pages_needed(csize)
            assert page[48 + 4] & 4
        # a scan of dst: the same blocks in the same order
        it = L.cryo_seqscan_iter_create()
        got = []
        while True:
            b = L.cryo_seqscan_iter_next(it)
            if L.cryo_memrel_nblocks(dmem) <= b:
                break
            e = C.c_int(-1)
            err = L.cryo_read_data(C.byref(dst), it, b, C.byref(e))
            if err == host.CRYO_ERR_EMPTY_BLOCK:
                continue
            assert err == host.CRYO_ERR_SUCCESS, (b, err)
            got.append(bytes(np.ctypeslib.as_array(C.cast(L.cryo_cache_get_data(e.value), C.POINTER(C.c_uint8)),
                                                   (host.get_block_size(),))))
        L.cryo_seqscan_iter_free(it)
        assert got == blocks and not errors
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def _sizes(L, dst, moved):
    out = []
    for _, new, _, _ in moved:
        comp, csize, method, xid = C.c_void_p(), C.c_size_t(), C.c_int(), C.c_uint32()
        chain, n = (C.c_uint32 * 64)(), C.c_uint32()
        assert L.cryo_stage_read_chain(C.byref(dst), new, C.byref(comp), C.byref(csize), C.byref(method), C.byref(xid), chain, 64,
                                       C.byref(n)) == 0
        out.append(csize.value)
    return out
