"""GPU tests of write verification: cryo_codec_verify_batch and CRYO_OPT_ENCODE_VERIFY.

verify_batch decodes streams with the automatic decode routes into handle workspace and compares them with the raw blocks:
every stream the oracle and the stock libraries write passes; a stream that decodes to other bytes fails with the offset of
its first differing byte (checked against the oracle's decode of the same stream), a stream the decoders reject fails with
no offset.  With the option on, every compress entry point returns the same bytes as with it off, chunks its verification
within CRYO_OPT_WORKSPACE_MAX_BYTES, never reads or writes outside a caller's slot area and leaves the decode counters alone."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc

pytestmark = pytest.mark.gpu

SIZES = [131072, 1 << 20, 300001]
NONE = cc.VERIFY_NONE


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def vc(codec):
    yield codec
    for opt, v in ((cc.OPT_ENCODE_VERIFY, 0), (cc.OPT_ENCODE_SEGMENT_BYTES, 0), (cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 1),
                   (cc.OPT_WORKSPACE_MAX_BYTES, 0), (cc.OPT_PIPE_MIN_BYTES, 64 << 20)):
        codec.set_option(opt, v)


def _verify(codec, method, raws, comps, B):
    """verify_batch over host arrays: (statuses, first-mismatch offsets)"""
    n = len(raws)
    offs = np.zeros(n, np.uint64)
    pos = 0
    for i, c in enumerate(comps):
        offs[i] = pos
        pos += (len(c) + 15) & ~15
    packed = np.zeros(max(pos, 16), np.uint8)
    for i, c in enumerate(comps):
        packed[int(offs[i]):int(offs[i]) + len(c)] = c
    bufs = [codec.alloc(n * B), codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(4 * n),
            codec.alloc(4 * n)]
    d_raw, d_comp, d_off, d_sz, d_st, d_first = bufs
    try:
        d_raw.upload(np.concatenate([np.asarray(r, np.uint8) for r in raws]))
        d_comp.upload(packed)
        d_off.upload(offs)
        d_sz.upload(np.array([len(c) for c in comps], np.uint32))
        d_st.memset(0x55)
        d_first.memset(0x55)
        codec.verify_batch(method, d_raw, B, B, n, d_comp, d_off, d_sz, d_st, d_first)
        codec.sync()
        return d_st.download(dtype=np.int32), d_first.download(dtype=np.uint32)
    finally:
        for b in bufs:
            b.free()


def _first_diff(a, b):
    d = np.nonzero(np.asarray(a, np.uint8) != np.asarray(b, np.uint8))[0]
    return int(d[0]) if len(d) else NONE


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_LZ4, 50), (METHOD_ZSTD, -5), (METHOD_ZSTD, 1),
                                          (METHOD_ZSTD, 3), (METHOD_ZSTD, 19)])
def test_accepts_oracle_and_stock_streams(vc, oracle, stock, method, param, B):
    raws = [oracle.synth(11, d, B, d) for d in range(5)]
    comps = [oracle.lz4_compress(r, param) if method == METHOD_LZ4 else oracle.zstd_compress(r, param) for r in raws]
    lib = stock.lz4 if method == METHOD_LZ4 else stock.zstd
    if lib is not None:
        comps += [stock.lz4_compress(r, param) if method == METHOD_LZ4 else stock.zstd_compress(r, param) for r in raws]
        raws = raws + raws
    st, first = _verify(vc, method, raws, comps, B)
    assert (st == cc.OK).all(), st
    assert (first == NONE).all()


def _lz4_literal_positions(s):
    """(stream position, output position) of the first literal of every sequence with literals"""
    out, pos, res = 0, 0, []
    while pos < len(s):
        t = int(s[pos]); pos += 1
        ll = t >> 4
        if ll == 15:
            while True:
                b = int(s[pos]); pos += 1; ll += b
                if b != 255:
                    break
        if ll:
            res.append((pos, out))
        pos += ll; out += ll
        if pos >= len(s):
            break
        pos += 2
        ml = t & 15
        if ml == 15:
            while True:
                b = int(s[pos]); pos += 1; ml += b
                if b != 255:
                    break
        out += ml + 4
    return res


def test_rejects_wrong_streams_with_exact_offsets(vc, oracle):
    B = 131072
    raw_w = oracle.synth(12, 0, B, cc.DIST_WIDE)
    raw_r = np.random.default_rng(12).integers(0, 256, B, dtype=np.uint8)  # incompressible: stored as a raw block
    raws, comps, expect = [], [], []
    # 1. an LZ4 literal byte flipped in the middle of the stream: still B bytes, one of them wrong
    good = oracle.lz4_compress(raw_w, 1)
    lits = _lz4_literal_positions(good)
    sp, op = lits[len(lits) // 2]
    bad = good.copy(); bad[sp] ^= 0x5A
    r, dec = oracle.lz4_decompress(bad, B)
    assert r == B and _first_diff(dec[:B], raw_w) == op > 0
    raws.append(raw_w); comps.append(bad); expect.append((cc.E_VERIFY, op))
    # 2. a byte of a zstd raw block flipped (incompressible data: the frame holds raw blocks)
    zgood = oracle.zstd_compress(raw_r, 1)
    assert len(zgood) > B
    zbad = zgood.copy(); zbad[len(zbad) // 2] ^= 0xFF
    r, dec = oracle.zstd_decompress(zbad, B)
    assert r == B
    off = _first_diff(dec[:B], raw_r)
    assert 0 < off < B
    raws.append(raw_r); comps.append(zbad); expect.append((cc.E_VERIFY, off))
    # 3. truncated streams: the decoders reject them
    raws += [raw_w, raw_w]; comps += [good[:-7], oracle.zstd_compress(raw_w, 1)[:-7]]
    expect += [(cc.E_VERIFY, NONE)] * 2
    # 4. streams that decode to B - 1 bytes
    raws += [raw_w, raw_w]; comps += [oracle.lz4_compress(raw_w[:B - 1], 1), oracle.zstd_compress(raw_w[:B - 1], 1)]
    expect += [(cc.E_VERIFY, NONE)] * 2
    # good blocks between them stay good
    raws += [raw_w, raw_r]; comps += [good, zgood]; expect += [(cc.OK, NONE)] * 2
    for method, idx in ((METHOD_LZ4, [0, 2, 4, 6]), (METHOD_ZSTD, [1, 3, 5, 7])):
        st, first = _verify(vc, method, [raws[i] for i in idx], [comps[i] for i in idx], B)
        for k, i in enumerate(idx):
            assert (st[k], first[k]) == expect[i], (method, i, st[k], first[k])
    # an LZ4 stream is no zstd frame
    st, first = _verify(vc, METHOD_ZSTD, [raw_w], [good], B)
    assert (st[0], first[0]) == (cc.E_VERIFY, NONE)


@pytest.mark.parametrize("B", [300001, 262148])
def test_exact_offsets_on_unaligned_raw_rows(vc, oracle, B):
    """block sizes that are not a multiple of 16 put raw rows at every byte (300 001) or 4-byte (262 148) offset: the
    compare's unaligned paths find the same first differing byte"""
    raws = [oracle.synth(19, i, B, cc.DIST_WIDE) for i in range(4)]
    comps = [oracle.lz4_compress(r, 1) for r in raws]
    want = [NONE] * 4
    for i in (1, 2, 3):
        lits = _lz4_literal_positions(comps[i])
        sp, op = lits[(len(lits) * i) // 4]
        comps[i] = comps[i].copy()
        comps[i][sp] ^= 0x21
        r, dec = oracle.lz4_decompress(comps[i], B)
        assert r == B
        want[i] = _first_diff(dec[:B], raws[i])
    st, first = _verify(vc, METHOD_LZ4, raws, comps, B)
    assert list(st) == [cc.OK] + [cc.E_VERIFY] * 3
    assert list(first) == want


def _compress_dev(codec, method, param, raw, n, B, stride=None):
    stride = stride or cc.bound(method, B)
    d_src, d_dst, d_sz, d_st = codec.alloc(n * B), codec.alloc(n * stride), codec.alloc(4 * n), codec.alloc(4 * n)
    try:
        d_src.upload(raw)
        d_dst.memset(0)
        codec.compress_batch(method, param, d_src, B, B, n, d_dst, stride, d_sz, d_st)
        codec.sync()
        sz, st, out = d_sz.download(dtype=np.uint32), d_st.download(dtype=np.int32), d_dst.download()
        return [out[i * stride:i * stride + int(sz[i])].copy() for i in range(n)], st
    finally:
        for b in (d_src, d_dst, d_sz, d_st):
            b.free()


def _batch(oracle, B, n, seed=13):
    return np.concatenate([oracle.synth(seed, i, B, i % 5) for i in range(n)])


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 0), (METHOD_LZ4, 1), (METHOD_LZ4, 50), (METHOD_ZSTD, -5),
                                          (METHOD_ZSTD, 1), (METHOD_ZSTD, 3), (METHOD_ZSTD, 9), (METHOD_ZSTD, 19)])
def test_option_leaves_identical_path_output_unchanged(vc, oracle, method, param):
    B, n = 131072, 10
    raw = _batch(oracle, B, n)
    off, st0 = _compress_dev(vc, method, param, raw, n, B)
    before = vc.counters()
    vc.set_option(cc.OPT_ENCODE_VERIFY, 1)
    on, st1 = _compress_dev(vc, method, param, raw, n, B)
    after = vc.counters()
    assert (st0 == 0).all() and (st1 == 0).all()
    assert all(np.array_equal(a, b) for a, b in zip(off, on))
    assert after["blocks_decompressed"] == before["blocks_decompressed"] and after["bytes_out"] == before["bytes_out"]
    assert after["blocks_compressed"] == before["blocks_compressed"] + n


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_ZSTD, 1), (METHOD_ZSTD, 5), (METHOD_ZSTD, 13)])
def test_option_in_segment_mode(vc, oracle, stock, method, param):
    B, n = 1 << 20, 5
    raw = _batch(oracle, B, n, seed=14)
    vc.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
    vc.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 6)
    off, st0 = _compress_dev(vc, method, param, raw, n, B)
    vc.set_option(cc.OPT_ENCODE_VERIFY, 1)
    on, st1 = _compress_dev(vc, method, param, raw, n, B)
    assert (st0 == 0).all() and (st1 == 0).all()
    assert all(np.array_equal(a, b) for a, b in zip(off, on))
    ident = oracle.lz4_compress(raw[:B], param) if method == METHOD_LZ4 else oracle.zstd_compress(raw[:B], param)
    assert not np.array_equal(on[0], ident), "segment mode did not apply"
    for i in range(n):
        r, dec = (oracle.lz4_decompress if method == METHOD_LZ4 else oracle.zstd_decompress)(on[i], B)
        assert r == B and np.array_equal(dec[:B], raw[i * B:(i + 1) * B])


def _host_blocks(codec, method, param, raw, n, B):
    cap = cc.bound(method, B)
    dst = np.zeros(n * cap, np.uint8)
    sz = (C.c_uint32 * n)()
    codec._chk(codec.L.cryo_codec_compress_blocks(codec.h, method, param, raw.ctypes.data, B, n, dst.ctypes.data, cap, sz),
               "compress_blocks")
    return [dst[i * cap:i * cap + sz[i]].copy() for i in range(n)]


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_ZSTD, 1)])
def test_option_on_host_buffer_calls_and_multi(vc, oracle, method, param):
    B = 131072
    raw = _batch(oracle, B, 160, seed=15)
    ref = [oracle.lz4_compress(raw[i * B:(i + 1) * B], param) if method == METHOD_LZ4 else
           oracle.zstd_compress(raw[i * B:(i + 1) * B], param) for i in range(160)]
    vc.set_option(cc.OPT_ENCODE_VERIFY, 1)
    assert vc.get_option(cc.OPT_ENCODE_VERIFY) == 1
    before = vc.counters()["blocks_decompressed"]
    # _block
    for i in (0, 3):
        assert np.array_equal(vc.compress_block(method, param, raw[i * B:(i + 1) * B]), ref[i])
    # _blocks, one-shot and pipelined (160 blocks >= 128, the pipeline threshold lowered)
    got = _host_blocks(vc, method, param, raw[:8 * B], 8, B)
    assert all(np.array_equal(got[i], ref[i]) for i in range(8))
    vc.set_option(cc.OPT_PIPE_MIN_BYTES, 1 << 20)
    got = _host_blocks(vc, method, param, raw, 160, B)
    assert all(np.array_equal(got[i], ref[i]) for i in range(160))
    assert vc.last_verify_failure() is None
    assert vc.counters()["blocks_decompressed"] == before
    # cryo_multi over two handles of device 0 (compress_blocks_host by pointer per handle)
    L = vc.L
    h = C.c_void_p()
    devs = (C.c_int * 2)(0, 0)
    assert L.cryo_multi_open(devs, 2, C.byref(h)) == 0
    try:
        assert L.cryo_multi_set_option(h, cc.OPT_ENCODE_VERIFY, 1) == 0
        assert L.cryo_multi_set_option(h, cc.OPT_ENCODE_VERIFY, 2) == cc.E_ARG
        n, cap = 12, cc.bound(method, B)
        dst = np.zeros(n * cap, np.uint8)
        sz = (C.c_uint32 * n)()
        assert L.cryo_multi_compress_blocks(h, method, param, raw.ctypes.data, B, n, dst.ctypes.data, cap, sz) == 0
        assert all(np.array_equal(dst[i * cap:i * cap + sz[i]], ref[i]) for i in range(n))
        b, o = C.c_uint64(), C.c_uint32()
        assert L.cryo_multi_last_verify_failure(h, C.byref(b), C.byref(o)) == 0
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_chunked_verification_within_workspace_cap(vc, oracle, method):
    """a 16 MiB cap on a 96 x 128 KiB batch (12 MiB of decoded blocks alone, plus the decoders' workspace): several chunks"""
    B, n = 131072, 96
    raw = _batch(oracle, B, n, seed=16)
    off, _ = _compress_dev(vc, method, 1, raw, n, B)
    vc.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 16 << 20)
    vc.set_option(cc.OPT_ENCODE_VERIFY, 1)
    on, st = _compress_dev(vc, method, 1, raw, n, B)
    assert (st == 0).all() and all(np.array_equal(a, b) for a, b in zip(off, on))
    # a damaged stream in a late chunk is found at its own index and offset
    raws = [raw[i * B:(i + 1) * B] for i in range(n)]
    comps = [c.copy() for c in on]
    if method == METHOD_LZ4:
        sp, op = _lz4_literal_positions(comps[90])[-2]
        comps[90][sp] ^= 0x33
    else:
        r3 = np.random.default_rng(16).integers(0, 256, B, dtype=np.uint8)
        raws[90], comps[90] = r3, oracle.zstd_compress(r3, 1)
        comps[90][len(comps[90]) // 3] ^= 0x33
    r, dec = (oracle.lz4_decompress if method == METHOD_LZ4 else oracle.zstd_decompress)(comps[90], B)
    assert r == B
    st, first = _verify(vc, method, raws, comps, B)
    assert st[90] == cc.E_VERIFY and first[90] == _first_diff(dec[:B], raws[90])
    assert (np.delete(st, 90) == 0).all() and (np.delete(first, 90) == NONE).all()


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
@pytest.mark.parametrize("shift", [0, 8])
def test_no_access_outside_an_exact_slot_area(vc, oracle, method, shift):
    """incompressible blocks in slots of exactly cryo_codec_bound bytes: the last stream ends at (or next to) the area's end.
    The area (n x bound bytes, at an offset of `shift` into the allocation) sits between two guard regions checksummed
    before and after the verified compress: nothing is WRITTEN outside it, and every block still verifies and decodes.
    A read beyond the area leaves no trace a test can see; that the pass never reads there rests on verify_pass decoding
    the edge slots from padded copies."""
    B, n, G = 131072, 6, 4096
    stride = cc.bound(method, B)
    raw = np.random.default_rng(17).integers(0, 256, n * B, dtype=np.uint8)  # incompressible: streams near the bound
    vc.set_option(cc.OPT_ENCODE_VERIFY, 1)
    total = G + shift + n * stride + G
    base = vc.alloc(total)
    d_src, d_sz, d_st = vc.alloc(n * B), vc.alloc(4 * n), vc.alloc(4 * n)
    try:
        rng = np.random.default_rng(5)
        fill = rng.integers(0, 256, total, dtype=np.uint8)
        base.upload(fill)
        d_src.upload(raw)
        area = G + shift
        guard_sum = lambda img: (cc.checksum64(img[:area]), cc.checksum64(img[area + n * stride:]))
        before = guard_sum(fill)
        rc = vc.L.cryo_codec_compress_batch(vc.h, method, 1, d_src.ptr, B, B, n, base.ptr + area, stride, d_sz.ptr, d_st.ptr)
        assert rc == 0
        vc.sync()
        img = base.download(total)
        assert guard_sum(img) == before
        st, sz = d_st.download(dtype=np.int32), d_sz.download(dtype=np.uint32)
        assert (st == 0).all()
        assert int(sz[-1]) > B, "the last stream is not an incompressible one"
        for i in range(n):
            comp = img[area + i * stride:area + i * stride + int(sz[i])]
            r, dec = (oracle.lz4_decompress if method == METHOD_LZ4 else oracle.zstd_decompress)(comp, B)
            assert r == B and np.array_equal(dec[:B], raw[i * B:(i + 1) * B])
    finally:
        for b in (base, d_src, d_sz, d_st):
            b.free()


def test_option_values_and_counters(vc, oracle):
    assert vc.get_option(cc.OPT_ENCODE_VERIFY) == 0
    for v in (-1, 2, 12):
        with pytest.raises(cc.CryoError) as e:
            vc.set_option(cc.OPT_ENCODE_VERIFY, v)
        assert e.value.code == cc.E_ARG
    assert vc.get_option(cc.OPT_ENCODE_VERIFY) == 0
    vc.set_option(cc.OPT_ENCODE_VERIFY, 1)
    B = 131072
    raw = _batch(oracle, B, 4, seed=18)
    c0 = vc.counters()
    vc.compress_blocks(METHOD_LZ4, 1, [raw[i * B:(i + 1) * B] for i in range(4)])
    vc.compress_block(METHOD_ZSTD, 1, raw[:B])
    c1 = vc.counters()
    assert c1["blocks_decompressed"] == c0["blocks_decompressed"] and c1["bytes_out"] == c0["bytes_out"]
    assert c1["blocks_compressed"] == c0["blocks_compressed"] + 5
    # the standalone check leaves them alone too; a real decode still counts
    comps = [oracle.lz4_compress(raw[i * B:(i + 1) * B], 1) for i in range(4)]
    st, _ = _verify(vc, METHOD_LZ4, [raw[i * B:(i + 1) * B] for i in range(4)], comps, B)
    assert (st == 0).all() and vc.counters()["blocks_decompressed"] == c0["blocks_decompressed"]
    vc.decompress_blocks(METHOD_LZ4, comps, B)
    assert vc.counters()["blocks_decompressed"] == c0["blocks_decompressed"] + 4


def test_failure_paths_with_injected_fault(tmp_path):
    """the failure paths of every compress entry point, against a CRYO_DEBUG build of the library whose compress calls flip
    one byte of a chosen slot before verification (CRYO_VERIFY_FAULT): CRYO_E_VERIFY for that block only, its index and
    exact first differing byte in cryo_codec_last_verify_failure / cryo_codec_last_error, the lowest global index across the
    handles of a cryo_multi call (tests/verify_fault_child.py, in a process of its own)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "pg_cryogen_amd", "csrc")
    dbg = str(tmp_path / "cryo_codec_dbg.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17",
                           "-I" + os.path.join(root, "include"), "-I" + csrc, "-Wno-pass-failed", "-DCRYO_DEBUG",
                           "-x", "hip", "-c", os.path.join(csrc, "cryo_codec.cpp"), "-o", dbg])
    objs = [o for o in sorted(glob.glob(os.path.join(csrc, "*.o"))) if os.path.basename(o) != "cryo_codec.o"]
    so = str(tmp_path / "libcryo_codec_dbg.so")
    subprocess.check_call(["g++", "-shared", "-o", so] + objs + [dbg, "-Wl,--no-as-needed", "-lstdc++", "-lm"])
    env = dict(os.environ, CRYO_CODEC_LIB=so)
    env.pop("CRYO_VERIFY_FAULT", None)
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "verify_fault_child.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "verify-fault ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
