"""GPU tests of the segment-parallel encoders (CRYO_OPT_ENCODE_SEGMENT_BYTES = S; pg_cryogen.gpu_encode_segment_kb).

With S set, a block of more than S bytes is encoded by ceil(B / S) waves.  The stream is not liblz4's / libzstd's own
output, but it must be a valid LZ4 block / zstd frame that the pinned oracle decoders and the stock libraries decode to
the input, of at most cryo_codec_bound() bytes, deterministic, and decoded by the device decoders on every path.  With S
back at 0, for blocks of at most S bytes and for zstd levels the segment encoder does not cover, the output is the
libraries' own again."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc, host

pytestmark = pytest.mark.gpu

SEGS = [4096, 8192, 16384, 32768, 65536, 131072]
LZ4_ACCELS = [0, 1, 7, 50, 65537]
ZSTD_LEVELS = [-5, -1, 1, 2]
DISTS = range(5)  # wide, narrow, int4, random, zeros
# 128 KiB, 1 MiB, and sizes that are not a multiple of S: 512 KiB + 7 leaves every S a last segment of 7 bytes
SIZES = [131072, 1 << 20, (512 << 10) + 7, 300001]


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def seg(codec):
    yield codec
    codec.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)


def _decode_check(oracle, stock, method, comp, raw):
    B = raw.nbytes
    assert len(comp) <= cc.bound(method, B)
    if method == METHOD_LZ4:
        r, out = oracle.lz4_decompress(comp, B, fill=0x5A)
        assert r == B and np.array_equal(out, raw)
        if stock.lz4 is not None:
            r, out = stock.lz4_decompress(comp, B, fill=0x5A)
            assert r == B and np.array_equal(out, raw)
    else:
        r, out = oracle.zstd_decompress(comp, B, fill=0x5A)
        assert r == B and np.array_equal(out, raw)
        if stock.zstd is not None:
            r, out = stock.zstd_decompress(comp, B, fill=0x5A)
            assert r == B and np.array_equal(out, raw)


def test_option_accepted_and_reported(seg):
    assert seg.get_option(cc.OPT_ENCODE_SEGMENT_BYTES) == 0
    for s in SEGS + [0]:
        seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, s)
        assert seg.get_option(cc.OPT_ENCODE_SEGMENT_BYTES) == s
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
    for bad in (-1, 1, 2048, 4095, 12288, 262144, 1 << 20):
        with pytest.raises(cc.CryoError) as e:
            seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, bad)
        assert e.value.code == cc.E_ARG
    assert seg.get_option(cc.OPT_ENCODE_SEGMENT_BYTES) == 16384


@pytest.mark.parametrize("S", SEGS)
@pytest.mark.parametrize("method,params", [(METHOD_LZ4, LZ4_ACCELS), (METHOD_ZSTD, ZSTD_LEVELS)], ids=["lz4", "zstd"])
def test_segment_streams_decode_to_the_input(seg, oracle, stock, S, method, params):
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
    for B in SIZES:
        blocks = [oracle.synth(3, 11, B, d) for d in DISTS]
        for p in params:
            comps = seg.compress_blocks(method, p, blocks)
            for raw, comp in zip(blocks, comps):
                _decode_check(oracle, stock, method, comp, raw)


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_ZSTD, 1)], ids=["lz4", "zstd"])
def test_device_decoders_read_segment_streams(seg, oracle, method, param):
    """every decode path of the device decoders takes the segment streams"""
    B = 1 << 20
    blocks = [oracle.synth(5, i, B, i % 5) for i in range(10)]
    opt, paths = ((cc.OPT_LZ4_DECODE_PATH, (0, 1, 2, 3)) if method == METHOD_LZ4 else (cc.OPT_ZSTD_DECODE_PATH, (0, 1, 2, 3)))
    try:
        for S in (4096, 16384, 131072):
            seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
            comps = seg.compress_blocks(method, param, blocks)
            for path in paths:
                seg.set_option(opt, path)
                outs, st = seg.decompress_blocks(method, comps, B)
                assert (st == 0).all(), (S, path, st)
                for raw, out in zip(blocks, outs):
                    assert np.array_equal(out, raw), (S, path)
    finally:
        seg.set_option(opt, 0)


def _carry_blocks(oracle, B):
    """literal-only segments in front of compressible ones: random bytes, then zeros / `wide`; random to the end but for
    a repeat inside the last segment; random bytes with one earlier stretch repeated far behind"""
    rnd = oracle.synth(9, 1, B, 3)
    wide = oracle.synth(9, 2, B, 0)
    a = rnd.copy(); a[B // 2:] = 0
    b = rnd.copy(); b[B * 3 // 4:] = wide[B * 3 // 4:]
    c = rnd.copy(); c[B - 3000:B - 1000] = rnd[B - 40000:B - 38000]
    d = rnd.copy(); d[B - 20:] = 7
    return [a, b, c, d, rnd]


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_LZ4, 65537), (METHOD_ZSTD, 1)], ids=["lz4", "lz4-a65537", "zstd"])
def test_carry_chains_and_size_bound(seg, oracle, stock, method, param):
    for B in (1 << 20, (256 << 10) + 5):
        blocks = _carry_blocks(oracle, B)
        for S in (4096, 16384):
            seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
            comps = seg.compress_blocks(method, param, blocks)
            for raw, comp in zip(blocks, comps):
                _decode_check(oracle, stock, method, comp, raw)
            assert len(comps[-1]) <= cc.bound(method, B)  # incompressible


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_ZSTD, 1), (METHOD_ZSTD, -5)], ids=["lz4", "zstd", "zstd-5"])
def test_deterministic_alone_or_in_a_batch(seg, oracle, method, param):
    B = 131072
    blocks = [oracle.synth(4, i, B, i % 5) for i in range(64)]
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 8192)
    batch = seg.compress_blocks(method, param, blocks)
    again = seg.compress_blocks(method, param, blocks)
    for x, y in zip(batch, again):
        assert np.array_equal(x, y)
    for i in (0, 1, 2, 3, 4, 37, 63):
        alone = seg.compress_blocks(method, param, [blocks[i]])[0]
        assert np.array_equal(alone, batch[i]), i
        assert np.array_equal(seg.compress_block(method, param, blocks[i]), batch[i]), i


def test_segment_output_differs_from_the_libraries(seg, oracle):
    """the mode does what it says: at S < B the stream is not the library's (else nothing was exercised)"""
    raw = oracle.synth(0, 0, 1 << 20, 0)
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
    assert not np.array_equal(seg.compress_blocks(METHOD_LZ4, 1, [raw])[0], oracle.lz4_compress(raw, 1))
    z = seg.compress_blocks(METHOD_ZSTD, 1, [raw])[0]
    assert not np.array_equal(z, oracle.zstd_compress(raw, 1))
    ident = oracle.zstd_compress(raw, 1)
    assert np.array_equal(z[:6], ident[:6])  # the frame header is the identical path's


def test_identity_where_it_must_hold(seg, oracle):
    blocks128 = [oracle.synth(1, i, 131072, i) for i in range(5)]
    # option back at 0
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 32768)
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
    for comp, raw in zip(seg.compress_blocks(METHOD_LZ4, 1, blocks128), blocks128):
        assert np.array_equal(comp, oracle.lz4_compress(raw, 1))
    for comp, raw in zip(seg.compress_blocks(METHOD_ZSTD, 1, blocks128), blocks128):
        assert np.array_equal(comp, oracle.zstd_compress(raw, 1))
    # blocks of at most S bytes
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 131072)
    for comp, raw in zip(seg.compress_blocks(METHOD_LZ4, 7, blocks128), blocks128):
        assert np.array_equal(comp, oracle.lz4_compress(raw, 7))
    for comp, raw in zip(seg.compress_blocks(METHOD_ZSTD, 2, blocks128), blocks128):
        assert np.array_equal(comp, oracle.zstd_compress(raw, 2))
    small = [oracle.synth(1, i, 4096, i) for i in range(5)]
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 4096)
    for comp, raw in zip(seg.compress_blocks(METHOD_LZ4, 1, small), small):
        assert np.array_equal(comp, oracle.lz4_compress(raw, 1))
    # zstd levels the segment encoder does not cover (dfast and up)
    seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
    for lvl in (3, 5):
        for comp, raw in zip(seg.compress_blocks(METHOD_ZSTD, lvl, blocks128), blocks128):
            assert np.array_equal(comp, oracle.zstd_compress(raw, lvl)), lvl


def test_host_batch_call_and_multi(seg, oracle, stock):
    """the host-buffer K-block call (cryo_codec_compress_blocks) and the multi-GPU form through cryo_multi_set_option"""
    L = cc.lib()
    B, n = 1 << 20, 4
    raw = np.concatenate([oracle.synth(6, i, B, i % 5) for i in range(n)])
    cap = cc.bound(METHOD_LZ4, B)
    for method, param in ((METHOD_LZ4, 1), (METHOD_ZSTD, 1)):
        cap = cc.bound(method, B)
        seg.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
        dst = np.zeros(n * cap, np.uint8)
        sz = (C.c_uint32 * n)()
        assert L.cryo_codec_compress_blocks(seg.h, method, param, raw.ctypes.data, B, n, dst.ctypes.data, cap, sz) == 0
        dev = seg.compress_blocks(method, param, [raw[i * B:(i + 1) * B] for i in range(n)])
        for i in range(n):
            comp = dst[i * cap:i * cap + sz[i]]
            assert np.array_equal(comp, dev[i])
            _decode_check(oracle, stock, method, comp, raw[i * B:(i + 1) * B])
    m = C.c_void_p()
    assert L.cryo_multi_open((C.c_int * 1)(0), 1, C.byref(m)) == 0
    try:
        assert L.cryo_multi_set_option(m, cc.OPT_ENCODE_SEGMENT_BYTES, 16384) == 0
        assert L.cryo_multi_set_option(m, cc.OPT_ENCODE_SEGMENT_BYTES, 3000) == cc.E_ARG
        cap = cc.bound(METHOD_ZSTD, B)
        dst = np.zeros(n * cap, np.uint8)
        sz = (C.c_uint32 * n)()
        assert L.cryo_multi_compress_blocks(m, METHOD_ZSTD, 1, raw.ctypes.data, B, n, dst.ctypes.data, cap, sz) == 0
        for i in range(n):
            comp = dst[i * cap:i * cap + sz[i]]
            assert not np.array_equal(comp, oracle.zstd_compress(raw[i * B:(i + 1) * B], 1))
            _decode_check(oracle, stock, METHOD_ZSTD, comp, raw[i * B:(i + 1) * B])
    finally:
        L.cryo_multi_close(m)


def test_host_layer_guc_writes_chains_stock_libraries_read(oracle, stock):
    """cryo_compress (the access method's write path, one 1 MiB block per call) with pg_cryogen.gpu_encode_segment_kb = 16:
    cryo_decompress and the stock libraries read the pages back"""
    host.use(production=True)
    L = host.lib()
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    B = host.get_block_size()
    try:
        L.cryo_define_compression_gucs()
        host.set_int("cryo_gpu_encode_segment_kb_guc", 16)
        checked = 0
        for dist in range(5):
            raw = oracle.synth(8, dist, B, dist)
            n = C.c_size_t(0)
            for meth, cmeth in ((host.COMP_LZ4, METHOD_LZ4), (host.COMP_ZSTD, METHOD_ZSTD)):
                p = L.cryo_compress(meth, raw.ctypes.data, C.byref(n))
                comp = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n.value,)).copy()
                ident = oracle.lz4_compress(raw, 1) if cmeth == METHOD_LZ4 else oracle.zstd_compress(raw, 1)
                if len(ident) < B // 2:  # (an incompressible block is one literal run either way)
                    assert not np.array_equal(comp, ident), "the GUC did not reach the encoder"
                    checked += 1
                out = np.zeros(B, np.uint8)
                assert L.cryo_decompress(meth, comp.ctypes.data, len(comp), out.ctypes.data) is True
                assert np.array_equal(out, raw)
                _decode_check(oracle, stock, cmeth, comp, raw)
        assert not errors and checked >= 4
    finally:
        host.set_int("cryo_gpu_encode_segment_kb_guc", 0)
        L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
        host.use(production=None)
