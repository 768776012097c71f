"""GPU tests of segment-parallel zstd encode for the strategies above `fast` (CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY;
pg_cryogen.gpu_encode_segment_zstd_strategy).

With CRYO_OPT_ENCODE_SEGMENT_BYTES = S and the strategy option at m, a zstd level whose strategy is at most m (2 dfast,
3 greedy, 4 lazy, 5 lazy2, 6 btlazy2) encodes a block of more than S bytes as ceil(B / S) zstd blocks, one wave each.
The frame is not libzstd's own, but it must decode to the input in the pinned oracle, in stock libzstd and on every
device decode path, fit cryo_codec_bound(), keep the identical path's frame header and come out the same whatever the
call.  Levels above m, the optimal parsers, S = 0 and blocks of at most S bytes keep libzstd's bytes.

The file uses a handle of its own, so that the options it sets never reach the session handle of the other files."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import zstd_craft
from pg_cryogen_amd import METHOD_ZSTD, Codec, codec as cc

pytestmark = pytest.mark.gpu

KIB = 1024
MIB = 1 << 20
SIZES = [128 * KIB, MIB, 512 * KIB + 7, 300001]
DISTS = range(5)  # wide, narrow, int4, random, zeros
# one level per (strategy, block size), from zstd_fast_cparams (libzstd 1.4.8's ZSTD_defaultCParameters): the table for
# sources above 256 KiB (1 MiB, 512 KiB + 7, 300 001) has dfast at 3, greedy at 5, lazy at 7, lazy2 at 9, btlazy2 at 13;
# the table for 16 .. 128 KiB has dfast at 3, greedy at 5, lazy at 6, lazy2 at 8, btlazy2 at 11
LEVELS = {2: (3, 3), 3: (5, 5), 4: (7, 6), 5: (9, 8), 6: (13, 11)}  # strategy: (level above 256 KiB, level at 128 KiB)


def level_for(strategy, B):
    return LEVELS[strategy][0 if B > 256 * KIB else 1]


@pytest.fixture(scope="module")
def zc():
    c = Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


def _set(c, S, strategy):
    c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
    c.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, strategy)


def _decode_check(oracle, stock, comp, raw):
    B = raw.nbytes
    assert len(comp) <= cc.bound(METHOD_ZSTD, B)
    r, out = oracle.zstd_decompress(comp, B, fill=0x5A)
    assert r == B and np.array_equal(out, raw)
    if stock.zstd is not None:
        r, out = stock.zstd_decompress(comp, B, fill=0x5A)
        assert r == B and np.array_equal(out, raw)


def _head_len(b):
    """bytes of a zstd frame header (RFC 8878 3.1.1.1), as zstd_craft.walk() reads them"""
    fhd = b[4]
    single = (fhd >> 5) & 1
    return 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]


def test_option_accepted_and_reported(zc):
    assert zc.get_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY) == 1
    for m in (1, 2, 3, 4, 5, 6):
        zc.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, m)
        assert zc.get_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY) == m
    zc.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 4)
    for bad in (0, 7, 8, 9, -1):
        with pytest.raises(cc.CryoError) as e:
            zc.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, bad)
        assert e.value.code == cc.E_ARG
    assert zc.get_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY) == 4
    zc.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 1)


@pytest.mark.parametrize("strategy", [2, 3, 4, 5, 6], ids=["dfast", "greedy", "lazy", "lazy2", "btlazy2"])
def test_round_trip_and_frame_shape(zc, oracle, stock, strategy):
    """every dist at S = 16 KiB, one dist (in turn) at the other S; every size"""
    try:
        for B in SIZES:
            lvl = level_for(strategy, B)
            blocks = [oracle.synth(21, strategy * 10 + d, B, d) for d in DISTS]
            for k, S in enumerate((4 * KIB, 16 * KIB, 32 * KIB, 64 * KIB)):
                todo = list(DISTS) if S == 16 * KIB else [(k + strategy) % 5]
                _set(zc, S, strategy)
                comps = zc.compress_blocks(METHOD_ZSTD, lvl, [blocks[d] for d in todo])
                for d, comp in zip(todo, comps):
                    raw = blocks[d]
                    _decode_check(oracle, stock, comp, raw)
                    info = zstd_craft.walk(comp)
                    assert info is not None and len(info["blocks"]) == -(-B // S), (B, S, d)
                    if S == 16 * KIB:
                        ident = oracle.zstd_compress(raw, lvl)
                        assert not np.array_equal(comp, ident), (B, d)
                        h = _head_len(ident)
                        assert _head_len(comp) == h and np.array_equal(comp[:h], ident[:h]), (B, d)
    finally:
        _set(zc, 0, 1)


@pytest.mark.parametrize("strategy", [2, 4, 6], ids=["dfast", "lazy", "btlazy2"])
def test_device_decoders_read_the_frames(zc, oracle, strategy):
    """zstd decode paths 0 .. 3 of CRYO_OPT_ZSTD_DECODE_PATH at 1, 64 and 320 frames"""
    B = 128 * KIB
    lvl = level_for(strategy, B)
    uniq = [oracle.synth(22, i, B, i % 5) for i in range(10)]
    try:
        _set(zc, 16 * KIB, strategy)
        ucomp = zc.compress_blocks(METHOD_ZSTD, lvl, uniq)
        for n in (1, 64, 320):
            comps = [ucomp[i % 10] for i in range(n)]
            for path in (0, 1, 2, 3):
                zc.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
                outs, st = zc.decompress_blocks(METHOD_ZSTD, comps, B)
                assert (st == 0).all(), (n, path, st)
                for i, out in enumerate(outs):
                    assert np.array_equal(out, uniq[i % 10]), (n, path, i)
    finally:
        zc.set_option(cc.OPT_ZSTD_DECODE_PATH, 0)
        _set(zc, 0, 1)


@pytest.mark.parametrize("strategy", [2, 3, 6], ids=["dfast", "greedy", "btlazy2"])
def test_deterministic_whatever_the_call(zc, oracle, strategy):
    """alone, in a batch, compress_batch on device buffers, compress_blocks (host buffers) and a two-handle cryo_multi"""
    B, n, S = MIB, 6, 16 * KIB
    lvl = level_for(strategy, B)
    blocks = [oracle.synth(23, i, B, i % 5) for i in range(n)]
    L = cc.lib()
    try:
        _set(zc, S, strategy)
        batch = zc.compress_blocks(METHOD_ZSTD, lvl, blocks)
        for i in (0, 2, 5):
            assert np.array_equal(zc.compress_blocks(METHOD_ZSTD, lvl, [blocks[i]])[0], batch[i]), i
            assert np.array_equal(zc.compress_block(METHOD_ZSTD, lvl, blocks[i]), batch[i]), i
        cap = cc.bound(METHOD_ZSTD, B)
        raw = np.concatenate(blocks)
        d_src, d_dst, d_sz, d_st = zc.alloc(n * B), zc.alloc(n * cap), zc.alloc(4 * n), zc.alloc(4 * n)
        try:
            d_src.upload(raw)
            zc.compress_batch(METHOD_ZSTD, lvl, d_src, B, B, n, d_dst, cap, d_sz, d_st)
            zc.sync()
            assert (d_st.download(dtype=np.int32) == 0).all()
            sz = d_sz.download(dtype=np.uint32)
            out = d_dst.download()
            for i in range(n):
                assert np.array_equal(out[i * cap:i * cap + int(sz[i])], batch[i]), i
        finally:
            for b in (d_src, d_dst, d_sz, d_st):
                b.free()
        dst = np.zeros(n * cap, np.uint8)
        sizes = (C.c_uint32 * n)()
        assert L.cryo_codec_compress_blocks(zc.h, METHOD_ZSTD, lvl, raw.ctypes.data, B, n, dst.ctypes.data, cap, sizes) == 0
        for i in range(n):
            assert np.array_equal(dst[i * cap:i * cap + sizes[i]], batch[i]), i
        m = C.c_void_p()
        assert L.cryo_multi_open((C.c_int * 2)(0, 0), 2, C.byref(m)) == 0
        try:
            assert L.cryo_multi_set_option(m, cc.OPT_ENCODE_SEGMENT_BYTES, S) == 0
            assert L.cryo_multi_set_option(m, cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, strategy) == 0
            assert L.cryo_multi_set_option(m, cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 7) == cc.E_ARG
            dst[:] = 0
            assert L.cryo_multi_compress_blocks(m, METHOD_ZSTD, lvl, raw.ctypes.data, B, n, dst.ctypes.data, cap, sizes) == 0
            for i in range(n):  # block i went to handle i mod 2: both took the option
                assert np.array_equal(dst[i * cap:i * cap + sizes[i]], batch[i]), i
        finally:
            L.cryo_multi_close(m)
    finally:
        _set(zc, 0, 1)


def test_identity_where_it_must_hold(zc, oracle):
    big = [oracle.synth(24, i, MIB, i) for i in range(5)]
    small = [oracle.synth(24, 10 + i, 128 * KIB, i) for i in range(5)]

    def same(level, blocks):
        for comp, raw in zip(zc.compress_blocks(METHOD_ZSTD, level, blocks), blocks):
            assert np.array_equal(comp, oracle.zstd_compress(raw, level)), level
    try:
        # S = 0 with the strategy option at its highest
        _set(zc, 0, 6)
        same(3, small)
        same(11, small)
        # a level whose strategy lies above the option: option dfast, levels 5 (greedy) and 9 (lazy2) at 1 MiB
        _set(zc, 16 * KIB, 2)
        same(5, big)
        same(9, big)
        # the optimal parsers stay out: btopt at 16 (1 MiB) and 13 (128 KiB) with the option at btlazy2
        _set(zc, 16 * KIB, 6)
        same(16, big[:2])
        same(13, small)
        # blocks of at most S bytes
        _set(zc, 128 * KIB, 6)
        same(5, small)
        same(11, small)
    finally:
        _set(zc, 0, 1)


def test_size_bound_on_wide(zc, oracle):
    """loose: at most 1.25x the identical path's size on `wide` rows (the tight figures are in the profile)"""
    B, S = MIB, 16 * KIB
    raws = [oracle.synth(25, i, B, 0) for i in range(2)]
    try:
        for strategy in (2, 3, 4, 5, 6):
            lvl = level_for(strategy, B)
            _set(zc, S, strategy)
            seg = sum(len(c) for c in zc.compress_blocks(METHOD_ZSTD, lvl, raws))
            ident = sum(len(oracle.zstd_compress(r, lvl)) for r in raws)
            assert seg <= 1.25 * ident, (strategy, seg, ident)
    finally:
        _set(zc, 0, 1)
