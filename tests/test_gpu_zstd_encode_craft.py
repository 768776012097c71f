"""GPU: the zstd encoders, every level, on matches placed at the edges of their 64-lane strides (tests/zstd_enc_craft.py).

The encoders share a scalar algorithm's steps across a wave: candidates grow 64 bytes at a time, hash tables are caught up
64 positions at a time, the price ladder and the histograms take 64 entries at a time.  The suite's other encode inputs draw
their lengths at random; these put a match length, a literal run, a distance and the distance to the block's end on 63, 64,
65, multiples of 64, one past each targetLength and around kOptNum, alone and combined, at 4096, 1024 and 1025 bytes
(ZSTD_PREDEF_THRESHOLD) and, for matches around kOptNum, 16 384.  Frames of several 128 KiB zstd blocks that differ in kind
carry repeat offsets, entropy tables and the optimal parser's statistics across raw, RLE and compressed blocks.

Bar: every frame equals the oracle's, byte for byte; tests/test_zstd_encode_craft_cpu.py pins the oracle to libzstd 1.4.8 on
these very inputs and shows that no input hides its sequences in a raw block.  The same lists go once through write
verification, checksummed frames, the host-buffer call and both device decoders."""
import numpy as np
import pytest

import oracle_lib
import zstd_enc_craft as zc
from pg_cryogen_amd import METHOD_ZSTD, codec as cc
from test_gpu_zstd_checksum import expected as checksummed

pytestmark = pytest.mark.gpu

LEVELS = [-5, -1] + list(range(1, 23))
ROUTE_LEVELS = (3, 9, 13, 22)                   # dfast, lazy2, btlazy2 and btultra2 at these sizes
SIZES = zc.SWEEP_SIZES + (zc.LONG_B,)
DECODE_LEVELS = (1, 22)
STOCK_FROM = 11                                 # where the stock library loads it is compared too, from this level up

_refs = {}
_device = {}                                    # (B, level): the device's frames, kept by the sweep test for the decoders


def ref(oracle, B, level):
    """the oracle's frames of a block size's cases at a level: computed once, shared, never written to"""
    key = (B, level)
    if key not in _refs:
        frames = [oracle.zstd_compress(b, level) for b in zc.blocks(B)[1]]
        for f in frames:
            f.setflags(write=False)
        _refs[key] = frames
    return _refs[key]


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def zcodec(codec):
    yield codec
    for opt, v in ((cc.OPT_ENCODE_VERIFY, 0), (cc.OPT_ZSTD_CHECKSUM, 0), (cc.OPT_ZSTD_DECODE_PATH, 0),
                   (cc.OPT_ENCODE_SEGMENT_BYTES, 0), (cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 1)):
        codec.set_option(opt, v)


def mismatches(B, level, got, want):
    """[(B, level, L, D, R, tail, bytes written, bytes expected)] of the blocks that differ"""
    cases = zc.blocks(B)[0]
    assert len(got) == len(want) == len(cases)
    return [(B, level) + c + (len(g), len(w)) for c, g, w in zip(cases, got, want) if not np.array_equal(g, w)]


def check(B, level, got, want, what=""):
    bad = mismatches(B, level, got, want)
    assert bad == [], "%s%d of %d blocks differ; (B, level, L, D, R, tail, written, expected): %s" % (
        what, len(bad), len(got), bad[:12])


# ---------------- the sweep and long-match lists ----------------
@pytest.mark.parametrize("level", LEVELS)
def test_sweep_and_long_matches_bit_exact(zcodec, oracle, stock, level):
    """one call per block size with all its cases as the batch"""
    for B in SIZES:
        blocks = zc.blocks(B)[1]
        got = zcodec.compress_blocks(METHOD_ZSTD, level, blocks)
        if level in DECODE_LEVELS:
            _device[B, level] = got
        check(B, level, got, ref(oracle, B, level))
        if stock.zstd is not None and level >= STOCK_FROM:
            check(B, level, got, [stock.zstd_compress(b, level) for b in blocks], "libzstd: ")


# ---------------- frames of several zstd blocks ----------------
@pytest.mark.parametrize("level", zc.MIXED_LEVELS)
@pytest.mark.parametrize("B", sorted(zc.mixed_by_size()))
def test_mixed_frames_bit_exact(zcodec, oracle, stock, B, level):
    """grouped by size: a call takes equal sizes (the optimal parser needs seconds for a frame of three blocks, so a size is
    a case of its own)"""
    group = zc.mixed_by_size()[B]
    got = zcodec.compress_blocks(METHOD_ZSTD, level, [a for _, a in group])
    for (name, a), g in zip(group, got):
        w = oracle.zstd_compress(a, level)
        assert np.array_equal(g, w), (name, B, level, len(g), len(w))
        if stock.zstd is not None and level >= STOCK_FROM:
            assert np.array_equal(g, stock.zstd_compress(a, level)), ("libzstd", name, B, level)


# ---------------- other routes, once ----------------
def test_write_verification_refuses_no_block(zcodec, oracle):
    """CRYO_OPT_ENCODE_VERIFY = 1: the same bytes, every status OK (compress_blocks raises on any other)"""
    zcodec.set_option(cc.OPT_ENCODE_VERIFY, 1)
    for level in ROUTE_LEVELS:
        for B in zc.SWEEP_SIZES:
            got = zcodec.compress_blocks(METHOD_ZSTD, level, zc.blocks(B)[1])
            check(B, level, got, ref(oracle, B, level), "verified: ")
    assert zcodec.last_verify_failure() is None


def test_checksummed_frames(zcodec, oracle, stock):
    """CRYO_OPT_ZSTD_CHECKSUM = 1: libzstd's frames under ZSTD_c_checksumFlag (without the library: the oracle's frame with
    the flag set and XXH64's low 32 bits behind it)"""
    zcodec.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    for level in ROUTE_LEVELS:
        for B in zc.SWEEP_SIZES:
            blocks = zc.blocks(B)[1]
            got = zcodec.compress_blocks(METHOD_ZSTD, level, blocks)
            check(B, level, got, [checksummed(stock, oracle, b, level) for b in blocks], "checksummed: ")


def test_host_buffer_call(zcodec, oracle):
    """cryo_codec_compress_blocks: host buffers both ways, a padded destination stride"""
    for level in ROUTE_LEVELS:
        for B in zc.SWEEP_SIZES:
            blocks = zc.blocks(B)[1]
            n = len(blocks)
            raw = np.concatenate(blocks)
            stride = cc.bound(METHOD_ZSTD, B) + 40
            out = np.zeros(n * stride, np.uint8)
            sizes = np.zeros(n, np.uint32)
            rc = zcodec.L.cryo_codec_compress_blocks(zcodec.h, METHOD_ZSTD, level, raw.ctypes.data, B, n, out.ctypes.data,
                                                     stride, sizes.ctypes.data)
            assert rc == 0, (B, level, rc)
            got = [out[i * stride:i * stride + int(sizes[i])] for i in range(n)]
            check(B, level, got, ref(oracle, B, level), "host buffers: ")


# ---------------- decode ----------------
@pytest.mark.parametrize("path", [1, 2], ids=["fused", "pipeline"])
def test_device_decoders_read_the_frames(zcodec, path):
    """the device's own frames of levels 1 and 22, every block size: a handful of sequences over kilobytes of Huffman literals
    is unusual decoder input"""
    for level in DECODE_LEVELS:
        for B in SIZES:
            cases, blocks = zc.blocks(B)
            if (B, level) not in _device:       # run on its own: encode them here
                _device[B, level] = zcodec.compress_blocks(METHOD_ZSTD, level, blocks)
            zcodec.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
            outs, st = zcodec.decompress_blocks(METHOD_ZSTD, _device[B, level], B)
            assert (st == 0).all(), (path, B, level, [c for c, s in zip(cases, st) if s != 0][:12])
            bad = [c for c, o, b in zip(cases, outs, blocks) if not np.array_equal(o, b)]
            assert bad == [], (path, B, level, len(bad), bad[:12])
