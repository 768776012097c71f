"""GPU: the zstd encoders' entropy stage on frames whose literals and sequences are dictated (tests/zstd_entropy_craft.py).

The second half of zstd_enc.hip -- Huffman and FSE table building, the literal section, the sequence bitstream, the tables
carried from block to block -- has wave geometry the scalar oracle does not have: Huffman streams split over 64 lanes and
packed by a bit-offset scan, the literal histogram and copy in rounds of 4096 and 1024 bytes and a tail, sequence batches of
64 with a partial dword carried from batch to batch, writes suppressed once the stream has outgrown its block.  The frames
here put literal counts, stream lengths, sequence counts, table modes and code histograms on those edges on purpose;
tests/test_zstd_entropy_craft_cpu.py proves on the CPU, from the oracle's branch counters and the frames' headers, that every
named property is reached at a level of every strategy class, and pins the oracle to libzstd 1.4.8 on these inputs.

Bar: every frame equals the oracle's, byte for byte, at one level per strategy and one negative level (the levels come from
the oracle's parameter table, by frame size; the optimal parsers get the shorter list that still reaches every property of
theirs, zstd_entropy_craft.OPT_CASES, and its chains of several dictated blocks at btultra alone); from level 11 up it equals libzstd's too where the library
loads.  The list goes once, at one level per strategy class, through write verification, checksummed frames, the host-buffer call (whose
padding beyond the bound must stay untouched, also behind blocks that end raw because their sequence stream outgrew them)
and both device decoders (these read the chains at btultra too), which read RLE literals, treeless literals and repeat tables out of our own encoder here."""
import numpy as np
import pytest

import oracle_lib
import zstd_entropy_craft as ze
from pg_cryogen_amd import METHOD_ZSTD, codec as cc
from test_gpu_zstd_checksum import expected as checksummed

pytestmark = pytest.mark.gpu

STRATEGIES = ("negative", "fast", "dfast", "greedy", "lazy", "lazy2", "btlazy2", "btopt", "btultra", "btultra2")
ROUTE_STRATEGIES = ("greedy", "btlazy2", "btultra2")        # one per class: below lazy | lazy to btopt | btultra, btultra2
STOCK_FROM = 11                                 # as tests/test_gpu_zstd_encode_craft.py: libzstd is compared from this level up
PATTERN = 0xC3

_refs = {}
_device = {}                                    # (size, level): the device's frames, kept by the sweep for the decoders


def level_of(oracle, size, strategy):
    """the level zstd_entropy_craft.levels() gives a strategy at a frame size"""
    lv = ze.levels(oracle, size)
    if strategy == "negative":
        return min(lv)
    return next(level for level, s in lv.items() if level > 0 and s == STRATEGIES.index(strategy))


def groups(strategy, part=None):
    """[(frame size, [Case])] of the list a strategy gets: all of it, or of the optimal parsers' shorter one the frames of one
    dictated block (the chains of several go through test_chains_at_btultra)"""
    st = max(STRATEGIES.index(strategy), 1)
    return sorted(ze.by_size(st, part or ("all" if st < ze.OPT_STRATEGY else "single")).items())


def ref(oracle, cases, size, level):
    """the oracle's frames of a size's cases at a level: computed once, shared, never written to"""
    key = (size, level)
    if key not in _refs:
        frames = [oracle.zstd_compress(c.frame, level) for c in cases]
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
    for opt, v in ((cc.OPT_ENCODE_VERIFY, 0), (cc.OPT_ZSTD_CHECKSUM, 0), (cc.OPT_ZSTD_DECODE_PATH, 0)):
        codec.set_option(opt, v)


def check(cases, size, level, got, want, what=""):
    assert len(got) == len(want) == len(cases)
    bad = [(c.name, len(g), len(w)) for c, g, w in zip(cases, got, want) if not np.array_equal(g, w)]
    assert bad == [], "%s%d of %d frames of %d bytes differ at level %d; (case, written, expected): %s" % (
        what, len(bad), len(got), size, level, bad[:12])


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_dictated_frames_bit_exact(zcodec, oracle, stock, strategy):
    """one call per frame size with all its cases as the batch"""
    for size, cases in groups(strategy):
        level = level_of(oracle, size, strategy)
        got = zcodec.compress_blocks(METHOD_ZSTD, level, [c.frame for c in cases])
        if strategy in ROUTE_STRATEGIES:
            _device[size, level] = got
        check(cases, size, level, got, ref(oracle, cases, size, level))
        if stock.zstd is not None and level >= STOCK_FROM:
            check(cases, size, level, got, [stock.zstd_compress(c.frame, level) for c in cases], "libzstd: ")


def test_chains_at_btultra(zcodec, oracle, stock):
    """the optimal parsers' frames of several dictated blocks: tables carried from block to block under the other minGain"""
    for size, cases in groups("btultra", "chains"):
        level = level_of(oracle, size, "btultra")
        got = zcodec.compress_blocks(METHOD_ZSTD, level, [c.frame for c in cases])
        _device[size, level] = got
        check(cases, size, level, got, ref(oracle, cases, size, level))
        if stock.zstd is not None and level >= STOCK_FROM:
            check(cases, size, level, got, [stock.zstd_compress(c.frame, level) for c in cases], "libzstd: ")


def test_write_verification_refuses_no_block(zcodec, oracle):
    """CRYO_OPT_ENCODE_VERIFY = 1: the same bytes, every status OK (compress_blocks raises on any other)"""
    zcodec.set_option(cc.OPT_ENCODE_VERIFY, 1)
    for strategy in ROUTE_STRATEGIES:
        for size, cases in groups(strategy):
            level = level_of(oracle, size, strategy)
            got = zcodec.compress_blocks(METHOD_ZSTD, level, [c.frame for c in cases])
            check(cases, size, level, got, ref(oracle, cases, size, level), "verified: ")
    assert zcodec.last_verify_failure() is None


def test_checksummed_frames(zcodec, oracle, stock):
    """CRYO_OPT_ZSTD_CHECKSUM = 1: libzstd's frames under ZSTD_c_checksumFlag (without the library: the oracle's frame with
    the flag set and XXH64's low 32 bits behind it)"""
    zcodec.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    for strategy in ROUTE_STRATEGIES:
        for size, cases in groups(strategy):
            level = level_of(oracle, size, strategy)
            got = zcodec.compress_blocks(METHOD_ZSTD, level, [c.frame for c in cases])
            check(cases, size, level, got, [checksummed(stock, oracle, c.frame, level) for c in cases], "checksummed: ")


def test_host_buffer_call_leaves_the_padding_alone(zcodec, oracle):
    """cryo_codec_compress_blocks: host buffers both ways, a padded destination stride filled with a pattern first.  Behind
    every slot's bound the pattern still stands, also where a block ended raw because its sequence stream outgrew it."""
    for strategy in ROUTE_STRATEGIES:
        for size, cases in groups(strategy):
            level = level_of(oracle, size, strategy)
            n = len(cases)
            raw = np.concatenate([c.frame for c in cases])
            bound = cc.bound(METHOD_ZSTD, size)
            stride = bound + 40
            out = np.full(n * stride, PATTERN, np.uint8)
            sizes = np.zeros(n, np.uint32)
            rc = zcodec.L.cryo_codec_compress_blocks(zcodec.h, METHOD_ZSTD, level, raw.ctypes.data, size, n, out.ctypes.data,
                                                     stride, sizes.ctypes.data)
            assert rc == 0, (size, level, rc)
            got = [out[i * stride:i * stride + int(sizes[i])] for i in range(n)]
            check(cases, size, level, got, ref(oracle, cases, size, level), "host buffers: ")
            pad = out.reshape(n, stride)[:, bound:]
            touched = [c.name for c, row in zip(cases, pad) if (row != PATTERN).any()]
            assert touched == [], (size, level, touched[:12])


@pytest.mark.parametrize("path", [1, 2], ids=["fused", "pipeline"])
def test_device_decoders_read_the_frames(zcodec, oracle, path):
    """the device's own frames back to the input: the list at one strategy per class, and the optimal parsers' chains of
    several dictated blocks (tables carried from block to block under the other minGain) at btultra"""
    for strategy, part in [(s, None) for s in ROUTE_STRATEGIES] + [("btultra", "chains")]:
        for size, cases in groups(strategy, part):
            level = level_of(oracle, size, strategy)
            if (size, level) not in _device:    # run on its own: encode them here
                _device[size, level] = zcodec.compress_blocks(METHOD_ZSTD, level, [c.frame for c in cases])
            zcodec.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
            outs, st = zcodec.decompress_blocks(METHOD_ZSTD, _device[size, level], size)
            assert (st == 0).all(), (path, size, level, [c.name for c, s in zip(cases, st) if s != 0][:12])
            bad = [c.name for c, o in zip(cases, outs) if not np.array_equal(o, c.frame)]
            assert bad == [], (path, size, level, len(bad), bad[:12])
