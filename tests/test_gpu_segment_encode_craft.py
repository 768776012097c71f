"""GPU: segment-parallel encode (CRYO_OPT_ENCODE_SEGMENT_BYTES = S, CRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY) on blocks
crafted around the segment boundaries s0 = k * S (tests/seg_craft.py), at sizes up to 16 MiB.

LZ4: every stream decodes to the input in the oracle and liblz4, keeps the block format (tests/seg_craft.lz4_walk) and the
segment rule that a match starting in an interior segment ends by its end, fits cryo_codec_bound(), is the same alone and
in a batch, and stays small on periodic data (the seeded table finds the earlier segments).  Blocks of 1 MiB + 1 to 16 MiB
run the segment kernel with tag planes and 8 high position bits; 16 MiB + 1 falls back to the identical path.

zstd, `fast` to `btlazy2` and level -5: the frame decodes in the oracle and libzstd, has ceil(B / S) blocks with fresh
tables (no treeless literals, no Repeat-mode tables) behind the identical path's header, and every segment block decodes
on its own behind raw-block history (independence) and behind only the W + S bytes before it (reach).

The device decoders read a sample of the streams on every route.  The file uses a handle of its own, so that the options
it sets never reach the session handle of the other files."""
import numpy as np
import pytest

import oracle_lib
import seg_craft as sc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, Codec, codec as cc

pytestmark = pytest.mark.gpu

KIB, MIB = 1024, 1 << 20
SEED = 11
LZ4_SEGS = [4096, 16384, 131072]
LZ4_ACCELS = [1, 2, 7, 64, 65537]
SHORT_TAILS = [1, 4, 5, 6, 7, 8, 11, 12, 13]      # B = m * S + r: a last segment of r bytes


@pytest.fixture(scope="module")
def c():
    h = Codec(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def stock():
    s = oracle_lib.StockLibs()
    if s.lz4 is None or s.zstd is None:
        pytest.fail("liblz4.so.1 and libzstd.so.1 are needed")
    return s


def _set(c, S, strategy=1):
    c.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
    c.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, strategy)


@pytest.fixture(autouse=True)
def _reset(c):
    yield
    _set(c, 0, 1)


def _lz4_check(oracle, stock, comp, raw, S, tag):
    B = raw.nbytes
    assert len(comp) <= cc.bound(METHOD_LZ4, B), tag
    for dec in (oracle.lz4_decompress, stock.lz4_decompress):
        r, out = dec(comp, B, fill=0x5A)
        assert r == B and np.array_equal(out, raw), tag
    try:
        seqs = sc.lz4_walk(comp, B)
    except sc.LZ4FormatError as e:
        raise AssertionError((tag, str(e)))
    sc.lz4_segment_checks(seqs, B, S)


def _effective(name, comp, B, S, lz4):
    """periodic blocks stay small (LZ4: at acceleration 1; from 7 up the search starts with a step of the acceleration and
    skips periods for any encoder)"""
    if name.startswith("periodic/"):
        P = int(name.split("/")[1])
        bound = sc.effectiveness_bound(P, B, S, lz4)
        assert len(comp) <= bound, (name, B, S, len(comp), bound)


def _lz4_run(c, oracle, stock, B, S, accels, cap=64, mixed=True):
    corpus = sc.segment_corpus(B, S, SEED, W=sc.LZ4_SEED, cap=cap)
    names, blocks = [n for n, _ in corpus], [a for _, a in corpus]
    _set(c, S)
    for accel in accels:
        comps = c.compress_blocks(METHOD_LZ4, accel, blocks)
        for name, raw, comp in zip(names, blocks, comps):
            tag = (B, S, accel, name)
            _lz4_check(oracle, stock, comp, raw, S, tag)
            if accel == 1:
                _effective(name, comp, B, S, lz4=True)
        if mixed:
            for i in (0, len(blocks) // 2, len(blocks) - 1):
                assert np.array_equal(c.compress_blocks(METHOD_LZ4, accel, [blocks[i]])[0], comps[i]), (B, S, accel, names[i])
    return names, blocks


# ---------------- LZ4 ----------------
@pytest.mark.parametrize("S", LZ4_SEGS)
def test_lz4_boundaries_up_to_1mib(c, oracle, stock, S):
    """S + 1, 2S - 1, 2S + 1, 1 MiB and last segments of 1 .. 13 bytes, every acceleration"""
    sizes = [S + 1, 2 * S - 1, 2 * S + 1, MIB] + [3 * S + r for r in SHORT_TAILS]
    for B in sizes:
        _lz4_run(c, oracle, stock, B, S, LZ4_ACCELS, mixed=B in (2 * S + 1, MIB))


@pytest.mark.parametrize("S", LZ4_SEGS)
def test_lz4_blocks_above_1mib(c, oracle, stock, S):
    """1 MiB + 1, 2 MiB + 5 and 4 MiB: the segment kernel with tag planes and 8 high position bits (k_lz4_enc2<2048, 8,
    true, true>), seeding through tab_put with tags"""
    for B in (MIB + 1, 2 * MIB + 5, 4 * MIB):
        _lz4_run(c, oracle, stock, B, S, (1, 7, 65537), mixed=B == 2 * MIB + 5)


@pytest.mark.parametrize("S", [16384, 131072])
def test_lz4_16mib(c, oracle, stock, S):
    """exactly 16 MiB (the largest block the segment path takes): a sample of 64 boundaries"""
    _lz4_run(c, oracle, stock, 16 * MIB, S, (1,), cap=64, mixed=False)


def test_lz4_above_16mib_keeps_the_identical_path(c, oracle):
    B = 16 * MIB + 1
    corpus = dict(sc.segment_corpus(B, 16384, SEED, cap=16))
    blocks = [corpus["straddle/0"], corpus["periodic/1000"]]
    _set(c, 16384)
    for raw, comp in zip(blocks, c.compress_blocks(METHOD_LZ4, 1, blocks)):
        assert np.array_equal(comp, oracle.lz4_compress(raw, 1))


# ---------------- zstd ----------------
ZSTD_SEGS = [4096, 16384]


def _zstd_sizes(S):
    return sorted({S + 1, 2 * S, 16 * KIB + 1, 128 * KIB + 1, 256 * KIB + 1, MIB, 2 * MIB + 5} - {B for B in range(S + 1)})


# the blocks the (slower) independence and reach checks walk
DEEP_CHECK = ("straddle/0", "straddle/1", "reps/default_trap", "reps/same_offset", "reps/alternate", "carry/thresholds",
              "periodic/1000")


@pytest.mark.parametrize("strategy", [0, 1, 2, 3, 4, 5, 6], ids=["l-5", "fast", "dfast", "greedy", "lazy", "lazy2", "btlazy2"])
@pytest.mark.parametrize("S", ZSTD_SEGS)
def test_zstd_boundaries(c, oracle, stock, S, strategy):
    """round trip (oracle and libzstd), structure, independence, reach, bound and effectiveness; at S = 4 KiB the sizes
    S + 1 and 2S have a window of 8 KiB, where zstd_seg_cparams clamps W to the window minus S"""
    decoders = [oracle.zstd_decompress, stock.zstd_decompress]
    for B in _zstd_sizes(S):
        level = -5 if strategy == 0 else sc.zstd_levels(stock, B)[strategy]
        wlog, strat = sc.zstd_cparams(stock, level, B)
        assert strat == max(strategy, 1)
        W = sc.zstd_seed_window(strat, wlog, S)
        corpus = sc.segment_corpus(B, S, SEED, W=W, cap=48)
        names, blocks = [n for n, _ in corpus], [a for _, a in corpus]
        ident_head = stock.zstd_compress(np.zeros(B, np.uint8), level)  # the identical path's header: libzstd's
        _set(c, S, max(strategy, 1))
        comps = c.compress_blocks(METHOD_ZSTD, level, blocks)
        for name, raw, comp in zip(names, blocks, comps):
            tag = (B, S, level, name)
            assert len(comp) <= cc.bound(METHOD_ZSTD, B), tag
            for dec in decoders:
                r, out = dec(comp, B, fill=0x5A)
                assert r == B and np.array_equal(out, raw), tag
            sc.zstd_structure_checks(comp, ident_head, B, S)
            _effective(name, comp, B, S, lz4=False)
            if name in DEEP_CHECK:
                ks = sc.segment_sample(-(-B // S), SEED, cap=12)
                assert sc.zstd_independence_failures(comp, raw, S, decoders, ks) == [], tag
                assert sc.zstd_reach_failures(comp, raw, S, W, decoders, ks) == [], (tag, W)


# ---------------- device decoders ----------------
def test_device_decoders_read_crafted_segment_streams(c, oracle):
    """LZ4 ring, indexed, few-blocks and automatic routes; zstd paths 0 .. 3"""
    lz4_paths = [(cc.LZ4_PATH_RING, 0), (cc.LZ4_PATH_INDEXED, 1), (cc.LZ4_PATH_INDEXED, 8), (cc.LZ4_PATH_FEW_BLOCKS, 0),
                 (cc.LZ4_PATH_AUTO, 0)]
    sets = []
    for B, S, accel in ((MIB, 4096, 1), (MIB, 131072, 65537), (2 * 16384 + 1, 16384, 7), (3 * 4096 + 5, 4096, 1)):
        blocks = [a for _, a in sc.segment_corpus(B, S, SEED, W=sc.LZ4_SEED)]
        _set(c, S)
        sets.append((METHOD_LZ4, B, blocks, c.compress_blocks(METHOD_LZ4, accel, blocks)))
    for B, S, level, strategy in ((MIB, 4096, 1, 1), (MIB, 16384, 13, 6), (128 * KIB + 1, 4096, 5, 3), (8192, 4096, 3, 2)):
        blocks = [a for _, a in sc.segment_corpus(B, S, SEED)]
        _set(c, S, strategy)
        sets.append((METHOD_ZSTD, B, blocks, c.compress_blocks(METHOD_ZSTD, level, blocks)))
    _set(c, 0, 1)
    saved = {k: c.get_option(k) for k in (cc.OPT_LZ4_DECODE_PATH, cc.OPT_LZ4_INDEX_WALKERS, cc.OPT_ZSTD_DECODE_PATH)}
    try:
        for method, B, blocks, comps in sets:
            routes = lz4_paths if method == METHOD_LZ4 else [(p, None) for p in (0, 1, 2, 3)]
            for path, walkers in routes:
                if method == METHOD_LZ4:
                    c.set_option(cc.OPT_LZ4_DECODE_PATH, path)
                    c.set_option(cc.OPT_LZ4_INDEX_WALKERS, walkers)
                else:
                    c.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
                outs, st = c.decompress_blocks(method, comps, B)
                assert (st == 0).all(), (method, B, path, walkers, st)
                for i, (raw, out) in enumerate(zip(blocks, outs)):
                    assert np.array_equal(out, raw), (method, B, path, walkers, i)
    finally:
        for k, v in saved.items():
            c.set_option(k, v)
