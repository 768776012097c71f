"""CPU tests of tests/seg_craft.py, the checkers and corpus the GPU tests of segment-parallel encode rely on
(tests/test_gpu_segment_encode_craft.py): the LZ4 walker agrees with the oracle's verdicts and rejects each broken rule,
re-framing reproduces a frame's first block and catches blocks that lean on earlier ones, and the corpus is deterministic
and puts its features where it says."""
import os
import re

import numpy as np
import pytest

import lz4_craft
import oracle_lib
import seg_craft as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
KIB, MIB = 1024, 1 << 20


@pytest.fixture(scope="module")
def stock():
    s = oracle_lib.StockLibs()
    if s.lz4 is None or s.zstd is None:
        pytest.fail("liblz4.so.1 and libzstd.so.1 are needed")
    return s


def _walk_ok(comp, B):
    try:
        sc.lz4_walk(comp, B)
        return True
    except sc.LZ4FormatError:
        return False


@pytest.mark.parametrize("B,n", [(4096, 300), (32768, 300), (131072, 300), (300001, 150), (1 << 20, 12)])
def test_walker_verdicts_match_the_oracle(oracle, B, n):
    """on lz4_craft's corpus the walker accepts a stream exactly when the oracle (liblz4 1.9.3's rules) decodes it to B
    bytes, but for offset 0: the block format calls it invalid and the walker rejects it, while LZ4_decompress_safe 1.9.3
    (and so the oracle) writes a match from the output position itself; no encoder may emit it"""
    agree = offset0 = 0
    for name, m in lz4_craft.corpus(B, n, 1):
        r, _ = oracle.lz4_decompress(m, B)
        w = _walk_ok(m, B)
        if w == (r == B):
            agree += 1
            if w:
                assert sum(ll + ml for _, ll, _, ml in sc.lz4_walk(m, B)) == B
            continue
        assert not w and r == B, (name, w, r)
        with pytest.raises(sc.LZ4FormatError, match="offset 0"):
            sc.lz4_walk(m, B)
        offset0 += 1
    assert agree > n // 2, (agree, offset0)


def test_walker_rejects_each_broken_rule(oracle):
    B = 4096
    enc = lambda seqs, last: np.frombuffer(bytes(lz4_craft.encode(seqs, last)), np.uint8)  # noqa: E731
    good = enc([(100, 50, 200)], B - 300)
    assert _walk_ok(good, B) and oracle.lz4_decompress(good, B)[0] == B
    cases = {
        "offset 0": enc([(100, 0, 200)], B - 300),
        "past the output": enc([(100, 101, 200)], B - 300),
        "after B - 12": enc([(B - 11, 50, 4)], 7),
        "inside the last 5 bytes": enc([(100, 50, B - 100 - 4)], 4),
        "not at B": enc([(100, 50, 200)], B - 301),
        "trailing": np.append(good, np.uint8(0)),
    }
    long_tail = enc([(100, 50, 200)], B - 299)
    for why, m in cases.items():
        with pytest.raises(sc.LZ4FormatError):
            sc.lz4_walk(m, B)
    assert not _walk_ok(long_tail, B) and not _walk_ok(good[:-1], B)
    # at the limits: a last match that starts at B - 12 and ends at B - 5; offset = the output so far; offset 65 535
    edge = enc([(100, 100, B - 112)], 12)
    assert _walk_ok(edge, B) and oracle.lz4_decompress(edge, B)[0] == B
    far = enc([(65535, 65535, 100)], 5)
    assert sc.lz4_walk(far, 65640)[0] == (0, 65535, 65535, 100)


@pytest.mark.parametrize("B", [4096, 128 * KIB, 128 * KIB + 1, MIB, MIB + 1, 16 * MIB])
def test_walker_accepts_encoder_output(oracle, stock, B):
    """the oracle's and liblz4's blocks of every size class of the device encoders (up to 128 KiB, 1 MiB, 16 MiB)"""
    for dist in ((0, 3) if B < 16 * MIB else (0,)):
        raw = oracle.synth(2, dist, B, dist)
        for comp in (oracle.lz4_compress(raw, 1), stock.lz4_compress(raw, 7)):
            seqs = sc.lz4_walk(comp, B)
            sc.lz4_segment_checks(seqs, B, B)
            assert all(0 < off <= sc.LZ4_MAX_OFFSET for _, _, off, ml in seqs if ml)


def test_interior_match_rule():
    S, B = 4096, 3 * 4096 + 100
    seqs = [(0, 100, 50, S - 100), (S, 10, 5, S - 10), (2 * S, S + 20, 7, 60), (3 * S + 80, 20, 0, 0)]
    sc.lz4_segment_checks(seqs, B, S)          # matches end at s1 (or, in the last segment, by the block's rules)
    with pytest.raises(AssertionError):
        sc.lz4_segment_checks([(0, 100, 50, S - 99), (S + 1, B - S - 1, 0, 0)], B, S)


def _independent_frame(stock, raw, S):
    """a frame whose blocks are those of separate one-block frames of each S-byte slice: independent, reach 0"""
    blocks = []
    for s0 in range(0, raw.nbytes, S):
        _, bl = sc.zstd_segment_blocks(stock.zstd_compress(raw[s0:s0 + S], 1))
        assert len(bl) == 1
        blocks.append(bytearray(bl[0][0]))
    for b in blocks[:-1]:
        b[0] &= 0xFE
    wl = sc.wlog_for(raw.nbytes)
    head = bytes(sc._MAGIC) + bytes([0, (wl - 10) << 3])
    return np.frombuffer(head + b"".join(bytes(b) for b in blocks), np.uint8)


def test_reframe_and_the_independence_check(oracle, stock):
    B = MIB
    raw = oracle.synth(0, 0, B, 0)
    lib = stock.zstd_compress(raw, 1)
    decoders = [oracle.zstd_decompress, stock.zstd_decompress]
    _, blocks = sc.zstd_segment_blocks(lib)
    # the first block alone is the frame's own output
    for dec in decoders:
        r, out = dec(sc.reframe(b"", blocks[0][0], 17), 128 * KIB)
        assert r == 128 * KIB and np.array_equal(out, raw[:128 * KIB])
    # teeth: libzstd's blocks lean on the ones before them (repeat offsets, repeated tables)
    bad = sc.zstd_independence_failures(lib, raw, 128 * KIB, decoders)
    assert bad and 0 not in bad, bad
    # blocks of separate frames pass both checks, with no history at all (as a whole frame they need not decode: libzstd
    # wrote them for the repeat offsets {1, 4, 8} of a frame's start, which is what re-framing gives them)
    ind = _independent_frame(stock, raw, 128 * KIB)
    assert sc.zstd_independence_failures(ind, raw, 128 * KIB, decoders) == []
    assert sc.zstd_reach_failures(ind, raw, 128 * KIB, 0, decoders) == []
    # the reach check has teeth too: the third 128 KiB block repeats the first, 256 KiB behind it
    rnd = np.random.default_rng(1).integers(0, 256, 256 * KIB, dtype=np.uint8)
    far = np.concatenate([rnd, rnd[:128 * KIB]])
    f = stock.zstd_compress(far, 1)
    assert sc.zstd_reach_failures(f, far, 128 * KIB, 0, decoders) == [2]
    assert sc.zstd_reach_failures(f, far, 128 * KIB, 128 * KIB, decoders) == []


def test_structure_checks(oracle, stock):
    raw = oracle.synth(0, 1, MIB, 0)
    lib = stock.zstd_compress(raw, 1)
    sc.zstd_structure_checks(lib, lib, MIB, 128 * KIB)
    with pytest.raises(AssertionError):
        sc.zstd_structure_checks(lib, lib, MIB, 64 * KIB)
    tgt = stock.zstd_compress2(raw[:128 * KIB], {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: 1, oracle_lib.ZSTD_C_TARGET_CBLOCK_SIZE: 1340})
    info = sc.zstd_craft.walk(tgt)
    n = len(info["blocks"])
    assert any(b.get("lit") == "treeless" or "repeat" in (b.get("modes") or ()) for b in info["blocks"])
    with pytest.raises(AssertionError, match="treeless|repeat"):
        sc.zstd_structure_checks(tgt, tgt, n * 1024, 1024)


def test_seed_constants_match_the_kernels():
    z = open(os.path.join(CSRC, "zstd_enc.hip")).read()
    lz = open(os.path.join(CSRC, "lz4_enc2.hip")).read()
    assert re.search(r"kZSegSeedBytes = %d\b" % sc.ZSTD_FAST_SEED, z)
    assert re.search(r"kZSegSeedBytesDfast = %d, kZSegSeedBytesLazy = %d\b" % (sc.ZSTD_DEEP_SEED, sc.ZSTD_DEEP_SEED), z)
    assert re.search(r"kSegSeedBytes = %d\b" % sc.LZ4_SEED, lz)
    assert "if (w + seg_bytes > win) w = win > seg_bytes ? win - seg_bytes : 0u;" in z


def test_seed_window_and_levels(stock):
    """W clamps to the window minus S only where the window is small; the level chooser finds every strategy"""
    assert sc.zstd_seed_window(1, 13, 4096) == 16384            # `fast` seeds 16 KiB whatever the window
    assert sc.zstd_seed_window(2, 13, 4096) == 4096             # B = S + 1 = 4097: window 8 KiB
    assert sc.zstd_seed_window(4, 15, 16384) == 16384           # B = 16 KiB + 1: window 32 KiB, no clamp
    assert sc.zstd_seed_window(6, 14, 4096) == 12288
    assert sc.zstd_seed_window(6, 21, 131072) == 16384
    for B in (4097, 16385, 128 * KIB + 1, 256 * KIB + 1, MIB):
        lv = sc.zstd_levels(stock, B)
        assert sorted(lv) == [1, 2, 3, 4, 5, 6], (B, lv)
        for strat, level in lv.items():
            assert sc.zstd_cparams(stock, level, B)[1] == strat


@pytest.mark.parametrize("B,S", [(4097, 4096), (2 * 4096 + 13, 4096), (MIB, 4096), (MIB, 131072), (2 * MIB + 5, 16384)])
def test_corpus_deterministic_and_as_stated(B, S):
    a = sc.segment_corpus(B, S, 3)
    b = sc.segment_corpus(B, S, 3)
    feats = sc.corpus_features(B, S, 3)
    assert [n for n, _ in a] == [n for n, _ in b] == list(feats)
    assert len(set(feats)) == len(a)
    for (name, x), (_, y) in zip(a, b):
        assert x.dtype == np.uint8 and x.nbytes == B and np.array_equal(x, y), name
        sc.check_features(x, feats[name])
    assert not np.array_equal(a[0][1], sc.segment_corpus(B, S, 4)[0][1])
    nb = -(-B // S) - 1
    if nb >= 48:
        # every boundary (or the sample) carries a straddling copy, a carried run and the three offset traps
        for name in ("straddle/0", "straddle/1", "carry/thresholds", "reps/same_offset"):
            assert len(feats[name]) >= min(nb, 64) - 1, (name, len(feats[name]))
        at = {int(f[5:].split("<")[0]) % S for f in feats["straddle/0"] + feats["straddle/1"]}
        assert {(S - d) % S for d in sc.STRADDLE_AT} <= at
        tu = {sum(map(int, f.split(":")[1].split("+"))) for f in feats["carry/thresholds"]}
        assert set(sc.CARRY_TOTALS) <= tu
        dist = {int(f[5:].split("<")[0]) - int(f.split("<")[1].split("+")[0]) for f in feats["straddle/0"] + feats["straddle/1"]}
        assert set(sc.straddle_distances(sc.ZSTD_FAST_SEED)) <= dist, sorted(dist)


@pytest.mark.parametrize("S", [4096, 16384])
def test_effectiveness_bound_separates_seeded_from_unseeded(oracle, S):
    """whole-block LZ4 (what seeding approaches) fits the bound; slices compressed on their own (no seeding) do not.
    (At S = 128 KiB a 1 MiB block has too few segments for the bound to tell the two apart.)"""
    B = MIB
    for P in sc.PERIODS:
        raw = dict(sc.segment_corpus(B, S, 5))["periodic/%d" % P]
        bound = sc.effectiveness_bound(P, B, S, lz4=True)
        assert len(oracle.lz4_compress(raw, 1)) <= bound
        alone = sum(len(oracle.lz4_compress(raw[s:s + S], 1)) for s in range(0, B, S))
        if P >= 1000:                 # (61 literals per segment are lost in the per-segment allowance)
            assert alone > 4 * bound, (P, S, alone, bound)
