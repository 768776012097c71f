"""CPU tests of tests/zstd_enc_craft.py, the inputs tests/test_gpu_zstd_encode_craft.py puts through the device encoders.

The GPU test's bar is equality with the oracle, so the oracle is pinned here: on every crafted input, at every level the
GPU test uses it at, its frame is stock libzstd's (1.4.8), byte for byte.  And the inputs are held to what makes them tests:
at every level >= 1 the first block of a sweep or long-match frame is a compressed block (a raw block would hide every
sequence decision), at every level >= 4 it has a sequence, and every sweep case comes out in at least two ways across the
levels (a case every strategy encodes alike tests nothing).  These are asserted on the oracle's frames, so they hold on a
machine without the stock library.  Negative levels write raw literals and mostly raw blocks here: compared, not counted.

Figures of this list (printed with -s): 906 / 834 / 834 sweep cases at 4096 / 1024 / 1025 bytes, 192 long-match cases at
16 384; at least 1 sequence in every first block at levels >= 4; 3 / 2 / 2 distinct frames per sweep case at the least
(median 6 / 3 / 4), 4 for the long matches (median 8)."""
import numpy as np
import pytest

import oracle_lib
import zstd_craft
import zstd_enc_craft as zc

LEVELS = (-5, -1) + tuple(range(1, 23))        # what the GPU test runs the sweep and long-match lists at
SIZES = zc.SWEEP_SIZES + (zc.LONG_B,)


@pytest.fixture(scope="module")
def stock():
    s = oracle_lib.StockLibs()
    if s.zstd is None:
        pytest.skip("libzstd.so.1 not loadable")
    return s


@pytest.fixture(scope="module")
def frames(oracle):
    """{B: {level: [the oracle's frame of every case]}}, computed once"""
    cache = {}

    def get(B):
        if B not in cache:
            _, blocks = zc.blocks(B)
            cache[B] = {lv: [oracle.zstd_compress(b, lv) for b in blocks] for lv in LEVELS}
        return cache[B]
    return get


# ---------------- the generator ----------------
def test_axes_and_case_list():
    assert zc.CASES == zc._case_list()                         # fixed by the seed in the file
    L, D, R, T = (set(a) for a in (zc.L_AXIS, zc.D_AXIS, zc.R_AXIS, zc.TAIL_AXIS))
    assert set(range(3, 10)) | {11, 12, 13} <= L
    assert {64 * k + d for k in range(1, 8) for d in (-2, -1, 0, 1, 2)} | {510, 511, 512, 513} <= L and 514 not in L
    assert {t + d for t in (12, 16, 24, 32, 48, 64, 128, 256, 512, 999) for d in (-1, 1)} <= L
    assert D == {1, 2, 3, 4, 5, 7, 8, 9, 16, 63, 64, 65, 127, 128, 129, 1000}
    assert R == {0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 66, 128}
    assert T == set(range(10)) | {12, 31, 32, 33, 63, 64, 65, 128}
    cases = set(zc.CASES)
    for a, at in ((L, 0), (D, 1), (R, 2), (T, 3)):             # every single-axis sweep around the base case
        for v in a:
            c = [zc.BASE] * 4
            c[at] = v
            assert tuple(c) in cases
    single = {c for c in cases if sum(v != zc.BASE for v in c) <= 1}
    assert len(cases) - len(single) >= 780                     # 800 random combinations, but for the few drawn twice
    assert len(zc.sweep_cases(4096)) == len(zc.CASES)          # all of them fit 4 KiB
    for B in (1024, 1025):
        kept = zc.sweep_cases(B)
        assert 800 <= len(kept) < len(zc.CASES) and all(zc.fits(B, *c) for c in kept)
        assert set(zc.CASES) - set(kept) == {c for c in zc.CASES if not zc.fits(B, *c)}
    lc = zc.long_cases()
    assert len(lc) == len(set(lc)) == 8 * 4 * 2 * 3 and all(zc.fits(zc.LONG_B, *c) for c in lc)
    assert {c[0] for c in lc} == set(range(4093, 4100)) | {8190}


@pytest.mark.parametrize("B", SIZES)
def test_blocks_are_as_stated(B):
    cases, blocks = zc.blocks(B)
    assert len(cases) == len(blocks) and zc.blocks(B)[1] is blocks
    for i, ((L, D, R, tail), x) in enumerate(zip(cases, blocks)):
        assert x.dtype == np.uint8 and x.nbytes == B and not x.flags.writeable
        p = B - tail - L
        q = p - R
        bg = np.random.default_rng(zc.SEED + i).integers(0, 64, B)
        assert np.array_equal(x[:q - 40], bg[:q - 40])                      # nothing before the leading match is touched
        assert np.array_equal(x[p:p + L], x[p - D:p - D + L])                # the match under test, at distance D
        assert np.array_equal(x[q - 40:q], x[q - 240:q - 200])              # the leading match, at distance 200
        if R > 0:
            assert x[q] != x[q - 200] and x[p - 1] != x[p - 1 - D]          # neither match goes on, nor starts sooner
            assert np.array_equal(x[q + 1:p - 1], bg[q + 1:p - 1])
        if tail > 0:
            assert x[p + L] != x[p + L - D]
            assert np.array_equal(x[p + L + 1:], bg[p + L + 1:])
        else:
            assert p + L == B
    assert np.array_equal(zc.sweep_block(5, B, *cases[0]), zc.sweep_block(5, B, *cases[0]))
    assert not np.array_equal(zc.sweep_block(5, B, *cases[0]), zc.sweep_block(6, B, *cases[0]))


def test_mixed_frames_are_as_stated():
    mf = dict(zc.mixed_frames())
    K = zc.ZSTD_BLOCK
    assert len(mf) == 8 and all(a.nbytes > K and not a.flags.writeable for a in mf.values())
    assert mf["text|random|zeros|text"].nbytes == 443216 and not mf["text|random|zeros|text"][2 * K:3 * K].any()
    assert mf["random|text"].nbytes == 262145 and mf["runs across the edge"].nbytes == 262149
    a = mf["zeros|text|run"]
    assert not a[:K].any() and (a[2 * K:] == a[2 * K]).all() and a[2 * K] != 0
    a = mf["match across the edge"]
    assert np.array_equal(a[K - 1700:K + 2300], a[K - 51700:K - 47700]) and a[K + 2300] != a[K - 47700]
    a = mf["second block repeats the first"]
    assert a.nbytes == 2 * K and np.array_equal(a[:K], a[K:])
    a = mf["runs across the edge"]
    assert len(set(a[:K - 1])) == 1 and a[K - 1] != a[K] and a[K - 1] != a[0] and a[K] != a[0] and a[K + 1] == a[0]
    a = mf["copy into the third block from the first"]
    assert np.array_equal(a[2 * K + 30000:2 * K + 90000], a[5000:65000])
    a = mf["3-byte words"].reshape(-1, 4)
    assert a.shape[0] * 4 == 3 * K and len({bytes(w) for w in a[:, :3]}) == 16
    assert sum(len(g) for g in zc.mixed_by_size().values()) == 8
    assert [n for n, _ in zc.mixed_frames()] == [n for n, _ in zc.mixed_frames()]


# ---------------- the frame peek ----------------
def test_first_block_agrees_with_the_frame_walker(oracle, frames):
    """on frames of every kind of first block and literals section, against tests/zstd_craft.walk"""
    kinds = {"raw": zc.BLOCK_RAW, "rle": zc.BLOCK_RLE, "compressed": zc.BLOCK_COMPRESSED}
    inputs = [oracle.zstd_compress(a, 1) for _, a in zc.mixed_frames()]
    inputs += [oracle.zstd_compress(np.zeros(n, np.uint8), 3) for n in (1, 40, 5000)]
    inputs += [oracle.zstd_compress(oracle.synth(1, d, 131072, d), lv) for d in range(5) for lv in (-5, 1, 5)]
    inputs += [f for lv in (-5, 1, 22) for f in frames(4096)[lv][::50]]
    # libzstd 1.4.8 never opens a frame with an RLE block: one by hand (single segment, 5 bytes of 0x41)
    inputs.append(np.frombuffer(b"\x28\xb5\x2f\xfd\x20\x05\x2b\x00\x00\x41", np.uint8))
    seen_types, seen_lits, long_count = set(), set(), False
    for f in inputs:
        b = zstd_craft.walk(f)["blocks"][0]
        assert zc.first_block(f) == (kinds[b["type"]], b.get("nseq", 0)), b
        seen_types.add(b["type"])
        seen_lits.add(b.get("lit"))
        long_count |= b.get("nseq", 0) >= 128
    assert seen_types == set(kinds) and {"raw", "compressed"} <= seen_lits and long_count
    with pytest.raises(AssertionError):
        zc.first_block(np.zeros(16, np.uint8))


# ---------------- the oracle is the stock library on these inputs ----------------
@pytest.mark.parametrize("B", SIZES)
def test_oracle_is_libzstd_on_every_case(stock, frames, B):
    assert stock.zstd.ZSTD_versionNumber() == 10408
    cases, blocks = zc.blocks(B)
    bad = [(B, lv, c) for lv in LEVELS for c, b, f in zip(cases, blocks, frames(B)[lv])
           if not np.array_equal(stock.zstd_compress(b, lv), f)]
    assert bad == [], (len(bad), bad[:10])


def test_oracle_is_libzstd_on_the_mixed_frames(oracle, stock):
    for name, a in zc.mixed_frames():
        for lv in zc.MIXED_LEVELS:
            f = oracle.zstd_compress(a, lv)
            assert np.array_equal(stock.zstd_compress(a, lv), f), (name, lv)
            r, out = oracle.zstd_decompress(f, a.nbytes)
            assert r == a.nbytes and np.array_equal(out, a), (name, lv)


# ---------------- the inputs cannot hide a failure ----------------
@pytest.mark.parametrize("B", SIZES)
def test_first_block_is_compressed_and_has_sequences(frames, B):
    cases, _ = zc.blocks(B)
    fewest = None
    for lv in LEVELS:
        if lv < 1:
            continue
        for c, f in zip(cases, frames(B)[lv]):
            btype, nseq = zc.first_block(f)
            assert btype == zc.BLOCK_COMPRESSED, (B, lv, c, btype)
            if lv >= 4:
                assert nseq >= 1, (B, lv, c)
                fewest = nseq if fewest is None else min(fewest, nseq)
    print("B = %d: %d cases, at least %d sequence(s) in a first block at levels >= 4" % (B, len(cases), fewest))


@pytest.mark.parametrize("B", SIZES)
def test_levels_encode_every_case_in_more_than_one_way(frames, B):
    cases, _ = zc.blocks(B)
    per_level = frames(B)
    distinct = [len({per_level[lv][i].tobytes() for lv in LEVELS}) for i in range(len(cases))]
    alike = [c for c, d in zip(cases, distinct) if d < 2]
    assert alike == [], (B, alike[:10])
    print("B = %d: distinct frames per case across %d levels: min %d, median %d"
          % (B, len(LEVELS), min(distinct), sorted(distinct)[len(distinct) // 2]))
