"""CPU tests: the references of tests/test_gpu_large_blocks.py on blocks above 1 MiB (tests/large_blocks.py).

The stock liblz4 1.9.3 / libzstd 1.4.8 are required here (a failure, not a skip, without them).  The oracle encoders equal
them byte for byte for LZ4 and zstd levels -5 .. 10; the oracle zstd encoder refuses levels 11 .. 22 above 1 MiB (its
tables stop at 2^21 entries), so there the live libzstd is the only reference; the oracle decoders equal the stock decoders
in verdict and bytes on crafted LZ4 streams, stock zstd frames, frames with offsets of 32 MiB and more, and damaged copies."""
import numpy as np
import pytest

import large_blocks as lb
import lz4_craft
import oracle_lib
import zstd_craft
from large_blocks import MIB

ENC_SIZES = [MIB + 1, 2 * MIB + 5, 4 * MIB + 24]
LZ4_ACCELS = [1, 7, 65537]
ZSTD_ORACLE_LEVELS = list(range(-5, 0)) + list(range(1, 11))
ZSTD_REFUSED_LEVELS = list(range(11, 23))


@pytest.fixture(scope="module")
def stock():
    return lb.require_stock()


def test_stock_libraries_are_the_pinned_versions(stock):
    assert (stock.lz4_version, stock.zstd_version) == ("1.9.3", "1.4.8")


def _encoders_agree(oracle, stock, name, raw):
    B = raw.nbytes
    for accel in LZ4_ACCELS:
        exp = stock.lz4_compress(raw, accel)
        assert len(exp) > 0
        assert np.array_equal(oracle.lz4_compress(raw, accel), exp), ("lz4", B, name, accel)
    for level in ZSTD_ORACLE_LEVELS:
        got = oracle.zstd_compress(raw, level)
        assert len(got) > 0, ("zstd oracle refuses", B, name, level)
        assert np.array_equal(got, stock.zstd_compress(raw, level)), ("zstd", B, name, level)


@pytest.mark.parametrize("B", ENC_SIZES)
def test_oracle_encoders_equal_stock(oracle, stock, B):
    for name, raw in lb.blocks(oracle, B):
        _encoders_agree(oracle, stock, name, raw)


def test_oracle_encoders_equal_stock_above_16mib(oracle, stock):
    for name, raw in lb.blocks(oracle, 16 * MIB + 1, ["wide", "far_repeats"]):
        _encoders_agree(oracle, stock, name, raw)


@pytest.mark.parametrize("B", ENC_SIZES + [16 * MIB + 1])
def test_oracle_zstd_encoder_refuses_deep_levels(oracle, B):
    """levels 11 .. 22 above 1 MiB need hash or chain tables beyond the oracle's 2^21 entries: it returns 0 and writes no
    frame.  When this fails because the oracle grew, extend test_oracle_encoders_equal_stock and the GPU file's references
    to those levels."""
    raw = lb.synth(oracle, 0, B)
    cap = oracle.L.cryo_oracle_zstd_bound(B)
    for level in ZSTD_REFUSED_LEVELS:
        d = np.full(cap, 0xC3, np.uint8)
        r = oracle.L.cryo_oracle_zstd_compress(raw.ctypes.data, B, d.ctypes.data, cap, level)
        assert r == 0, (B, level, r)
        assert bytes(d[:4]) != (0xFD2FB528).to_bytes(4, "little"), (B, level)


def test_zstd_levels_cover_every_strategy(stock):
    """the levels the GPU file encodes at hold every strategy of libzstd's table, at every size class"""
    import seg_craft
    assert sorted(set(lb.ZSTD_STRATEGY.values())) == list(range(1, 10))
    for B in lb.ZSTD_ENC:
        for level, strategy in lb.ZSTD_STRATEGY.items():
            assert seg_craft.zstd_cparams(stock, level, B)[1] == strategy, (B, level)


def _decoders_agree(oracle, stock, method, cases, B):
    """verdict and bytes of oracle and stock decoder on [(name, stream)]; returns the number accepted"""
    ok = 0
    for name, m in cases:
        if method == "lz4":
            r1, o1 = stock.lz4_decompress(m, B, fill=0xA5)
            r2, o2 = oracle.lz4_decompress(m, B, fill=0xA5)
        else:
            r1, o1 = stock.zstd_decompress(m, B, fill=0xA5)
            r2, o2 = oracle.zstd_decompress(m, B, fill=0xA5)
        assert (r1 == B) == (r2 == B), (method, B, name, r1, r2)
        if r2 == B:
            assert np.array_equal(o1, o2), (method, B, name)
            ok += 1
    return ok


@pytest.mark.parametrize("B,n,accepted", [(b, lb.DEC_CRAFTED_LZ4[b], a) for b, a in ((2 * MIB + 8, 6), (4 * MIB + 24, 2), (16 * MIB + 8, 1))])
def test_oracle_lz4_decoder_equals_liblz4_on_crafted_streams(oracle, stock, B, n, accepted):
    cases = lz4_craft.corpus(B, n, lb.CRAFTED_LZ4_SEED)
    ok = _decoders_agree(oracle, stock, "lz4", cases, B)
    assert 1 <= ok < n, (B, ok, n)
    assert ok == accepted, (B, ok)
    muts = [x for name, m in cases for x in lb.mutants(name, m, 2)]
    _decoders_agree(oracle, stock, "lz4", muts, B)


def test_oracle_decoders_equal_stock_on_stock_streams(oracle, stock):
    B = 4 * MIB + 24
    n_ok = n_bad = 0
    for name, raw in lb.blocks(oracle, B):
        frames = [("%s/l%d" % (name, lvl), stock.zstd_compress(raw, lvl)) for lvl in (1, 3, 9, 19)]
        for fname, f in frames:
            r, out = oracle.zstd_decompress(f, B)
            assert r == B and np.array_equal(out, raw), fname
        muts = [x for fname, f in frames for x in lb.mutants(fname, f, 3)]
        k = _decoders_agree(oracle, stock, "zstd", frames + muts, B)
        n_ok += k
        n_bad += len(frames) + len(muts) - k
        streams = [("%s/a%d" % (name, a), stock.lz4_compress(raw, a)) for a in (1, 50)]
        muts = [x for sname, s in streams for x in lb.mutants(sname, s, 3)]
        assert _decoders_agree(oracle, stock, "lz4", streams + muts, B) >= len(streams)
    assert n_ok >= 40 and n_bad >= 20, (n_ok, n_bad)


@pytest.fixture(scope="module")
def far(stock):
    return lb.far_frames(stock)


def test_far_window_frames_decode_alike(oracle, stock, far):
    assert len({name: f for name, _, f in far}["far_window/wlog27/l3"]) == 1051026
    for name, raw, f in far:
        for dec in (stock.zstd_decompress, oracle.zstd_decompress):
            r, out = dec(f, raw.nbytes)
            assert r == raw.nbytes and np.array_equal(out, raw), name
    muts = [x for name, _, f in far for x in lb.mutants(name, f, 3)]
    ok = _decoders_agree(oracle, stock, "zstd", muts, lb.FAR)
    assert ok < len(muts)


def test_far_window_frames_hold_offset_codes_25_and_26(far):
    """the windowLog-27 frames really reach 40 MiB back (offset code 25: 25 extra bits in one read) and those of
    far_window_split 71 MiB back as well (code 26); far_window's own last copy is served from 31 MiB back (code 24), and
    plain level 1 (windowLog 19) reaches neither"""
    for name, _, f in far:
        codes = lb.frame_offset_codes(f)
        w = zstd_craft.walk(f)
        assert w is not None and w["end"] == len(f), name
        if "wlog27" in name:
            assert any(c >= 25 for c in codes), (name, sorted(codes))
            if name.startswith("far_window_split"):
                assert any(c >= 26 for c in codes), (name, sorted(codes))
        else:
            assert max(codes, default=0) <= 19, (name, sorted(codes))


def test_offset_code_reader_on_known_frames(oracle, stock):
    """the reader against frames whose offsets are known by construction: one far copy at a chosen distance"""
    rng = np.random.default_rng(3)
    for dist, code in ((1 << 12, 12), (300000, 18), (3 * MIB, 21)):
        B = dist + 70000
        raw = rng.integers(0, 256, B, dtype=np.uint8)
        raw[dist:dist + 60000] = raw[:60000]
        f = stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: 3, oracle_lib.ZSTD_C_WINDOWLOG: 23})
        codes = lb.frame_offset_codes(f)
        assert max(codes) == code, (dist, sorted(codes))


def test_zstd_frames_straddle_the_planner_block_cap(oracle, stock):
    """253 x 128 KiB and 8 bytes more: stock frames of 253 and 254 blocks, either side of zstd_craft.zstd_nbmax"""
    for B, nb in zip(lb.ZSTD_ONLY_DEC, (253, 254)):
        f = stock.zstd_compress(lb.synth(oracle, 0, B), 1)
        assert len(zstd_craft.walk(f)["blocks"]) == nb, B
    assert zstd_craft.zstd_nbmax(lb.ZSTD_ONLY_DEC[0]) == 254


def test_builders_are_deterministic_and_hold_what_they_claim(oracle):
    B = 2 * MIB + 5
    for name in lb.BUILDERS:
        a, b = lb.build(oracle, name, B), lb.build(oracle, name, B)
        assert a.dtype == np.uint8 and a.nbytes == B and np.array_equal(a, b), name
    a = lb.far_repeats(4 * MIB)
    pos = lb.far_repeat_positions(4 * MIB)
    assert {(1 << 16) + 100, (1 << 17) - 3100, MIB + 100, 2 * MIB - 3100, 4 * MIB - 3100} <= set(pos)
    for p in pos:
        assert np.array_equal(a[p:p + lb.CHUNK], a[:lb.CHUNK]), p
    w = lb.far_window(lb.FAR)
    assert np.array_equal(w[40 * MIB:41 * MIB], w[:MIB]) and np.array_equal(w[-MIB:], w[:MIB]) and not w[MIB:40 * MIB].any()
