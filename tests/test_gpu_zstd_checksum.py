"""GPU tests of zstd content checksums (CRYO_OPT_ZSTD_CHECKSUM).

With the option on, every zstd frame the encoders write is libzstd's frame with ZSTD_c_checksumFlag = 1: the checksum flag
in the frame header and the low 32 bits of XXH64 of the input after the last block.  Segment mode adds the same flag and
trailer to its own frames.  With the option off, or switched back off, the bytes are today's.  Checksummed frames decode on
every route, and a frame whose content no longer matches its checksum is rejected on every route."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import zstd_craft
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

pytestmark = pytest.mark.gpu

CK = {oracle_lib.ZSTD_C_CHECKSUM_FLAG: 1}
M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = (11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579,
                      2870177450012600261)


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, v):
    return (_rotl((acc + v * P2) & M64, 31) * P1) & M64


def xxh64_py(data):
    """XXH64, seed 0 (for machines without libzstd.so.1)"""
    b = bytes(data)
    n, o = len(b), 0
    if n >= 32:
        v = [(P1 + P2) & M64, P2, 0, (-P1) & M64]
        while o + 32 <= n:
            for k in range(4):
                v[k] = _round(v[k], int.from_bytes(b[o + 8 * k:o + 8 * k + 8], "little"))
            o += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for x in v:
            h = (((h ^ _round(0, x)) * P1) + P4) & M64
    else:
        h = P5
    h = (h + n) & M64
    while o + 8 <= n:
        h ^= _round(0, int.from_bytes(b[o:o + 8], "little"))
        h = (_rotl(h, 27) * P1 + P4) & M64
        o += 8
    if o + 4 <= n:
        h ^= (int.from_bytes(b[o:o + 4], "little") * P1) & M64
        h = (_rotl(h, 23) * P2 + P3) & M64
        o += 4
    while o < n:
        h ^= (b[o] * P5) & M64
        h = (_rotl(h, 11) * P1) & M64
        o += 1
    h ^= h >> 33
    h = (h * P2) & M64
    h ^= h >> 29
    h = (h * P3) & M64
    return h ^ (h >> 32)


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


def xxh64(stock, raw):
    a = np.ascontiguousarray(raw, np.uint8)
    if stock.zstd is not None:
        f = stock.zstd.ZSTD_XXH64
        f.restype, f.argtypes = C.c_uint64, [C.c_void_p, C.c_size_t, C.c_ulonglong]
        return int(f(a.ctypes.data, a.nbytes, 0))
    return xxh64_py(a)


def with_checksum(stock, frame, raw):
    """a frame without a checksum -> the same frame with one: the flag in the descriptor byte, XXH64's low 32 bits behind"""
    f = np.array(frame, np.uint8)
    assert f[4] & 0x04 == 0
    f[4] |= 0x04
    return np.concatenate([f, np.frombuffer((xxh64(stock, raw) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)])


def expected(stock, oracle, raw, level):
    if stock.zstd is not None:
        return stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: level, **CK})
    return with_checksum(stock, oracle.zstd_compress(raw, level), raw)


def decode_ref(stock, oracle, frame, B):
    """(size or -1, bytes) of the stock decoder where present, else of the oracle"""
    return stock.zstd_decompress(frame, B) if stock.zstd is not None else oracle.zstd_decompress(frame, B)


@pytest.fixture()
def ck(codec):
    yield codec
    for opt, v in ((cc.OPT_ZSTD_CHECKSUM, 0), (cc.OPT_ENCODE_VERIFY, 0), (cc.OPT_ENCODE_SEGMENT_BYTES, 0),
                   (cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, 1), (cc.OPT_ZSTD_DECODE_PATH, 0)):
        codec.set_option(opt, v)


def test_option_values(ck):
    assert ck.get_option(cc.OPT_ZSTD_CHECKSUM) == 0
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    assert ck.get_option(cc.OPT_ZSTD_CHECKSUM) == 1
    for bad in (-1, 2, 1 << 40):
        with pytest.raises(CryoError):
            ck.set_option(cc.OPT_ZSTD_CHECKSUM, bad)
    assert ck.get_option(cc.OPT_ZSTD_CHECKSUM) == 1


@pytest.mark.parametrize("level", list(range(-5, 0)) + list(range(1, 23)))
def test_identical_to_libzstd_every_level_128k(ck, oracle, stock, level):
    B = 131072
    raws = [oracle.synth(50 + level, i, B, i % 5) for i in range(5)]   # every generator distribution
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    got = ck.compress_blocks(METHOD_ZSTD, level, raws)
    for i, r in enumerate(raws):
        want = expected(stock, oracle, r, level)
        assert np.array_equal(got[i], want), (level, i)
    # the host-buffer entry point, one block
    assert np.array_equal(ck.compress_block(METHOD_ZSTD, level, raws[level % 5]), expected(stock, oracle, raws[level % 5], level))


@pytest.mark.parametrize("B,levels", [(1 << 20, (-5, 1, 2, 3, 6, 9, 13, 19)),
                                      (1, (1, 3)), (31, (1, 19)), (32, (1,)), (33, (1, 5)), (100, (1, 12)),
                                      (1000, (-1, 1, 3, 19)), (4096, (1, 7, 22)), (65536 + 257, (1, 3, 16)),
                                      (300001, (1, 4))])
def test_identical_to_libzstd_sizes(ck, oracle, stock, B, levels):
    """odd sizes put blocks at every alignment (the rows of a batch lie B bytes apart) and exercise the hash's tail steps"""
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    for level in levels:
        raws = [oracle.synth(7, i, B, i % 5) for i in range(5 if B < (1 << 20) else 2)]
        got = ck.compress_blocks(METHOD_ZSTD, level, raws)
        for i, r in enumerate(raws):
            assert np.array_equal(got[i], expected(stock, oracle, r, level)), (B, level, i)


def test_fallback_derivation_matches_libzstd(oracle, stock):
    """the expected bytes of machines without libzstd (oracle frame + flag + Python XXH64) are libzstd's"""
    if stock.zstd is None:
        pytest.skip("libzstd.so.1 not present")
    for B, level in ((131072, 1), (1000, 3), (31, 1)):
        r = oracle.synth(3, 0, B, 1)
        assert xxh64_py(r) == xxh64(stock, r)
        assert np.array_equal(with_checksum(stock, oracle.zstd_compress(r, level), r), expected(stock, oracle, r, level))


def test_off_means_unchanged(ck, oracle):
    B = 131072
    raws = [oracle.synth(9, i, B, i % 5) for i in range(5)]
    want = [oracle.zstd_compress(r, 3) for r in raws]
    for got in (ck.compress_blocks(METHOD_ZSTD, 3, raws), None, None):
        if got is None:   # 0 -> 1 -> 0 on the same handle
            ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
            on = ck.compress_blocks(METHOD_ZSTD, 3, raws)
            assert all(len(a) == len(b) + 4 for a, b in zip(on, want))
            ck.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
            got = ck.compress_blocks(METHOD_ZSTD, 3, raws)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_lz4_unaffected(ck, oracle):
    B = 131072
    raws = [oracle.synth(4, i, B, i % 5) for i in range(5)]
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    got = ck.compress_blocks(METHOD_LZ4, 1, raws)
    assert all(np.array_equal(g, oracle.lz4_compress(r, 1)) for g, r in zip(got, raws))


@pytest.mark.parametrize("B", [131072, 1 << 20])
@pytest.mark.parametrize("strategy", [1, 6])
def test_segment_mode(ck, oracle, stock, B, strategy):
    level = 1 if strategy == 1 else (11 if B == 131072 else 13)   # `fast`; `btlazy2` at these sizes (libzstd 1.4.8)
    S = 32768
    raws = [oracle.synth(21, i, B, i % 5) for i in range(5)]
    ck.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, S)
    ck.set_option(cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY, strategy)
    plain = ck.compress_blocks(METHOD_ZSTD, level, raws)
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    checked = ck.compress_blocks(METHOD_ZSTD, level, raws)
    for i, r in enumerate(raws):
        assert zstd_craft.walk(plain[i])["checksum"] is False
        assert np.array_equal(checked[i], with_checksum(stock, plain[i], r)), i
        n, out = decode_ref(stock, oracle, checked[i], B)
        assert n == B and np.array_equal(out, r), i
        outs, st = ck.decompress_blocks(METHOD_ZSTD, [checked[i]], B)
        assert st[0] == 0 and np.array_equal(outs[0], r)


@pytest.mark.parametrize("n", [1, 8, 64, 4096])
@pytest.mark.parametrize("path", [0, 1, 2, 3])
def test_round_trip_every_route(ck, oracle, stock, n, path):
    """path 0 at up to 64 frames is the few-frames route, path 3 the same pipeline without it, 1 the fused kernel"""
    B = 131072 if n <= 64 else 32768
    uniq = [oracle.synth(31, i, B, i % 5) for i in range(min(n, 40))]
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    comps_u = ck.compress_blocks(METHOD_ZSTD, 1 + (n % 3), uniq)
    assert all(zstd_craft.walk(c)["checksum"] for c in comps_u)
    ck.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
    outs, st = ck.decompress_blocks(METHOD_ZSTD, [comps_u[i % len(uniq)] for i in range(n)], B)
    assert (st == 0).all(), np.unique(st)
    for i in range(n):
        assert np.array_equal(outs[i], uniq[i % len(uniq)]), i


@pytest.mark.parametrize("dist", [0, 1])
def test_one_frame_1mib_host_buffer(ck, oracle, dist):
    """the reference's read shape: one 1 MiB frame per call through the host-buffer entry point, on every route"""
    B = 1 << 20
    r = oracle.synth(5, 0, B, dist)
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    f = ck.compress_block(METHOD_ZSTD, 1, r)
    for path in range(4):
        ck.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
        assert np.array_equal(ck.decompress_block(METHOD_ZSTD, f, B), r), path
        bad = f.copy()
        bad[-1] ^= 0x01   # the stored checksum
        assert ck.decompress_block(METHOD_ZSTD, bad, B) is None, path


def _payload_offsets(frame, want):
    """offsets in the frame of the first block of kind `want`: ("raw", start, size) or ("rawlit", first literal, count)"""
    b = bytes(frame)
    info = zstd_craft.walk(b)
    fhd = b[4]
    single, did, fcs_flag = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    for blk in info["blocks"]:
        p += 3
        if want == "raw" and blk["type"] == "raw" and blk["size"] > 64:
            return p, blk["size"]
        if want == "rawlit" and blk["type"] == "compressed" and blk.get("lit") == "raw" and blk.get("nseq", 0) > 0:
            b0 = b[p]
            hl = (1, 2, 1, 3)[(b0 >> 2) & 3]
            size = b0 >> 3 if hl == 1 else int.from_bytes(b[p:p + hl], "little") >> 4
            if size > 64:
                return p + hl, size
        p += 1 if blk["type"] == "rle" else blk["size"]
    return None


@pytest.mark.parametrize("kind", ["raw", "rawlit"])
def test_corruption_caught(ck, oracle, stock, kind):
    B = 131072
    rng = np.random.default_rng(7)
    if kind == "raw":
        raw = rng.integers(0, 256, B, dtype=np.uint8)   # incompressible: raw blocks
    else:
        half = rng.integers(0, 256, B // 2, dtype=np.uint8)   # random literals (kept raw) and one long match
        raw = np.concatenate([half, half])
    plain = ck.compress_blocks(METHOD_ZSTD, 1, [raw])[0]
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    checked = ck.compress_blocks(METHOD_ZSTD, 1, [raw])[0]
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
    assert np.array_equal(checked, with_checksum(stock, plain, raw))
    at = _payload_offsets(checked, kind)
    assert at is not None, zstd_craft.walk(checked)
    assert _payload_offsets(plain, kind) == at   # the flag bit moves nothing
    pos = at[0] + at[1] // 2
    bad_plain, bad_checked = plain.copy(), checked.copy()
    bad_plain[pos] ^= 0x40
    bad_checked[pos] ^= 0x40
    for path in range(4):
        ck.set_option(cc.OPT_ZSTD_DECODE_PATH, path)
        for n in (1, 24):   # the few-frames route / the batch pipeline with many frames
            outs, st = ck.decompress_blocks(METHOD_ZSTD, [bad_plain] * n, B)
            assert (st == 0).all(), (path, n)   # why the feature exists: a "valid" frame with wrong bytes
            diff = np.nonzero(outs[0] != raw)[0]
            assert len(diff) >= 1 and (kind != "raw" or len(diff) == 1), (path, len(diff))
            outs, st = ck.decompress_blocks(METHOD_ZSTD, [bad_checked] * n + [checked], B)
            assert (st[:n] == cc.E_CORRUPT).all() and st[n] == 0, (path, n, st)
            assert np.array_equal(outs[n], raw)
        assert ck.decompress_block(METHOD_ZSTD, bad_checked, B) is None, path
    if stock.zstd is not None:
        n, out = stock.zstd_decompress(bad_plain, B)
        assert n == B and not np.array_equal(out, raw)
        assert stock.zstd_decompress(bad_checked, B)[0] == -1


@pytest.mark.parametrize("segment", [0, 32768])
def test_write_verification_accepts_checksummed_frames(ck, oracle, stock, segment):
    B = 131072
    raws = [oracle.synth(61, i, B, i % 5) for i in range(10)]
    ck.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    ck.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, segment)
    ck.set_option(cc.OPT_ENCODE_VERIFY, 1)
    got = ck.compress_blocks(METHOD_ZSTD, 1, raws)   # raises on CRYO_E_VERIFY
    ck.set_option(cc.OPT_ENCODE_VERIFY, 0)
    assert all(np.array_equal(g, h) for g, h in zip(got, ck.compress_blocks(METHOD_ZSTD, 1, raws)))
    if not segment:
        assert all(np.array_equal(g, expected(stock, oracle, r, 1)) for g, r in zip(got, raws))
