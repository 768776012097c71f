"""Raw blocks above 1 MiB for tests/test_large_blocks_cpu.py and tests/test_gpu_large_blocks.py (test infrastructure, no GPU).

Deterministic, seeded builders of one raw block of B bytes each, and the size classes the two test files walk.  Every size is
there for a reason that lies in the kernels:

LZ4 encode   1 MiB + 1 .. 16 MiB take k_lz4_enc2<2048, 8, true, false> (8 high position bits, no tag bits); above 16 MiB the
             serial kernel.
zstd encode  the window of level 2 is smaller than the block from 1 MiB + 1 on, of levels 3-9 from 2 MiB + 1, of levels
             10-16 from 4 MiB + 1, of levels 17-19 from 8 MiB + 1; table entries keep 32 - ib tag bits, ib = 32 - clz(B).
decode       LZ4 and zstd switch route at 2 MiB per block and 64 MiB per call; the zstd planner takes frames of fewer than
             254 blocks (253 x 128 KiB and 8 bytes more lie on either side); offset codes 25 and 26 need 72 MiB.
"""
import numpy as np

import oracle_lib
import stress_gpu

KIB, MIB = 1 << 10, 1 << 20
SEED = 0x1a7

LZ4_ENC = [MIB + 1, MIB + 8, 2 * MIB + 5, 4 * MIB, 16 * MIB, 16 * MIB + 1, 72 * MIB + 24]
ZSTD_ENC = [MIB + 1, 2 * MIB, 2 * MIB + 1, 4 * MIB + 24, 8 * MIB + 1, 72 * MIB + 24]
DEC = [MIB + 8, 2 * MIB, 2 * MIB + 8, 4 * MIB + 24, 16 * MIB + 8, 253 * 128 * KIB, 253 * 128 * KIB + 8, 72 * MIB + 24]
ZSTD_ONLY_DEC = (253 * 128 * KIB, 253 * 128 * KIB + 8)          # frames of 253 and 254 zstd blocks
FAR = 72 * MIB + 24                                             # the smallest size far_window() builds
# crafted LZ4 streams per decode size: lz4_craft.corpus(B, n, CRAFTED_LZ4_SEED) holds accepted and rejected streams for each
DEC_CRAFTED_LZ4 = {MIB + 8: 12, 2 * MIB: 12, 2 * MIB + 8: 12, 4 * MIB + 24: 8, 16 * MIB + 8: 4, 72 * MIB + 24: 4}
CRAFTED_LZ4_SEED = 1

# zstd levels of the encode tests and their strategy in libzstd's table for sources above 256 KiB: one level or more of each,
# fast (-5, 1), dfast (3, 4), greedy (6), lazy (7), lazy2 (8, 10, 12), btlazy2 (13), btopt (16), btultra (18), btultra2 (19, 22)
ZSTD_STRATEGY = {-5: 1, 1: 1, 3: 2, 4: 2, 6: 3, 7: 4, 8: 5, 10: 5, 12: 5, 13: 6, 16: 7, 18: 8, 19: 9, 22: 9}
ZSTD_LEVELS = sorted(ZSTD_STRATEGY)

SYNTH = ["wide", "narrow", "int4", "random", "zeros"]
CHUNK = 3000


def _rng(name, B):
    return np.random.default_rng([SEED, sum(name.encode()), B])


def synth(oracle, dist, B):
    return oracle.synth(SEED, dist, B, dist)


def far_repeat_positions(B):
    """where far_repeats() copies its chunk: 100 bytes below and 100 bytes above each anchor"""
    anchors = [1 << 16, 1 << 17] + [1 << k for k in range(20, 32) if (1 << k) <= B] + [B // 2]
    pos = []
    for a in anchors:
        pos += [a - CHUNK - 100, a + 100]
    pos.append(B - CHUNK - 100)
    return sorted({p for p in pos if p >= CHUNK and p + CHUNK <= B})


def far_repeats(B):
    """random bytes with the first 3 000 copied to just below and just above 2^16, 2^17, every power of two from 2^20 up to
    B, B / 2, and to B - 3 100"""
    a = _rng("far_repeats", B).integers(0, 256, B, dtype=np.uint8)
    chunk = a[:CHUNK].copy()
    for p in far_repeat_positions(B):
        a[p:p + CHUNK] = chunk
    return a


def long_runs(B):
    z = np.zeros(B, np.uint8)
    z[B // 3:B // 3 + 100] = _rng("long_runs", B).integers(0, 256, 100, dtype=np.uint8)
    return z


def periodic_noise(B):
    t = np.frombuffer((b"abcdefghij" * (B // 10 + 1))[:B], np.uint8).copy()
    t[::997] = _rng("periodic_noise", B).integers(0, 256, len(t[::997]), dtype=np.uint8)
    return t


def text_noise(B):
    w = np.frombuffer((b"the quick brown fox jumps over the lazy dog, " * (B // 45 + 1))[:B], np.uint8).copy()
    w[_rng("text_noise", B).integers(0, B, B // 50)] = 0x5A
    return w


def incompressible(B):
    return _rng("incompressible", B).integers(0, 256, B, dtype=np.uint8)


def far_window(B):
    """zeros except 1 MiB of random bytes at 0, copied to 40 MiB and to B - 1 MiB: the only matches for the copies lie
    40 MiB and B - 41 MiB (about 31 MiB) or B - 1 MiB (about 71 MiB) back"""
    assert B >= FAR
    a = np.zeros(B, np.uint8)
    a[:MIB] = _rng("far_window", B).integers(0, 256, MIB, dtype=np.uint8)
    a[40 * MIB:41 * MIB] = a[:MIB]
    a[B - MIB:] = a[:MIB]
    return a


def far_window_split(B):
    """far_window() with only the first half of the random MiB copied to 40 MiB: the second half of the copy at B - 1 MiB
    has one possible match, B - 1 MiB (about 71 MiB) back.  In far_window() itself the compressors serve the last copy
    from the nearer one at 40 MiB (offset code 24), so that no code of 26 occurs in its frames."""
    a = far_window(B)
    a[40 * MIB + MIB // 2:41 * MIB] = 0
    return a


CRAFTED = {"far_repeats": far_repeats, "long_runs": long_runs, "periodic_noise": periodic_noise, "text_noise": text_noise,
           "incompressible": incompressible}
BUILDERS = SYNTH + list(CRAFTED)


def build(oracle, name, B):
    if name in SYNTH:
        return synth(oracle, SYNTH.index(name), B)
    if name in ("far_window", "far_window_split"):
        return far_window(B) if name == "far_window" else far_window_split(B)
    return CRAFTED[name](B)


def blocks(oracle, B, names=None):
    """[(name, block)] of every builder (or the named ones) at size B"""
    return [(n, build(oracle, n, B)) for n in (names or BUILDERS)]


def require_stock():
    """the stock libraries the codec promises to equal, or a failure (never a skip)"""
    import pytest
    s = oracle_lib.StockLibs()
    if s.lz4 is None or s.zstd is None:
        pytest.fail("liblz4.so.1 and libzstd.so.1 are needed: they are the reference above 1 MiB")
    if s.lz4_version != "1.9.3" or s.zstd_version != "1.4.8":
        pytest.fail("stock libraries report %s / %s, the codec is pinned to 1.9.3 / 1.4.8" % (s.lz4_version, s.zstd_version))
    s.zstd_check_param_bounds()
    return s


def far_frames(stock, B=FAR):
    """[(name, raw block, frame)] of far_window(B) and far_window_split(B): windowLog 27 at levels 1 and 3 (offsets of 40 MiB
    and more are in reach), and far_window(B) by plain ZSTD_compress level 1"""
    out = []
    for bname, raw in (("far_window", far_window(B)), ("far_window_split", far_window_split(B))):
        for lvl in (1, 3):
            f = stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: lvl, oracle_lib.ZSTD_C_WINDOWLOG: 27})
            assert f is not None
            out.append(("%s/wlog27/l%d" % (bname, lvl), raw, f))
        if bname == "far_window":
            out.append(("far_window/plain/l1", raw, stock.zstd_compress(raw, 1)))
    return out


def mutants(name, stream, n):
    """n damaged copies of a stream (stress_gpu.mutate), seeded by its name and length"""
    rng = np.random.default_rng([SEED, sum(name.encode()), len(stream)])
    return [("mutated%d/%s" % (k, name), stress_gpu.mutate(rng, stream)) for k in range(n)]


# ---------------- the highest offset code of a frame ----------------
class _Bits:
    """the backward bit stream of RFC 8878 4.1: the last byte holds the end mark, bits are read from the top down"""

    def __init__(self, b):
        assert b and b[-1], "no end mark"
        self.v = int.from_bytes(b, "little")
        self.n = 8 * (len(b) - 1) + b[-1].bit_length() - 1

    def read(self, k):
        self.n -= k
        if self.n < 0:                                   # reading past the start yields zeros, as in the decoders
            r = (self.v << -self.n) & ((1 << k) - 1) if self.n + k > 0 else 0
            self.v, self.n = 0, 0
            return r
        return (self.v >> self.n) & ((1 << k) - 1)


OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]   # RFC 8878 3.1.1.3.2.2.3


def _fse_read_counts(b, p, max_log):
    """an FSE table description at b[p:] (RFC 8878 4.1.1): (normalised counts, accuracy log, bytes read)"""
    v = int.from_bytes(b[p:p + 64], "little")
    bit = 0

    def take(k):
        nonlocal bit
        r = (v >> bit) & ((1 << k) - 1)
        bit += k
        return r
    log = take(4) + 5
    assert log <= max_log
    remaining, counts = (1 << log) + 1, []
    while remaining > 1:
        nb = remaining.bit_length()
        low_n = (1 << nb) - 1 - remaining
        x = take(nb - 1)
        if x >= low_n:
            x |= take(1) << (nb - 1)
            if x >= (1 << (nb - 1)):
                x -= low_n
        c = x - 1
        remaining -= abs(c)
        counts.append(c)
        if c == 0:
            while True:
                r = take(2)
                counts += [0] * r
                if r != 3:
                    break
    return counts, log, (bit + 7) // 8


def _fse_symbols(counts, log):
    """state -> symbol of the decoding table the counts spread into (RFC 8878 4.1.1)"""
    size = 1 << log
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(counts):
        if c == -1:
            sym[high] = s
            high -= 1
    pos, step = 0, (size >> 1) + (size >> 3) + 3
    for s, c in enumerate(counts):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    return sym


def frame_offset_codes(frame):
    """the set of offset codes that occur in a frame's sequence sections.  Offset tables are walked by their mode: an RLE
    table is its one symbol, a predefined or described table contributes every symbol that a state the stream visits
    decodes to.  The three interleaved state machines (literal length, offset, match length) are all followed, since their
    bits share one stream; no literal is decoded."""
    b = bytes(frame)
    assert int.from_bytes(b[:4], "little") == 0xFD2FB528
    fhd = b[4]
    fcs_flag, single, checksum, did = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    codes, prev = set(), {}
    while True:
        h = int.from_bytes(b[p:p + 3], "little")
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        p += 3
        if btype == 2:
            codes |= _block_offset_codes(b[p:p + bsize], prev)
        p += 1 if btype == 1 else bsize
        if last:
            return codes


LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
              1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _decode_table(counts, log):
    """[(symbol, nbits, baseline)] per state"""
    sym = _fse_symbols(counts, log)
    size = 1 << log
    nxt = [c if c > 0 else 1 for c in counts]
    out = []
    for st in range(size):
        s = sym[st]
        x = nxt[s]
        nxt[s] += 1
        nb = log - (x.bit_length() - 1)
        out.append((s, nb, (x << nb) - size))
    return out


def _block_offset_codes(b, prev):
    b0 = b[0]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt < 2:
        hl = (1, 2, 1, 3)[sf]
        size = b0 >> 3 if hl == 1 else (int.from_bytes(b[:hl], "little") >> 4)
        p = hl + (size if lt == 0 else 1)
    else:
        hl, bits = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
        p = hl + ((int.from_bytes(b[:hl], "little") >> (4 + bits)) & ((1 << bits) - 1))
    s0 = b[p]
    nseq, p = (s0, p + 1) if s0 < 128 else ((((s0 - 128) << 8) + b[p + 1], p + 2) if s0 < 255 else
                                            (b[p + 1] + (b[p + 2] << 8) + 0x7F00, p + 3))
    if nseq == 0:
        return set()
    modes = b[p]
    p += 1
    tabs = {}
    for key, mode, default, dlog, mlog in (("ll", modes >> 6, LL_DEFAULT, 6, 9), ("of", (modes >> 4) & 3, OF_DEFAULT, 5, 8),
                                           ("ml", (modes >> 2) & 3, ML_DEFAULT, 6, 9)):
        if mode == 0:
            tabs[key] = (_decode_table(default, dlog), dlog)
        elif mode == 1:
            tabs[key] = ([(b[p], 0, 0)], 0)
            p += 1
        elif mode == 2:
            counts, log, used = _fse_read_counts(b, p, mlog)
            tabs[key] = (_decode_table(counts, log), log)
            p += used
        else:
            tabs[key] = prev[key]
        prev[key] = tabs[key]
    bs = _Bits(b[p:])
    (llt, lll), (oft, ofl), (mlt, mll) = tabs["ll"], tabs["of"], tabs["ml"]
    ls, os_, ms = bs.read(lll), bs.read(ofl), bs.read(mll)
    codes = set()
    for i in range(nseq):
        lsym, lnb, lbase = llt[ls]
        osym, onb, obase = oft[os_]
        msym, mnb, mbase = mlt[ms]
        codes.add(osym)
        bs.read(osym)                      # an offset code's extra bits are as many as the code
        bs.read(ML_BITS[msym])
        bs.read(LL_BITS[lsym])
        if i + 1 < nseq:
            ls = lbase + bs.read(lnb)
            ms = mbase + bs.read(mnb)
            os_ = obase + bs.read(onb)
    assert bs.n == 0, "sequence bit stream not used up: %d bits left" % bs.n
    return codes


def drop_content_size(frame, B):
    """the same frame without Frame_Content_Size: not single-segment, a window descriptor that covers B instead (what a
    streaming compressor that was not told the size writes); the blocks and the checksum flag stay"""
    fhd = int(frame[4])
    fcs_flag, single, did = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    hdr = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    wlog = max(10, (B - 1).bit_length())
    return np.concatenate([frame[:4], np.array([fhd & 0x04, (wlog - 10) << 3], np.uint8), frame[hdr:]])

