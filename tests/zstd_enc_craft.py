"""Crafted inputs for the zstd encoders, placed at the edges of the 64-lane strides (tests/test_gpu_zstd_encode_craft.py,
tests/test_zstd_encode_craft_cpu.py).  Test infrastructure only.

The encoders mirror a scalar algorithm (oracle/zstd_enc_oracle.c) with the work of a step shared across the 64 lanes of a
wave: candidates grow 64 bytes at a time, tables are caught up 64 positions at a time, prices and histograms are taken 64
entries at a time.  The scalar mirror has no edge at 64, so an input tests that geometry only where a match length, a
literal run, a distance or the distance to the block's end is 63, 64 or 65, a multiple of 64, one past a strategy's
targetLength, or at the optimal parser's table size (kOptNum = 4096).  sweep_block() puts one match of a chosen length at
a chosen distance, a chosen number of literals behind an earlier match and a chosen number of bytes before the block's
end, in a background no encoder can compress by matching; the lists below walk each of the four around those edges.

    sweep_block(seed, B, L, D, R, tail)   one block
    sweep_cases(B)                        the fixed list of (L, D, R, tail) for a block size, cases that do not fit dropped
    LONG_B, long_cases()                  matches around kOptNum in 16 KiB blocks
    mixed_frames()                        frames of several 128 KiB zstd blocks whose blocks differ in kind
    first_block(frame)                    (block type, number of sequences) of a frame's first block
"""
import functools

import numpy as np

SEED = 20250614                 # fixes the background of every block and the random combinations of the case list
N_RANDOM = 800                  # random combinations of the four axes, behind the single-axis sweeps
BASE = 64                       # the base case: L = D = R = tail = 64
SWEEP_SIZES = (4096, 1024, 1025)    # 1024 | 1025: ZSTD_PREDEF_THRESHOLD, where the optimal parser's first statistics change
LEAD_LEN, LEAD_DIST = 40, 200   # the leading match
ALPHABET = 64

# targetLength of every level >= 11 in the four parameter tables of libzstd 1.4.8 (and `sufficient` of the optimal parser)
TARGET_LENGTHS = (12, 16, 24, 32, 48, 64, 128, 256, 512, 999)

L_AXIS = tuple(sorted(set(range(3, 10)) | {11, 12, 13}
                      | {64 * k + d for k in range(1, 9) for d in (-2, -1, 0, 1, 2) if 64 * k + d <= 513}
                      | {t + d for t in TARGET_LENGTHS for d in (-1, 0, 1)}))
D_AXIS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 63, 64, 65, 127, 128, 129, 1000)
R_AXIS = (0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 66, 128)
TAIL_AXIS = tuple(range(10)) + (12, 31, 32, 33, 63, 64, 65, 128)

LONG_B = 16384
LONG_L = (4093, 4094, 4095, 4096, 4097, 4098, 4099, 8190)      # ml > kOptNum, cur + max_ml >= kOptNum, sufficient = 4095
LONG_D = (1, 3, 64, 5000)
LONG_R = (0, 64)
LONG_TAIL = (0, 1, 64)

ZSTD_BLOCK = 131072             # ZSTD_BLOCKSIZE_MAX
MIXED_LEVELS = (1, 3, 5, 7, 9, 12, 13, 16, 17, 19, 22)      # one per strategy and size class of blocks above 256 KiB


def fits(B, L, D, R, tail):
    """the match under test starts at p = B - tail - L; its source and the leading match's source lie inside the block"""
    p = B - tail - L
    return p - D >= 0 and p - R - LEAD_LEN - LEAD_DIST >= 0


def sweep_block(seed, B, L, D, R, tail):
    """B bytes over a 64-symbol alphabet (random bytes would come out as a raw block, which hides every sequence decision)
    with a leading match of 40 bytes at distance 200 that ends R bytes before the match under test, and the match under test:
    L bytes at distance D, copied byte by byte (D < L overlaps), ending `tail` bytes before the block's end.  The byte after
    each match, and the byte in front of the second when R > 0, differs from the byte that would continue the match: it is
    that byte XOR 0x80, outside the alphabet."""
    assert fits(B, L, D, R, tail), (B, L, D, R, tail)
    x = np.random.default_rng(seed).integers(0, ALPHABET, B).astype(np.uint8)
    p = B - tail - L
    q = p - R                                   # the leading match is [q - 40, q)
    x[q - LEAD_LEN:q] = x[q - LEAD_LEN - LEAD_DIST:q - LEAD_DIST].copy()
    if R > 0:
        x[q] = x[q - LEAD_DIST] ^ 0x80
        # R = 1: one byte ends the first match and fronts the second; both bytes it must differ from lie in the alphabet
        x[p - 1] = x[p - 1 - D] ^ 0x80
    if D >= L:
        x[p:p + L] = x[p - D:p - D + L].copy()
    else:
        period = x[p - D:p].copy()
        x[p:p + L] = np.resize(period, L)
    if tail > 0:
        x[p + L] = x[p + L - D] ^ 0x80
    return x


def _case_list():
    cases = []
    for L in L_AXIS:
        cases.append((L, BASE, BASE, BASE))
    for D in D_AXIS:
        cases.append((BASE, D, BASE, BASE))
    for R in R_AXIS:
        cases.append((BASE, BASE, R, BASE))
    for tail in TAIL_AXIS:
        cases.append((BASE, BASE, BASE, tail))
    rng = np.random.default_rng(SEED)
    for _ in range(N_RANDOM):
        cases.append(tuple(int(rng.choice(axis)) for axis in (L_AXIS, D_AXIS, R_AXIS, TAIL_AXIS)))
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return tuple(out)


CASES = _case_list()


def sweep_cases(B):
    """the case list at block size B: every case of CASES that fits"""
    return tuple(c for c in CASES if fits(B, *c))


def long_cases():
    return tuple((L, D, R, tail) for L in LONG_L for D in LONG_D for R in LONG_R for tail in LONG_TAIL)


@functools.lru_cache(maxsize=None)
def blocks(B):
    """(cases, blocks) of a block size: the sweep list at SWEEP_SIZES, the long-match list at LONG_B.  Block i's background
    has the seed SEED + i, so no two blocks of a batch share one.  The arrays are read-only: they are shared."""
    cases = long_cases() if B == LONG_B else sweep_cases(B)
    out = []
    for i, c in enumerate(cases):
        a = sweep_block(SEED + i, B, *c)
        a.setflags(write=False)
        out.append(a)
    return cases, tuple(out)


# ---------------- frames of several zstd blocks ----------------
_WORDS = ("block", "tuple", "page", "relation", "scan", "index", "offset", "the", "of", "and", "to", "in", "is", "a", "cold",
          "storage", "column", "vacuum", "xid", "chain", "frame", "window", "literal", "sequence", "match", "table", "level",
          "repeat", "header", "with", "for", "not", "null", "integer", "timestamp", "2021-03-04", "0.125", "select", "from",
          "where", "order", "by", "limit", "insert", "into", "values", "compressed", "archive")


def _text(rng, n):
    """n bytes of words from a short list, separated by spaces, with a line end now and then"""
    words = [w.encode() for w in _WORDS]
    parts, have = [], 0
    while have < n:
        w = words[int(rng.integers(0, len(words)))] + (b"\n" if rng.integers(0, 12) == 0 else b" ")
        parts.append(w)
        have += len(w)
    return np.frombuffer(b"".join(parts)[:n], np.uint8).copy()


def _random(rng, n):
    return rng.integers(0, 256, n).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def mixed_frames():
    """eight (name, bytes) inputs of more than one 128 KiB zstd block whose blocks differ in kind: repeat offsets, the entropy
    tables' repeat modes and the optimal parser's statistics carry across raw, RLE and compressed blocks, and btultra2 runs
    its first block twice.  Read-only arrays."""
    K = ZSTD_BLOCK
    rng = np.random.default_rng(SEED + 1)
    out = []
    # compressed | raw | RLE | compressed
    out.append(("text|random|zeros|text", np.concatenate([_text(rng, K), _random(rng, K), np.zeros(K, np.uint8),
                                                          _text(rng, 443216 - 3 * K)])))
    # RLE | compressed | RLE of another byte
    out.append(("zeros|text|run", np.concatenate([np.zeros(K, np.uint8), _text(rng, K), np.full(K, 0x41, np.uint8)])))
    # raw | compressed, the second block one byte over a block
    out.append(("random|text", np.concatenate([_random(rng, K), _text(rng, K + 1)])))
    # a 4000-byte match laid across the block edge, its source 50 000 bytes back
    a = rng.integers(0, ALPHABET, 2 * K).astype(np.uint8)
    a[K - 1700:K + 2300] = a[K - 51700:K - 47700].copy()
    a[K + 2300] = a[K - 47700] ^ 0x80
    out.append(("match across the edge", a))
    # the second block repeats the first: every match at distance 131 072
    a = _text(rng, K)
    out.append(("second block repeats the first", np.concatenate([a, a])))
    # runs across the edge with two odd bytes at it
    a = np.full(262149, 0x20, np.uint8)
    a[K - 1], a[K] = 0x01, 0x02
    a[K + 70000:] = 0x7E
    out.append(("runs across the edge", a))
    # a 60 000-byte copy into the third block from the first
    a = np.concatenate([_text(rng, K), rng.integers(0, ALPHABET, K).astype(np.uint8), _text(rng, K)])
    a[2 * K + 30000:2 * K + 90000] = a[5000:65000].copy()
    out.append(("copy into the third block from the first", a))
    # three blocks of 3-byte words from a 16-word list with a random byte between them
    words = rng.integers(0, 256, (16, 3)).astype(np.uint8)
    n = 3 * K // 4
    a = np.concatenate([words[rng.integers(0, 16, n)], _random(rng, n).reshape(n, 1)], axis=1).reshape(-1)
    out.append(("3-byte words", a))
    for _, a in out:
        assert a.dtype == np.uint8 and a.nbytes > K
        a.setflags(write=False)
    return tuple(out)


def mixed_by_size():
    """{size: [(name, bytes)]}: a compress call takes blocks of one size"""
    groups = {}
    for name, a in mixed_frames():
        groups.setdefault(a.nbytes, []).append((name, a))
    return groups


# ---------------- a peek into a frame ----------------
BLOCK_RAW, BLOCK_RLE, BLOCK_COMPRESSED = 0, 1, 2


def first_block(frame):
    """(block_type, n_sequences) of a zstd frame's first block: the frame header, the block header, the literals section
    header and the sequence count are read, nothing else; n_sequences is 0 for a raw or RLE block"""
    f = bytes(np.asarray(frame, dtype=np.uint8))
    assert f[:4] == b"\x28\xb5\x2f\xfd", "not a zstd frame"
    fhd = f[4]
    single, dict_flag, fcs_flag = (fhd >> 5) & 1, fhd & 3, fhd >> 6
    assert fhd & 0x08 == 0, "reserved bit"
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[dict_flag] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    bh = f[pos] | (f[pos + 1] << 8) | (f[pos + 2] << 16)
    btype, bsize = (bh >> 1) & 3, bh >> 3
    pos += 3
    assert btype != 3, "reserved block type"
    if btype != BLOCK_COMPRESSED:
        return btype, 0
    end = pos + bsize
    ltype, fmt = f[pos] & 3, (f[pos] >> 2) & 3
    if ltype < 2:                               # raw / RLE literals: 5-, 12- or 20-bit regenerated size
        hdr = (1, 2, 1, 3)[fmt]
        word = int.from_bytes(f[pos:pos + hdr], "little")
        regen = word >> (3 if hdr == 1 else 4)
        payload = regen if ltype == 0 else 1
    else:                                       # Huffman literals, with a tree or without: 10-, 14- or 18-bit sizes
        hdr, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[fmt]
        word = int.from_bytes(f[pos:pos + hdr], "little")
        payload = (word >> (4 + bits)) & ((1 << bits) - 1)
    pos += hdr + payload
    assert pos < end, "literals run past the block"
    b0 = f[pos]
    if b0 < 128:
        nseq = b0
    elif b0 < 255:
        nseq = ((b0 - 128) << 8) + f[pos + 1]
    else:
        nseq = f[pos + 1] + (f[pos + 2] << 8) + 0x7F00
    return btype, nseq
