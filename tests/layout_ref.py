"""Reference of the stored-block check's layout rules (include/cryo_codec.h, "checking stored blocks"), in numpy: what
cryo_codec_check_batch must report for a decoded block.  Test infrastructure only.

A block of B bytes (B a multiple of 8, at least 16; fields LE u32): lower at 0, upper at 4, n = (lower - 8) / 8, item i =
(off_i at 8 + 8i, len_i at 12 + 8i), MAXALIGN(x) = (x + 7) & ~7.
  1. HEADER   lower >= 8, (lower - 8) % 8 == 0, n <= 290, lower <= upper <= B, upper == B when n == 0
  2. ITEM i   fails when len_i == 0, off_i + MAXALIGN(len_i) != (B if i == 0 else off_{i-1} as stored), or i == n - 1 and
              off_i != upper
  3. NONZERO  a nonzero byte in [lower, upper) or in a pad [off_i + len_i, off_i + MAXALIGN(len_i))
The first failing class wins: (HEADER, 0), (ITEM, 8 + 8i of the lowest failing i), (NONZERO, lowest such byte); a block that
passes gets (OK, 0xFFFFFFFF), a stream the decoders reject (STREAM, 0xFFFFFFFF)."""
import numpy as np

OK, STREAM, HEADER, ITEM, NONZERO = 0, 1, 2, 3, 4
NONE = 0xFFFFFFFF
MAX_ITEMS = 290


def maxalign(x):
    return (x + 7) & ~7


def check_block(block):
    """(reason, offset) of one decoded block (uint8 array of B bytes)"""
    b = np.ascontiguousarray(block, dtype=np.uint8)
    B = b.size
    assert B % 8 == 0 and B >= 16
    lower, upper = (int(v) for v in b[:8].view("<u4"))
    n = (lower - 8) // 8
    if lower < 8 or (lower - 8) % 8 or n > MAX_ITEMS or not lower <= upper <= B or (n == 0 and upper != B):
        return HEADER, 0
    items = b[8:8 + 8 * n].view("<u4").reshape(n, 2).astype(np.int64)
    off, ln = items[:, 0], items[:, 1]
    prev = np.concatenate([[B], off[:-1]]) if n else np.zeros(0, np.int64)
    bad = (ln == 0) | (off + maxalign(ln) != prev)
    if n:
        bad[n - 1] |= off[n - 1] != upper
    if bad.any():
        return ITEM, 8 + 8 * int(np.argmax(bad))
    nz = np.flatnonzero(b[lower:upper])
    lowest = lower + int(nz[0]) if nz.size else None
    for i in range(n):
        pad = b[off[i] + ln[i]:off[i] + maxalign(ln[i])]
        pz = np.flatnonzero(pad)
        if pz.size:
            at = int(off[i] + ln[i] + pz[0])
            lowest = at if lowest is None else min(lowest, at)
    if lowest is not None:
        return NONZERO, lowest
    return OK, NONE


def decode(oracle, method, comp, B):
    """the oracle's decode of a stream: the B bytes, or None when it does not decode to exactly B bytes"""
    r, out = (oracle.lz4_decompress if method == 0 else oracle.zstd_decompress)(np.asarray(comp, np.uint8), B)
    return out.copy() if r == B else None


def check_stream(oracle, method, comp, B):
    """(reason, offset) of a stored stream: STREAM when the oracle does not decode it to B bytes"""
    raw = decode(oracle, method, comp, B)
    return (STREAM, NONE) if raw is None else check_block(raw)


def _u32(b, at):
    return int(b[at:at + 4].view("<u4")[0])


def _set_u32(b, at, v):
    b[at:at + 4] = np.frombuffer(int(v & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)


def corrupt(block, rng):
    """one seeded corruption of a valid block: a header field, an item, a gap, pad or tuple-body byte, or a mix"""
    b = np.array(block, np.uint8)
    B = b.size
    lower, upper = _u32(b, 0), _u32(b, 4)
    n = (lower - 8) // 8
    kind = int(rng.integers(0, 11))
    if kind == 0:                                   # lower out of range
        _set_u32(b, 0, int(rng.choice([0, 4, 7, lower + 1, lower + 4, upper + 8, 8 + 8 * 291])))
    elif kind == 1:                                 # upper out of range
        _set_u32(b, 4, int(rng.choice([lower - 8, B + 8, B + 1, upper + 4, 0xFFFFFFFF])))
    elif kind == 2 and n:                           # a zero len
        _set_u32(b, 12 + 8 * int(rng.integers(n)), 0)
    elif kind == 3 and n:                           # the slot chain broken at the first, a middle or the last item
        i = int(rng.choice([0, n // 2, n - 1]))
        _set_u32(b, 8 + 8 * i, _u32(b, 8 + 8 * i) + int(rng.choice([8, -8, 1, 0x10000])))
    elif kind == 4 and n:                           # a len changed (within its slot: the pad moves)
        i = int(rng.integers(n))
        _set_u32(b, 12 + 8 * i, _u32(b, 12 + 8 * i) + int(rng.choice([1, -1, -3, 7, 8])))
    elif kind == 5 and upper > lower:               # a gap byte
        b[int(rng.integers(lower, upper))] = int(rng.integers(1, 256))
    elif kind == 6 and n:                           # a pad byte (where the rows have pads)
        i = int(rng.integers(n))
        off, ln = _u32(b, 8 + 8 * i), _u32(b, 12 + 8 * i)
        if ln % 8:
            b[off + ln + int(rng.integers(0, maxalign(ln) - ln))] = int(rng.integers(1, 256))
        else:
            b[int(rng.integers(lower, upper)) if upper > lower else 0] ^= 0x40
    elif kind == 7 and n:                           # a tuple body byte: invisible to the check
        i = int(rng.integers(n))
        off, ln = _u32(b, 8 + 8 * i), _u32(b, 12 + 8 * i)
        b[off + int(rng.integers(0, ln))] ^= 0x5A
    elif kind == 8 and n and upper > lower:         # an item and a gap byte: the item wins
        _set_u32(b, 12 + 8 * int(rng.integers(n)), 0)
        b[int(rng.integers(lower, upper))] = 1
    elif kind == 9:                                 # any byte of the header, the item array or just behind it
        b[int(rng.integers(0, min(lower + 16, B)))] = int(rng.integers(0, 256))
    else:                                           # n = 291 where it fits
        _set_u32(b, 0, 8 + 8 * 291)
    return b
