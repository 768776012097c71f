"""Crafted inputs and stream checkers for the segment-parallel encoders (CRYO_OPT_ENCODE_SEGMENT_BYTES = S; test
infrastructure).

A segment stream has no oracle that states its bytes: the contract is a valid stream that decodes to the input.  The rules
the segment encoders add all live at the segment boundaries s0 = k * S, so this module builds blocks with repeats, runs,
offset patterns and literal runs placed around them (segment_corpus), and checks what round trips cannot see:
  - lz4_walk(): the sequences of an LZ4 block, rejecting any stream that breaks the block format (offsets 1 .. 65 535 and
    within the output so far, no match starting after B - 12 or ending inside the last 5 bytes, the last sequence ending
    exactly at B, no trailing bytes); lz4_segment_checks(): a match that starts in an interior segment ends by its end.
  - zstd_segment_blocks() / reframe(): a segment block moved into a frame of its own behind raw-block history.  Raw blocks
    leave a decoder at the repeat offsets {1, 4, 8} and without entropy tables, so the block decodes there only if it uses
    nothing of the blocks before it (independence); with only the last W + S bytes as history it decodes only if its
    matches reach back no further (reach).
Deterministic for a given seed; pure Python and numpy."""
import ctypes as C

import numpy as np

import zstd_craft

KIB = 1024
MIB = 1 << 20

# ---------------- the kernels' constants ----------------
# zstd_enc.hip kZSegSeedBytes: `fast` seeds a segment's table from the 16 KiB before it (every second position)
ZSTD_FAST_SEED = 16384
# zstd_enc.hip kZSegSeedBytesDfast / kZSegSeedBytesLazy: the seed window W of dfast .. btlazy2, which zstd_seg_cparams
# clamps to the frame window minus S when W + S exceeds the window
ZSTD_DEEP_SEED = 16384
# lz4_enc2.hip kSegSeedBytes: the LZ4 segment kernel's seed span
LZ4_SEED = 16384
LZ4_MAX_OFFSET = 65535
LZ4_MFLIMIT, LZ4_LASTLITERALS = 12, 5


class LZ4FormatError(ValueError):
    pass


# ---------------- LZ4 ----------------
def lz4_walk(comp, B):
    """the sequences of an LZ4 block of B bytes: [(pos, lit_len, offset, match_len)], pos = where its literals land, the
    last sequence (literals only) as (pos, lit_len, 0, 0).  Parses headers only (the decoders check the bytes); raises
    LZ4FormatError where the stream breaks the block format."""
    b = bytes(comp)
    n, ip, op = len(b), 0, 0
    seqs = []
    append = seqs.append
    while True:
        if ip >= n:
            raise LZ4FormatError("input ends before a token at %d" % ip)
        tok = b[ip]
        ip += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                if ip >= n:
                    raise LZ4FormatError("input ends inside a literal length")
                s = b[ip]
                ip += 1
                ll += s
                if s != 255:
                    break
        if ip + ll > n:
            raise LZ4FormatError("literals past the input at %d" % ip)
        ip += ll
        if ip == n:
            if op + ll != B:
                raise LZ4FormatError("the last sequence ends at %d, not at B = %d" % (op + ll, B))
            append((op, ll, 0, 0))
            return seqs
        mpos = op + ll
        if mpos > B - LZ4_MFLIMIT:
            raise LZ4FormatError("a match starts at %d, after B - 12 (or trailing bytes)" % mpos)
        if ip + 2 > n:
            raise LZ4FormatError("input ends inside an offset")
        off = b[ip] | (b[ip + 1] << 8)
        ip += 2
        ml = tok & 15
        if ml == 15:
            while True:
                if ip >= n:
                    raise LZ4FormatError("input ends inside a match length")
                s = b[ip]
                ip += 1
                ml += s
                if s != 255:
                    break
        ml += 4
        if off == 0:
            raise LZ4FormatError("offset 0 at %d" % mpos)
        if off > mpos:
            raise LZ4FormatError("offset %d past the output (%d bytes) at %d" % (off, mpos, mpos))
        if mpos + ml > B - LZ4_LASTLITERALS:
            raise LZ4FormatError("a match ends at %d, inside the last 5 bytes" % (mpos + ml))
        append((op, ll, off, ml))
        op = mpos + ml


def lz4_segment_checks(seqs, B, S):
    """a match that starts in an interior segment [s0, s1) (s1 < B) ends at or before s1; positions add up to B"""
    total = 0
    for pos, ll, off, ml in seqs:
        assert pos == total, (pos, total)
        total += ll + ml
        if ml:
            m = pos + ll
            s1 = (m // S + 1) * S
            if s1 < B:
                assert m + ml <= s1, ("match crosses an interior segment end", m, ml, s1)
    assert total == B, (total, B)


# ---------------- zstd ----------------
_MAGIC = (0xFD2FB528).to_bytes(4, "little")
RAW_MAX = 128 * KIB


def frame_header_len(b):
    """bytes of a zstd frame header (RFC 8878 3.1.1.1)"""
    fhd = b[4]
    single = (fhd >> 5) & 1
    return 5 + (0 if single else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if single else 0), 2, 4, 8)[fhd >> 6]


def zstd_segment_blocks(frame):
    """(header bytes, [(block bytes with their 3-byte header, last-block bit)]) of a frame, cut where zstd_craft.walk()
    reads its blocks; None where the structure is broken"""
    b = bytes(frame)
    info = zstd_craft.walk(b)
    if info is None:
        return None
    p = frame_header_len(b)
    head = b[:p]
    out = []
    for blk in info["blocks"]:
        ln = 3 + (1 if blk["type"] == "rle" else blk["size"])
        out.append((b[p:p + ln], b[p] & 1))
        p += ln
    return head, out


def wlog_for(nbytes):
    """the smallest window log (>= 10) whose window holds nbytes"""
    w = 10
    while (1 << w) < nbytes:
        w += 1
    return w


def reframe(history, block, wlog):
    """a frame of its own: a header without the single-segment flag, without content size and with a window of 2^wlog
    bytes; `history` as raw blocks (at most min(128 KiB, window) each); then `block` (one block with its header) with its
    last-block bit set"""
    history = bytes(history)
    block = bytearray(block)
    out = bytearray(_MAGIC)
    out.append(0x00)                         # FHD: no content size, not single-segment, no checksum, no dictionary id
    out.append((wlog - 10) << 3)             # window descriptor: exponent only
    step = min(RAW_MAX, 1 << wlog)
    for i in range(0, len(history), step):
        part = history[i:i + step]
        out += ((len(part) << 3) | (0 << 1) | 0).to_bytes(3, "little")
        out += part
    block[0] |= 1
    out += block
    return np.frombuffer(bytes(out), np.uint8).copy()


class ZstdParams(C.Structure):
    _fields_ = [("windowLog", C.c_uint), ("chainLog", C.c_uint), ("hashLog", C.c_uint), ("searchLog", C.c_uint),
                ("minMatch", C.c_uint), ("targetLength", C.c_uint), ("strategy", C.c_int)]


def zstd_cparams(stock, level, B):
    """libzstd's ZSTD_getCParams(level, B, 0): (windowLog, strategy) -- what zstd_fast_cparams mirrors"""
    Z = stock.zstd
    Z.ZSTD_getCParams.restype = ZstdParams
    Z.ZSTD_getCParams.argtypes = [C.c_int, C.c_ulonglong, C.c_size_t]
    p = Z.ZSTD_getCParams(level, B, 0)
    return p.windowLog, p.strategy


def zstd_levels(stock, B):
    """{strategy: the lowest level of 1 .. 22 that has it at blocks of B bytes}, strategies 1 `fast` .. 6 `btlazy2`"""
    out = {}
    for level in range(1, 23):
        st = zstd_cparams(stock, level, B)[1]
        if st <= 6:
            out.setdefault(st, level)
    return out


def zstd_seed_window(strategy, wlog, S):
    """W: the bytes before a segment its tables are seeded from (zstd_seg_cparams)"""
    if strategy == 1:
        return ZSTD_FAST_SEED
    w = ZSTD_DEEP_SEED
    win = 1 << wlog
    if w + S > win:
        w = win - S if win > S else 0
    return w


def zstd_structure_checks(frame, ident_head, B, S):
    """ceil(B / S) blocks, the last-block bit on the final one only, no treeless literals, no Repeat-mode sequence tables,
    the identical path's frame header"""
    info = zstd_craft.walk(frame)
    assert info is not None and info["end"] == len(frame), "broken frame"
    nseg = -(-B // S)
    assert len(info["blocks"]) == nseg, (len(info["blocks"]), nseg)
    head, blocks = zstd_segment_blocks(frame)
    assert [last for _, last in blocks] == [0] * (nseg - 1) + [1]
    for k, blk in enumerate(info["blocks"]):
        assert blk["type"] != "reserved" and not blk.get("broken"), (k, blk)
        if blk["type"] == "compressed":
            assert blk["lit"] != "treeless", (k, blk)
            assert blk["modes"] is None or "repeat" not in blk["modes"], (k, blk)
    assert head == bytes(ident_head[:len(head)]) and frame_header_len(bytes(ident_head)) == len(head)


def _decodes_to(dec, frame, want):
    r, out = dec(frame, len(want), fill=0x5A)
    return r == len(want) and np.array_equal(out, want)


def zstd_independence_failures(frame, raw, S, decoders, ks=None):
    """the segments k whose block, moved behind raw-block history raw[:s0], does not decode to raw[:s1] in every one of
    `decoders` (callables like Oracle.zstd_decompress)"""
    B = raw.nbytes
    _, blocks = zstd_segment_blocks(frame)
    wlog = wlog_for(B)
    bad = []
    for k in (range(len(blocks)) if ks is None else ks):
        s0, s1 = k * S, min(B, (k + 1) * S)
        f = reframe(raw[:s0], blocks[k][0], wlog)
        if not all(_decodes_to(d, f, raw[:s1]) for d in decoders):
            bad.append(k)
    return bad


def zstd_reach_failures(frame, raw, S, W, decoders, ks=None):
    """the segments k whose block, behind only the last min(s0, W + S) bytes, does not decode to raw[s0 - h:s1]"""
    B = raw.nbytes
    _, blocks = zstd_segment_blocks(frame)
    bad = []
    for k in (range(len(blocks)) if ks is None else ks):
        s0, s1 = k * S, min(B, (k + 1) * S)
        h = min(s0, W + S)
        f = reframe(raw[s0 - h:s0], blocks[k][0], wlog_for(h + S))
        if not all(_decodes_to(d, f, raw[s0 - h:s1]) for d in decoders):
            bad.append(k)
    return bad


def segment_sample(nseg, seed, cap=24):
    """segments to check: all of them up to `cap`, else the first 8, the last 4 and a seeded sample of the rest"""
    if nseg <= cap:
        return list(range(nseg))
    rng = np.random.default_rng([seed, nseg])
    mid = rng.choice(np.arange(8, nseg - 4), size=cap - 12, replace=False)
    return sorted(set(range(8)) | set(range(nseg - 4, nseg)) | {int(x) for x in mid})


def effectiveness_bound(P, B, S, lz4):
    """a periodic block of period P: the whole block is about P literals plus a small cost per segment (LZ4 adds its
    255-byte match-length runs, which any encoder pays); a segment that sees no earlier segment re-emits P literals"""
    nseg = -(-B // S)
    return 1.25 * P + 64 * nseg + (B // 255 if lz4 else 0)


# ---------------- the crafted corpus ----------------
STRADDLE_AT = [0, 1, 3, 4, 5, 7, 8, 12]          # the copy starts this many bytes before s0


def straddle_distances(W):
    return [1, 2, 3, 4, 8, W - 1, W, W + 1, 65535, 65536]


RUN_KINDS = [("byte", b"\x41"), ("zeros", b"\x00"), ("period2", b"\x5a\xc3"), ("period3", b"\x01\x02\x03"),
             ("period7", b"\x10\x32\x54\x76\x98\xba\xdc")]
CARRY_TOTALS = [13, 14, 15, 16, 268, 269, 270, 271, 523, 524, 525, 526]
PERIODS = [61, 1000, 8191]


def boundaries(B, S, rng, cap):
    ks = list(range(1, -(-B // S)))
    if len(ks) > cap:
        ks = sorted(int(k) for k in rng.choice(ks, size=cap, replace=False))
    return ks


def _copy(a, dst, src, n):
    """a[dst:dst + n] = the bytes a decoder writes for a match of offset dst - src (overlapping copies repeat)"""
    d = dst - src
    if d >= n:
        a[dst:dst + n] = a[src:src + n]
    else:
        for i in range(0, n, d):
            m = min(d, n - i)
            a[dst + i:dst + i + m] = a[src:src + m]


def _differ(a, i, v):
    """make a[i] differ from v (a random byte could repeat the run before it)"""
    if a[i] == v:
        a[i] ^= 0x80


def _build(B, S, seed, W, cap):
    rng = np.random.default_rng([seed, B, S])
    noise = lambda: rng.integers(0, 256, B, dtype=np.uint8)   # noqa: E731
    out = []
    ks = boundaries(B, S, rng, cap)
    nseg = -(-B // S)

    # straddling repeats: the copy starts STRADDLE_AT before s0, its source a menu distance behind
    for variant in range(2):
        a, feats = noise(), []
        dists = straddle_distances(W)
        for j, k in enumerate(ks):
            s0 = k * S
            at = STRADDLE_AT[(j + variant * 3) % len(STRADDLE_AT)]
            dist = dists[(j * 3 + variant) % len(dists)]
            dst = s0 - at
            n = min(48 + 37 * ((j + variant) % 4), S // 2, B - dst)
            if dist > dst or n < 4:
                dist = dists[j % 5]
                if dist > dst:
                    continue
            _copy(a, dst, dst - dist, n)
            feats.append("copy@%d<%d+%d" % (dst, dst - dist, n))
        out.append(("straddle/%d" % variant, a, feats))

    # long runs over three or more segments (or to the block's end): one block per kind
    for name, pat in RUN_KINDS:
        a = noise()
        start = S // 2 + 3
        n = min(3 * S + 17, B - start)
        p = np.frombuffer(pat * (-(-n // len(pat))), np.uint8)[:n]
        a[start:start + n] = p
        if start + n < B:
            _differ(a, start + n, a[start + n - len(pat)])
        out.append(("run/" + name, a, ["period%d@%d+%d" % (len(pat), start, n)]))
    a = noise()
    start = max(1, S - 7)
    a[start:] = 0
    out.append(("run/zeros_to_end", a, ["period1@%d+%d" % (start, B - start)]))

    # repeat-offset traps: segment k - 1 ends on matches of offsets 3, 5, 9, segment k opens on runs of periods 1, 4, 8
    # (the default reps); the first match of k repeats the offset of the last of k - 1; two offsets alternate back to back
    a, feats = noise(), []
    for k in ks:
        s0 = k * S
        if s0 < 100 or s0 + 100 > B:
            continue
        p = s0 - 90
        for off in (3, 5, 9):
            p += 6
            _copy(a, p, p - off, 24)
            feats.append("copy@%d<%d+%d" % (p, p - off, 24))
            p += 24
        q = s0 + 2
        for off in (1, 4, 8):
            _copy(a, q, q - off, 24)
            feats.append("copy@%d<%d+%d" % (q, q - off, 24))
            q += 24 + 5
    out.append(("reps/default_trap", a, feats))
    a, feats = noise(), []
    for j, k in enumerate(ks):
        s0 = k * S
        off = 300 + 17 * (j % 7)
        if s0 < off + 64 or s0 + 64 > B:
            continue
        _copy(a, s0 - 40, s0 - 40 - off, 32)
        _copy(a, s0 + 3, s0 + 3 - off, 32)
        feats += ["copy@%d<%d+32" % (s0 - 40, s0 - 40 - off), "copy@%d<%d+32" % (s0 + 3, s0 + 3 - off)]
    out.append(("reps/same_offset", a, feats))
    a, feats = noise(), []
    for j, k in enumerate(ks):
        s0 = k * S
        oa, ob = 40 + (j % 5), 100 + 3 * (j % 4)
        if s0 < 400 or s0 + 64 > B:
            continue
        p = s0 - 64
        for i in range(8):
            off = oa if i % 2 == 0 else ob
            _copy(a, p, p - off, 16)
            feats.append("copy@%d<%d+16" % (p, p - off))
            p += 16
    out.append(("reps/alternate", a, feats))

    # literal runs carried across a boundary: segment k - 1's last match (a run) ends t bytes before s0, segment k's first
    # match (a copy of 48 bytes from 700 before s0, found through the seeded table) starts u bytes after it; t + u on both
    # sides of the 15 / 270 / 525 steps of the LZ4 length code
    a, feats = noise(), []
    for j, k in enumerate(ks):
        s0 = k * S
        tot = CARRY_TOTALS[j % len(CARRY_TOTALS)]
        t = [0, 1, tot // 2, tot - 2][(j // len(CARRY_TOTALS)) % 4]
        u = tot - t
        src = s0 - 700
        if src < 1 or s0 + u + 49 > B:
            continue
        c1 = int(a[s0 - t - 65]) ^ 0x33
        a[s0 - t - 64:s0 - t] = c1
        _differ(a, s0 - t, c1)
        a[s0 + u:s0 + u + 48] = a[src:src + 48]
        _differ(a, s0 + u - 1, a[src - 1])
        _differ(a, s0 + u + 48, a[src + 48])
        feats.append("carry@%d:%d+%d" % (s0, t, u))
    out.append(("carry/thresholds", a, feats))
    # random over many segments, then a compressible last segment; and all random
    a = noise()
    last0 = (nseg - 1) * S
    a[last0:] = 0
    out.append(("carry/random_then_zeros", a, ["period1@%d+%d" % (last0, B - last0)]))
    out.append(("carry/random", noise(), []))

    # seeding effectiveness: random data of period P
    for P in PERIODS:
        if P * 2 > B:
            P = max(8, B // 4)
        a = np.resize(rng.integers(0, 256, P, dtype=np.uint8), B)
        out.append(("periodic/%d" % P, a, ["period%d@0+%d" % (P, B)]))
    return out


def segment_corpus(B, S, seed, W=ZSTD_FAST_SEED, cap=64):
    """[(name, block)]: blocks of B bytes over random background with features placed around the boundaries s0 = k * S
    (all of them, or a seeded sample of `cap`): straddling repeats, long runs, repeat-offset traps, carried literal runs,
    random stretches, periodic data.  corpus_features() states where every feature sits."""
    return [(name, a) for name, a, _ in _build(B, S, seed, W, cap)]


def corpus_features(B, S, seed, W=ZSTD_FAST_SEED, cap=64):
    """{name: [feature]}: `copy@dst<src+n` (block[dst:dst + n] is what a match of offset dst - src writes there),
    `periodP@at+n` (block[at:at + n] has period P), `carry@s0:t+u` (a run ends t bytes before s0, a 48-byte copy of
    block[s0 - 700:] starts u bytes after it)"""
    return {name: f for name, _, f in _build(B, S, seed, W, cap)}


def check_features(block, feats):
    """every feature of a block is where its name says"""
    for f in feats:
        if f.startswith("copy@"):
            dst, rest = f[5:].split("<")
            src, n = rest.split("+")
            dst, src, n = int(dst), int(src), int(n)
            d = dst - src
            for i in range(n):
                assert block[dst + i] == block[dst + i - d], f
        elif f.startswith("period"):
            per, rest = f[6:].split("@")
            at, n = rest.split("+")
            per, at, n = int(per), int(at), int(n)
            seg = block[at:at + n]
            assert np.array_equal(seg[per:], seg[:n - per]), f
        elif f.startswith("carry@"):
            s0, rest = f[6:].split(":")
            t, u = rest.split("+")
            s0, t, u = int(s0), int(t), int(u)
            c1, src, dst = block[s0 - t - 1], s0 - 700, s0 + u
            assert (block[s0 - t - 64:s0 - t] == c1).all() and block[s0 - t] != c1, f
            assert np.array_equal(block[dst:dst + 48], block[src:src + 48]), f
            assert block[dst - 1] != block[src - 1] and block[dst + 48] != block[src + 48], f
        else:
            raise AssertionError(f)
