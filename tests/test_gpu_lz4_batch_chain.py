"""GPU: the batch chain of the indexed LZ4 decoder (csrc/lz4_dec2.hip, csrc/lz4_copy.h) on streams written sequence by
sequence (tests/lz4_craft.py), against the oracle: bytes and status.

What the streams aim at:
  match space -- the per-chunk bases are written by the lane whose dependent match holds byte 64c of match space: matches that
      start or end exactly on a boundary, a boundary inside a 4-byte match, matches of 65 ... 273 bytes over 2-5 boundaries,
      batches that are nothing but dependent matches (64, 128 and 1 536 bytes of them), no dependent match, only a rank-0 one;
  lane_runs -- a run with exactly 16 bytes left is finished by the closing 16-byte copy, except a far one: literal runs and
      independent matches around 16 / 32 / 48 bytes, runs that cross the end of the output ring and of the input ring, far
      matches of exactly 16 and 32 bytes;
  hard stops -- a batch ends in front of a sequence no batch takes (a 255-run in either length, an overlap above 64 bytes, a
      far match above 32), the general path takes that one and the batches resume behind it with entries requested afresh
      or ahead: as the block's first sequence, as lane 0 / 1 / 5 / 63, two in a row, in front of the last sequence, behind a
      short batch; and streams mutated behind a stop, where the verdict is the oracle's.
Every case runs with one wave per block and with two (CRYO_OPT_LZ4_DECODE_WAVES), and with 1 and 4 index walkers."""
import numpy as np
import pytest

import lz4_craft
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD
from pg_cryogen_amd import codec as cc
from test_gpu_decode_conformance import _batch_check, _options, _truth

pytestmark = pytest.mark.gpu

B_SMALL, B_MID, B_BIG = 8192, 32768, 131072
IN_RING = 2048
NEAR1, NEAR2 = 2560, 5120          # a match is "far" from here on: one wave per block (4 KiB ring), two (8 KiB ring)
STOPS = ["ll255", "ml255", "overlap", "far"]


class Blk:
    """a block under construction: sequences (ll, off, ml), bytes written so far, compressed bytes so far"""

    def __init__(self, B, seed):
        self.B, self.rng, self.seqs, self.op, self.cp = B, np.random.default_rng(seed), [], 0, 0
        self.lit_runs = []     # (compressed position, output position, length) of every literal run
        self.marks = []        # compressed position behind every stop()

    def add(self, ll, off, ml):
        assert ml >= 4 and 1 <= off <= self.op + ll, (ll, off, ml, self.op)
        assert self.op + ll + ml <= self.B - 16
        self.lit_runs.append((self.cp + 1 + (0 if ll < 15 else (ll - 15) // 255 + 1), self.op, ll))
        self.seqs.append((ll, off, ml))
        self.op += ll + ml
        self.cp += lz4_craft.csize_of([(ll, off, ml)], 0) - 1
        return self

    def plain(self, n=1, ll=None, ml=None, max_off=1500):
        """n everyday sequences: short or 29-32 byte literal runs, matches of 4-12 bytes at small offsets"""
        r = self.rng
        for _ in range(n):
            a = int(r.choice([0, 0, 1, 3, 8, 14, 29, 30, 31, 32])) if ll is None else ll
            if self.op + a == 0:
                a = 5
            m = int(r.integers(4, 13)) if ml is None else ml
            self.add(a, int(r.integers(1, min(self.op + a, max_off) + 1)), m)
        return self

    def until(self, op):
        """everyday sequences until exactly `op` bytes are written"""
        while self.op < op:
            left = op - self.op
            if left < 60:                  # (an everyday sequence is at most 44 bytes: at least 16 are left behind it)
                self.add(left - 4, int(self.rng.integers(1, min(self.op + left - 4, 1500) + 1)), 4)
            else:
                self.plain()
        assert self.op == op
        return self

    def stop(self, kind):
        """one sequence that no batch takes"""
        if kind == "ll255":
            self.add(15 + 255 + int(self.rng.integers(0, 40)), int(self.rng.integers(1, self.op + 200)), 6)
        elif kind == "ml255":
            ml = 4 + 15 + 255 + int(self.rng.integers(0, 300))
            self.add(3, ml + 7 if self.op + 3 >= ml + 7 else 1, ml)
        elif kind == "overlap":
            self.add(2, int(self.rng.integers(1, 3)), int(self.rng.integers(65, 274)))
        else:
            assert kind == "far" and self.op >= NEAR2 + 100
            self.add(1, int(self.rng.integers(NEAR2, self.op)), int(self.rng.integers(33, 274)))
        self.marks.append(self.cp)
        return self

    def done(self, tail_ll=None):
        """everyday sequences up to the end, then the last literals"""
        if tail_ll is None:
            while self.op < self.B - 120:
                self.plain()
            tail_ll = self.B - self.op
        assert tail_ll == self.B - self.op and tail_ll >= 12
        return np.frombuffer(bytes(lz4_craft.encode(self.seqs, tail_ll, lit_seed=int(self.rng.integers(0, 1 << 30)))), np.uint8).copy()


def _cases(oracle, B, named, accept=True):
    """[(name, stream)] -> [(name, stream, the oracle's block or None)]; crafted (not mutated) streams must be valid"""
    truth = _truth(oracle, METHOD_LZ4, [s for _, s in named], B)
    if accept:
        bad = [n for (n, _), t in zip(named, truth) if t is None]
        assert not bad, ("the oracle rejects a crafted stream", bad)
    return [(n, s, t) for (n, s), t in zip(named, truth)]


def _run(codec, cases, B, waves, walkers, tag):
    with _options(codec, {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_INDEXED, cc.OPT_LZ4_INDEX_WALKERS: walkers,
                          cc.OPT_LZ4_DECODE_WAVES: waves}):
        _batch_check(codec, METHOD_LZ4, cases, B, (tag, B, waves, walkers))


CONFIGS = [(1, 1), (1, 4), (2, 1), (2, 4)]   # (waves, walkers)


# ------------------------------------------------------------------ match space
def _match_space_blocks():
    out = []

    def blk(name, body, B=B_SMALL, lead=3000):
        b = Blk(B, len(out) + 1)
        b.until(lead).stop("overlap")       # the batch under test begins behind a stop, 3 000 bytes into the block
        body(b)
        b.stop("overlap")                  # ... and ends in front of one
        out.append((name, b.done()))

    # eight dependent matches of 8 bytes = 64 bytes of match space, then a match that starts exactly on the boundary
    for k, nm in ((8, "starts_on_64"), (16, "starts_on_128")):
        blk(nm, lambda b, k=k: (b.add(20, 16, 8), [b.add(2, 10, 8) for _ in range(k - 1)], b.add(3, 12, 9), b.add(0, 30, 5)))
        blk(nm.replace("starts", "ends"), lambda b, k=k: (b.add(20, 16, 8), [b.add(2, 10, 8) for _ in range(k - 1)]))
    # 56 + 6 = 62 bytes, then a 4-byte match over bytes 62..65
    blk("boundary_in_4", lambda b: (b.add(20, 16, 8), [b.add(2, 10, 8) for _ in range(6)], b.add(1, 9, 6), b.add(0, 20, 4), b.add(5, 8, 7)))
    # a long dependent match that does not overlap itself, source inside the batch, at match-space position 64 and 60
    for n in (65, 128, 129, 273):
        for first in (8, 4):
            blk("long_%d_at_%d" % (n, 56 + first),
                lambda b, n=n, first=first: (b.add(40, 16, first), [b.add(40, 10, 8) for _ in range(7)], b.add(0, 300, n), b.add(2, 5, 6)))
    # nothing but dependent matches: 64, 128 and 1 536 bytes of match space
    blk("all_dep_64", lambda b: [b.add(0, 3, 4) for _ in range(16)])
    blk("all_dep_128", lambda b: [b.add(0, 5, 8) for _ in range(16)])
    blk("all_dep_1536", lambda b: [b.add(0, 7, 24) for _ in range(64)])
    # no dependent match (every source ends before the batch begins); only a rank-0 one
    blk("no_dep", lambda b: [b.add(10, 2000, 8) for _ in range(20)])
    blk("rank0_only", lambda b: (b.add(10, 4, 8), [b.add(10, 2000, 8) for _ in range(10)]))
    # the same shapes as the first batch of a block
    b = Blk(B_SMALL, 99)
    b.add(40, 16, 8)
    for _ in range(7):
        b.add(40, 10, 8)
    b.add(0, 300, 273)
    out.append(("long_273_first_batch", b.done()))
    return out


@pytest.fixture(scope="module")
def match_space_cases(oracle):
    return _cases(oracle, B_SMALL, _match_space_blocks())


@pytest.mark.parametrize("waves,walkers", CONFIGS)
def test_match_space_chunk_bases(codec, match_space_cases, waves, walkers):
    _run(codec, match_space_cases, B_SMALL, waves, walkers, "match space")


# ------------------------------------------------------------------ literal runs and independent matches
LIT_LENS = [15, 16, 17, 31, 32, 33, 47, 48, 49]


def _crosses(runs, ring):
    """does some run (start, length) cross a multiple of `ring`?"""
    return any(s // ring != (s + n - 1) // ring for s, n in runs if n)


def _run_blocks():
    out = []
    for L in LIT_LENS:
        # a block of runs of L bytes; the matches' lengths cycle so that the runs meet the rings' ends at changing phases
        b = Blk(B_MID, 100 + L)
        i = 0
        while b.op < B_MID - 200:
            b.add(L, int(b.rng.integers(1, min(b.op + L, 1200) + 1)), 4 + (i % 5))
            if i % 7 == 3:
                b.add(0, int(b.rng.integers(1, min(b.op, 1200) + 1)), 5)
            i += 1
        s = b.done(B_MID - b.op)
        runs = [(cp, op, n) for cp, op, n in b.lit_runs if n == L]
        for R in (4096, 8192):
            assert _crosses([(op, n) for _, op, n in runs], R), (L, R)
        for delta in range(0, 128):        # wherever the stream starts inside a 128-byte line
            assert _crosses([(cp + delta, n) for cp, _, n in runs], IN_RING), (L, delta)
        out.append(("lit_%d" % L, s))
    for ML in (16, 17, 32, 33):
        # independent matches: the source ends before the batch begins (offset beyond a batch's 1 536 bytes, inside the ring)
        b = Blk(B_MID, 200 + ML).until(2600)
        i = 0
        while b.op < B_MID - 200:
            b.add(i % 4, int(b.rng.integers(1600, 2500)), ML)
            if i % 5 == 2:
                b.plain()
            i += 1
        out.append(("indep_%d" % ML, b.done(B_MID - b.op)))
    for ML in (16, 32, 31, 20):
        # far matches (source already flushed, for both ring sizes): exactly 16 and 32 bytes have no closing copy to fall back on
        b = Blk(B_MID, 300 + ML).until(6000)
        i = 0
        while b.op < B_MID - 200:
            b.add(i % 3, int(b.rng.integers(NEAR2, min(b.op, 20000))), ML)
            if i % 4 == 1:
                b.add(2, int(b.rng.integers(NEAR1, NEAR2)), ML)     # far for the 4 KiB ring only
            if i % 6 == 2:
                b.plain()
            i += 1
        out.append(("far_%d" % ML, b.done(B_MID - b.op)))
    return out


@pytest.fixture(scope="module")
def run_cases(oracle):
    return _cases(oracle, B_MID, _run_blocks())


@pytest.mark.parametrize("waves,walkers", CONFIGS)
def test_lane_runs_around_16_32_48_and_the_rings_ends(codec, run_cases, waves, walkers):
    _run(codec, run_cases, B_MID, waves, walkers, "lane runs")


# ------------------------------------------------------------------ hard stops
def _stop_blocks(B, marks=False):
    """[(name, stream)], or with marks [(name, stream, compressed positions behind the stops)]"""
    out = []
    lead = NEAR2 + 180

    def keep(name, b, tail_ll=None):
        s = b.done(tail_ll)
        out.append((name, s, list(b.marks)) if marks else (name, s))
    for kind in STOPS:
        if kind != "far":
            b = Blk(B, 400 + len(out))
            if kind == "ml255":
                b.add(20, 1, 300)             # the first sequence can only repeat what its own literals gave it
                b.marks.append(b.cp)
            else:
                b.stop(kind)
            keep("first_in_block_" + kind, b)
        for k in (0, 1, 5, 63):
            # 64 small sequences fill a batch; the stop is lane k of the next one (k = 0: also two stops in a row when
            # the sequence in front is one)
            b = Blk(B, 500 + len(out)).until(lead).stop("overlap")
            for _ in range(64 + k if k != 63 else 63):
                b.plain(ll=4, ml=8)
            b.stop(kind)
            keep("lane_%d_%s" % (k, kind), b)
        b = Blk(B, 600 + len(out)).until(lead).stop(kind).stop(kind).plain(3).stop("ll255").stop(kind)
        keep("in_a_row_" + kind, b)
        # the stop is the last sequence with a match: behind it only the block's last literals
        b = Blk(B, 700 + len(out)).until(lead)
        while b.op < B - 700:
            b.plain()
        b.stop(kind)
        keep("before_last_" + kind, b, B - b.op)
    return out


@pytest.fixture(scope="module")
def stop_cases(oracle):
    return {B: _cases(oracle, B, _stop_blocks(B)) for B in (B_SMALL, B_BIG)}


@pytest.mark.parametrize("B", [B_SMALL, B_BIG])
@pytest.mark.parametrize("waves,walkers", CONFIGS)
def test_hard_stops_of_every_kind_at_every_place(codec, stop_cases, waves, walkers, B):
    _run(codec, stop_cases[B], B, waves, walkers, "hard stops")


@pytest.fixture(scope="module")
def mutated_cases(oracle):
    """streams changed behind a stop: the sequences the batches resume with are others than the ones written (or the stream
    is no longer valid at all); the verdict and the bytes are the oracle's"""
    rng = np.random.default_rng(77)
    named = []
    for name, s, marks in _stop_blocks(B_SMALL, marks=True):
        for j in range(2):
            m = s.copy()
            # one to three bytes changed among the 24 behind a stop: tokens, lengths and offsets of the sequences that follow
            p = int(rng.choice(marks)) + int(rng.integers(0, 24))
            for q in range(p, min(p + int(rng.integers(1, 4)), len(m))):
                m[q] = int(rng.choice([0, 0x0f, 0xf0, 0xff, int(rng.integers(0, 256))]))
            named.append(("%s_mut%d@%d" % (name, j, p), m))
    cases = _cases(oracle, B_SMALL, named, accept=False)
    return cases


@pytest.mark.parametrize("waves,walkers", CONFIGS)
def test_streams_mutated_behind_a_stop_keep_the_oracles_verdict(codec, mutated_cases, waves, walkers):
    _run(codec, mutated_cases, B_SMALL, waves, walkers, "mutated")


# ------------------------------------------------------------------ zstd: the same engine with longer matches
@pytest.fixture(scope="module")
def zstd_long_match_cases(oracle):
    """blocks of units `random bytes, the same bytes again`: level 1 writes each repeat as one match of several hundred bytes
    whose source is the literal run in front of it -- a dependent match of the batch above 256 bytes, over 5-11 boundaries"""
    B, out = B_BIG, []
    for i in range(24):
        rng = np.random.default_rng(900 + i)
        parts, total = [], 0
        while B - total >= 1400:
            a = rng.integers(0, 256, int(rng.integers(280, 700)), dtype=np.uint8)
            parts += [a, a]
            total += 2 * len(a)
        parts.append(rng.integers(0, 256, B - total, dtype=np.uint8))
        raw = np.concatenate(parts)
        assert len(raw) == B
        f = oracle.zstd_compress(raw, 1)
        assert len(f) < B * 0.6, "the repeats were not found"
        out.append(("unit_repeat_%d" % i, f, raw))
    return out


@pytest.mark.parametrize("path", [1, 2])
def test_zstd_dependent_matches_above_256_bytes(codec, zstd_long_match_cases, path):
    with _options(codec, {cc.OPT_ZSTD_DECODE_PATH: path}):
        _batch_check(codec, METHOD_ZSTD, zstd_long_match_cases, B_BIG, ("zstd long dependent matches", path))
