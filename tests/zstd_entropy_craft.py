"""Frames whose literals and sequences are dictated, for the entropy stage of the zstd encoders (tests/
test_zstd_entropy_craft_cpu.py, tests/test_gpu_zstd_entropy_craft.py).  Test infrastructure only; every input is fixed by SEED.

The second half of the encoder (Huffman and FSE table building, ZSTD_compressLiterals, ZSTD_encodeSequences) sees only what
the match finders hand it, and the suite's other inputs were built to drive the match finders.  Here the hand-over itself
is dictated.  A frame opens with 128 KiB of random bytes: the first zstd block, which comes out raw and leaves no tables.
Every block behind it is assembled from a list of (ll, ml) and a literal string: ll bytes from the string, then ml bytes
copied from a random place in the first block, and so on.  The copy's source is drawn so that the bytes around the copy
cannot lengthen it, so the block's literal section is the dictated string and its sequence list the dictated one wherever
the parser takes every copy (`greedy` and up with copies of 16 bytes; `fast` and `dfast` stride ever wider through the
random block and know little of it: they get long copies out of its first bytes, the "/near" variants, or the single-block
form).  Copies whose sources overlap would match each other, so the sources of a block are disjoint where they fit, and in
a chain of dictated blocks every block copies from a random block of its own.  What each case really reaches is not taken on trust: the CPU test reads it off the
oracle's branch counters and the frames' headers.

    dictated(rng, hist, seqs, lits, ...)   one block behind `hist`
    two_block / chain / single             the frame forms
    cases()                                the fixed list of Case(name, frame, raw_ok, skip)
    by_size(strategy, part)                {frame size: [Case]}: a compress call takes frames of one size
    PROPERTIES                             {name: (classes that must reach it, predicate(blocks, trace, case name))}
    levels(oracle, n), strategy_class(s)   one level per strategy for frames of n bytes, and a strategy's class

Branches of the entropy stage that a bounded search (tests/hunt_entropy.py: seed 20250921, 600 random literal distributions
and sequence lists through dictated(), every level of levels()) did not reach, and that therefore have no case and no test:
    huf_undescribable       a Huffman table over more than 128 symbols whose weights do not compress
    seq_last_ncount_raw     fewer than 4 bytes behind the last table description
    huf_hsz12_raw, huf_hsz12_treeless      hsz + 12 >= n
    tab_norm_fail           a failing normalisation in build_ctable
    sel_default_disallowed  an offset table with the default disallowed (needs offset code 29: out of reach of 128 KiB blocks)
"""
import collections
import functools

import numpy as np

SEED = 20250921
K = 131072                      # ZSTD_BLOCKSIZE_MAX: the raw first block, and every dictated block but a frame's last
PAD_SMALL, PAD_MID = 8192, 32768        # what a frame's last dictated block is padded to
NEAR = 1024                     # sources of the "/near" variants lie in the first block's first bytes
SINGLE_B, SINGLE_DICT = 16384, 2048     # the single-block form: a random dictionary, then the dictated part

Case = collections.namedtuple("Case", "name frame raw_ok skip")     # skip: the random blocks in front


# ---------------- the generator ----------------
def dictated(rng, hist, seqs, lits, total=None, pad="stretch", of_code=None, of_codes=None, src_lo=1, src_hi=K, tail=b""):
    """One block behind the bytes `hist`: for every (ll, ml) of seqs, ll bytes of `lits`, then ml bytes copied from hist[s:]
    with s in [src_lo, src_hi - ml); what is left of lits, then `tail`, ends the block.  The copies' sources are disjoint
    where they fit the range, and no source is taken whose byte in front equals the byte in front of the copy or whose byte
    behind equals the byte behind the copy (either would lengthen the match).  of_code: every offset + 3 lies in [2^of_code, 2^(of_code + 1)), one offset code
    (of_codes: {index of a sequence: its offset code}, for these in place of of_code and from anywhere in hist's first block).
    total: the block's size; pad = "stretch" lengthens the copies evenly to reach it (up to half the source range), pad = "tail" appends bytes of a
    128-symbol alphabet behind the last literal.  Returns the block."""
    seqs = [(int(a), int(b)) for a, b in seqs]
    lits = np.frombuffer(bytes(lits), np.uint8) if not isinstance(lits, np.ndarray) else lits.astype(np.uint8)
    tail = np.frombuffer(bytes(tail), np.uint8)
    used = sum(a + b for a, b in seqs)
    n_in_seq = sum(a for a, _ in seqs)
    assert n_in_seq <= len(lits)
    size = used + (len(lits) - n_in_seq) + len(tail)
    if total is not None:
        assert size <= total, (size, total)
        slack = total - size
        if pad == "stretch" and seqs:
            q, r = divmod(slack, len(seqs))
            longest = max((src_hi - src_lo) // 2, max(b for _, b in seqs))     # what does not fit the copies goes to the tail
            grown = [(a, min(b + q + (i < r), max(b, longest))) for i, (a, b) in enumerate(seqs)]
            slack -= sum(g[1] - s[1] for g, s in zip(grown, seqs))
            seqs = grown
        if slack:
            tail = np.concatenate([tail, rng.integers(0, 128, slack).astype(np.uint8)])
    base = len(hist)
    out = np.empty(sum(a + b for a, b in seqs) + (len(lits) - n_in_seq) + len(tail), np.uint8)
    rest = np.concatenate([lits[n_in_seq:], tail])
    cur, lp, cont = 0, 0, None                  # cont: the byte that would lengthen the previous copy
    slots = _slots(rng, [b for _, b in seqs], src_lo, src_hi - 1) if of_code is None else None
    of_codes = of_codes or {}

    def at(i):                                  # byte i of history + block so far
        return hist[i] if i < base else out[i - base]

    for k, (ll, ml) in enumerate(seqs):
        out[cur:cur + ll] = lits[lp:lp + ll]
        lp += ll
        cur += ll
        if ll:
            cont = None
        nxt = None                              # the byte behind this copy, where it is known now
        if k + 1 < len(seqs):
            if seqs[k + 1][0]:
                nxt = int(lits[lp])
        elif len(rest):
            nxt = int(rest[0])
        before = int(at(base + cur - 1)) if base + cur > 0 else None

        def fits(s):
            return not ((before is not None and s > 0 and int(hist[s - 1]) == before)
                        or (cont is not None and int(hist[s]) == cont) or (nxt is not None and int(hist[s + ml]) == nxt))

        s = None
        code = of_codes.get(k, of_code)
        if slots is not None and code is None:  # a free slot of this length whose surroundings fit
            free = slots[ml]
            for j in range(min(len(free), 64)):
                if fits(free[j]):
                    s = free.pop(j)
                    break
        if s is None:                           # a random place: it may overlap another copy's source
            lo, hi = (1, min(base, K) - ml) if k in of_codes else (src_lo, src_hi - ml)
            if code is not None:                # offset = base + cur - s
                lo = max(lo, base + cur - ((2 << code) - 1 - 3))
                hi = min(hi, base + cur - ((1 << code) - 3) + 1)
            assert lo < hi, (k, ll, ml, lo, hi)
            for _ in range(400):
                s = int(rng.integers(lo, hi))
                if fits(s):
                    break
            else:
                raise AssertionError("no source for copy %d" % k)
        out[cur:cur + ml] = hist[s:s + ml]
        cont = int(hist[s + ml])
        cur += ml
    out[cur:] = rest
    return out


def _slots(rng, mls, lo, hi):
    """{ml: [source positions]}: disjoint sources for copies of these lengths in [lo, hi), in random order with the room
    that is left spread at random between them; None where they do not fit.  Two copies with overlapping sources would
    match each other, and the parser would take that nearer match for a part of the later one."""
    spare = hi - lo - sum(mls)
    if spare < 0:
        return None
    gaps = np.sort(rng.integers(0, spare + 1, len(mls)))
    out, pos = {}, lo
    for g, k in zip(gaps, rng.permutation(len(mls))):
        out.setdefault(mls[k], []).append(pos + int(g))
        pos += mls[k]
    for v in out.values():
        rng.shuffle(v)
    return out


def first_block(rng):
    return rng.integers(0, 256, K).astype(np.uint8)


def two_block(seed, seqs, lits, total=PAD_SMALL, **kw):
    """128 KiB of random bytes, then one dictated block"""
    rng = np.random.default_rng(seed)
    h = first_block(rng)
    return np.concatenate([h, dictated(rng, h, seqs, lits, total=total, **kw)])


def _pad_for(n_bytes):
    return PAD_SMALL if n_bytes <= PAD_SMALL else (PAD_MID if n_bytes <= PAD_MID else K)


def chain(seed, blocks, total=None):
    """Several dictated blocks in a row, to carry tables from block to block: as many random blocks of 128 KiB as there
    are dictated ones, then the blocks: a dict of dictated()'s arguments, or 128 KiB given as bytes.  Dictated block i
    copies from random block i alone (two blocks copying from one would match each other's copies), and all but the last
    are exactly 128 KiB."""
    rng = np.random.default_rng(seed)
    n = sum(isinstance(b, dict) for b in blocks)
    h = np.concatenate([first_block(rng) for _ in range(n)])
    parts, i = [h], 0
    for j, b in enumerate(blocks):
        if not isinstance(b, dict):
            assert len(b) == K and j + 1 < len(blocks)
            parts.append(np.asarray(b, np.uint8))
            continue
        size = K
        if j + 1 == len(blocks):
            size = total or _pad_for(sum(x + y for x, y in b["seqs"]) + len(b["lits"]) - sum(x for x, _ in b["seqs"]))
        parts.append(dictated(rng, h, total=size, src_lo=i * K + 1, src_hi=(i + 1) * K, **b))
        i += 1
    return np.concatenate(parts)


def single(seed, seqs, lits, total=SINGLE_B, **kw):
    """one block: SINGLE_DICT random bytes, then the dictated part copying from them.  The literal section holds the dictionary
    too, and random bytes of a 128-symbol alphabet fill the block up; cheap at every level, for properties of the sequences."""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, SINGLE_DICT).astype(np.uint8)
    return np.concatenate([d, dictated(rng, d, seqs, lits, total=total - SINGLE_DICT, src_hi=SINGLE_DICT, pad="tail", **kw)])


# ---------------- literal strings ----------------
def by_counts(rng, counts, symbols=None):
    """a shuffled string with counts[i] times symbols[i] (symbols default 0, 1, ...)"""
    symbols = np.arange(len(counts)) if symbols is None else np.asarray(symbols)
    a = np.repeat(symbols.astype(np.uint8), counts)
    rng.shuffle(a)
    return a


def skewed(rng, n, nsym, top=None):
    """n literals over nsym symbols, geometric-like counts; the highest symbol value is `top` (default nsym - 1)"""
    nsym = max(2, min(nsym, n // 4))
    w = 0.8 ** np.arange(nsym)
    counts = np.maximum(1, np.floor(w / w.sum() * n)).astype(np.int64)
    counts[0] += n - counts.sum()
    assert counts[0] > 0
    symbols = np.arange(nsym)
    if top is not None:
        symbols[-1] = top
    return by_counts(rng, counts, symbols)


def fib_counts(k, extra=0, scale=1):
    """Fibonacci counts over k symbols (a Huffman tree of depth k - 1), `extra` more symbols of count 1, all times `scale`"""
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return [c * scale for c in f[:k][::-1] + [1] * extra]


def ones(n, ml=16):
    """n sequences of one literal and a copy of ml bytes"""
    return [(1, ml)] * n


def ends_long(seqs):
    """the last copy 8 bytes longer: no match finder starts a match in a block's last 8 bytes"""
    return seqs[:-1] + [(seqs[-1][0], seqs[-1][1] + 8)]


# ---------------- the case list ----------------
LIT_COUNTS = (64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5119, 5120, 5121, 16383, 16384, 16385)
SMALL_LIT_COUNTS = (31, 32, 63)                 # raw by size
STREAM_COUNTS = (63, 64, 65, 127, 128, 129, 1023, 1024, 1025)      # symbols of one stream
# literal counts that give such a stream: the only stream below 256 literals (63 or fewer stay raw), else the first three
# (ceil(n / 4) symbols each) or the last (the rest: 261 = 3 * 66 + 63)
STREAM_LITS = {63: 261, 64: 64, 65: 65, 127: 127, 128: 128, 129: 129, 1023: 4 * 1023 - 3, 1024: 4 * 1024 - 3, 1025: 4 * 1025 - 3}
STREAM_LITS_4 = {64: 256, 65: 257, 127: 4 * 127 - 3, 128: 4 * 128 - 3, 129: 4 * 129 - 3}       # the same in one of four streams
NSEQ = (1, 2, 3, 63, 64, 65, 127, 128, 129, 192, 193)


@functools.lru_cache(maxsize=None)
def cases():
    """the fixed list; frames are read-only"""
    out = []
    seed = [SEED]

    def add(name, frame, raw_ok=False, skip=1):
        frame.setflags(write=False)
        out.append(Case(name, frame, raw_ok, skip))

    def nxt():
        seed[0] += 1
        return seed[0]

    def lit_case(name, lits, ml=16, raw_ok=False, total=None):
        """twice: sources anywhere in the first block, and ("/near") in its first NEAR bytes, which `fast` and `dfast`,
        striding ever wider through the random block, still have in their tables"""
        n = len(lits)
        if n * (1 + ml) + 8 <= K:
            add(name, two_block(nxt(), ends_long(ones(n, ml)), lits, total=total or _pad_for(n * (1 + ml) + 8)), raw_ok)
        else:                                   # two literals between copies of 13 bytes or fewer (three in front of the first)
            m2 = min(13, (K - n - 8) // (n // 2))
            sq = [(2 + (n & 1), m2)] + [(2, m2)] * (n // 2 - 1)
            add(name, two_block(nxt(), ends_long(sq), lits, total=K), raw_ok)
        ml = ml if n * (1 + ml) + 8 <= K else 6
        ml = 64 if n * 65 + 8 <= K else ml
        add(name + "/near", two_block(nxt(), ends_long(ones(n, ml)), lits, total=total or _pad_for(n * (1 + ml) + 8), src_hi=NEAR),
            raw_ok)

    rng = np.random.default_rng(SEED)
    # -- literal counts: every size format of the header, 1 and 4 streams, the histogram's and the copy's rounds
    for n in SMALL_LIT_COUNTS + LIT_COUNTS:
        lit_case("lits/%d" % n, skewed(rng, n, 24))
    for n in LIT_COUNTS[8:]:                    # the same counts in runs of 256 literals between long copies: for the parsers below `lazy`
        sq = [(256 + n % 256, 64)] + [(256, 64)] * (n // 256 - 1)
        add("lits/%d/runs" % n, two_block(nxt(), ends_long(sq), rng.integers(0, 64, n).astype(np.uint8), total=K))
    for n in (4 * 300 + 1, 4 * 300 + 2, 4 * 300 + 3):                 # 4k + 1 .. 4k + 3: a shorter last stream
        lit_case("lits/4k+%d" % (n & 3), skewed(rng, n, 24))
    for m in STREAM_COUNTS:
        lit_case("stream/%d" % m, skewed(rng, STREAM_LITS[m], 24))
        if m in STREAM_LITS_4:
            lit_case("stream/%d/of-four" % m, skewed(rng, STREAM_LITS_4[m], 24))
    for i in range(3):                                                 # the header's last size format: more draws of it
        for n in (16383, 16384, 16385):
            lit_case("lits/%d/%d" % (n, i), skewed(rng, n, 24))
    # -- histograms
    lit_case("rle/1024", np.full(1024, 0x41, np.uint8))
    lit_case("rle/200", np.full(200, 0x00, np.uint8))
    lit_case("rle/5000", np.full(5000, 0xFF, np.uint8))
    lit_case("all-but-one/1024", by_counts(rng, [1023, 1], [0x41, 0x42]))
    lit_case("all-but-one/4097", by_counts(rng, [4096, 1], [0x07, 0xF0]))
    lit_case("two-symbols/1024", by_counts(rng, [700, 324], [0x30, 0x31]))
    lit_case("two-symbols/200", by_counts(rng, [100, 100], [0x00, 0xFF]))
    lit_case("flat/2048", by_counts(rng, [8] * 256))                   # largest 8 <= (2048 >> 7) + 4 = 20
    lit_case("flat-edge/2048", by_counts(rng, [20] + [8] * 253 + [4]))  # largest = 20: still raw
    lit_case("flat-over/2048", by_counts(rng, [21] + [8] * 253 + [3]))  # largest = 21: Huffman is tried (and gains too little)
    # Fibonacci-like counts: the depth clip, by one level and by more.  Every clip leaves a debt (`total > 0`) and runs the
    # repay loop, so that loop has no counter of its own; the loop for a repayment that overshoots (`total < 0`) has one
    lit_case("fib/13x8", by_counts(rng, fib_counts(13, scale=8)))      # 4872 literals, table log 11, depth 12
    lit_case("fib/14", by_counts(rng, fib_counts(14)))                 # 986 literals, table log 8, depth 13
    lit_case("fib/14+16", by_counts(rng, fib_counts(14, extra=16)))    # 30 symbols
    lit_case("fib/16+8", by_counts(rng, fib_counts(16, extra=8)))      # 24 symbols, 2591 literals
    lit_case("fib/17+23", by_counts(rng, fib_counts(17, extra=23)))    # 40 symbols, 4203 literals
    lit_case("fib/20+8", by_counts(rng, fib_counts(20, extra=8)))      # 28 symbols, 17718 literals
    lit_case("fib/12+20x3", by_counts(rng, fib_counts(12, extra=20, scale=3)))
    # alphabets by their top symbol: direct against FSE-compressed weights, and the limit of 128
    for top in (127, 128, 129, 255):
        lit_case("top/%d/few" % top, skewed(rng, 1500, 12, top))       # 12 symbols used, weights mostly 0: compress well
        lit_case("top/%d/dense" % top, by_counts(rng, rng.integers(1, 40, top + 1)))   # every symbol up to top, ragged weights
    lit_case("top/20/direct", skewed(rng, 300, 21))
    # a gain just short of minGain, and just enough: 1024 literals over 128 symbols, nearly flat
    for bump in (100, 150, 200, 250, 300, 350, 400):
        q, r = divmod(1024 - bump, 127)
        lit_case("mingain/%d" % bump, by_counts(rng, [bump] + [q + (i < r) for i in range(127)]), raw_ok=True)

    # -- Huffman tables across blocks
    def blk(n, lits, **kw):
        return dict(seqs=ends_long(ones(n)), lits=lits, **kw)

    a1024 = skewed(rng, 1024, 24)
    a5000 = skewed(rng, 5000, 24)
    for name, l1, l2 in (("same/1024-1024", a1024, rng.permutation(a1024)),        # preferRepeat below lazy; by cost above
                         ("same/5000-5000", a5000, rng.permutation(a5000)),        # by cost at every strategy
                         ("same/5000-1025", a5000, rng.permutation(a5000)[:1025]),
                         ("same/5000-200", a5000, rng.permutation(a5000)[:200]),   # one stream, treeless
                         ("same/5000-100", a5000, rng.permutation(a5000)[:100]),
                         ("same/5000-255", a5000, rng.permutation(a5000)[:255]),
                         ("same/1024-200", a1024, rng.permutation(a1024)[:200]),
                         ("other/5000-5000", a5000, (23 - rng.permutation(a5000)).astype(np.uint8)),   # a new table is cheaper
                         ("other/1024-1024", a1024, (23 - rng.permutation(a1024)).astype(np.uint8)),
                         ("lacks/1024-1024", a1024, np.concatenate([rng.permutation(a1024)[:1023], [200]])),
                         ("lacks/5000-5000", a5000, np.concatenate([rng.permutation(a5000)[:4999], [24]]))):
        add("huf2/" + name, skip=2, frame=chain(nxt(), [blk(len(l1), l1), blk(len(l2), l2)]))
    # a raw block, an RLE block, raw literals, RLE literals between two blocks of one distribution
    add("huf3/raw-block", skip=2, frame=chain(nxt(), [blk(1024, a1024), first_block(rng), blk(1024, rng.permutation(a1024))]))
    add("huf3/rle-block", skip=2, frame=chain(nxt(), [blk(1024, a1024), np.full(K, 0x55, np.uint8), blk(1024, rng.permutation(a1024))]))
    for name, mid in (("raw-lits", by_counts(rng, [4] * 256)), ("rle-lits", np.full(1024, 3, np.uint8))):
        add("huf3/" + name, skip=3, frame=chain(nxt(), [blk(1024, a1024), blk(len(mid), mid), blk(1024, rng.permutation(a1024))]))

    # -- sequences
    few = skewed(rng, 400, 24)
    some = rng.integers(0, 64, 260).astype(np.uint8)
    add("nseq/0", two_block(nxt(), [], rng.integers(0, 64, PAD_SMALL).astype(np.uint8)))
    add("nseq/0/short", two_block(nxt(), [], rng.integers(0, 64, 400).astype(np.uint8), total=None))   # minMatch 3 finds nothing either
    # the first block alone: a raw block, and at the levels of minMatch 3 one whose few sequences behind 128 KiB of raw literals
    # outgrow the block, so that the sequence stream's writes stop at src_size + 32
    add("cap/random", first_block(np.random.default_rng(nxt())), raw_ok=True, skip=0)
    for n in NSEQ:
        add("nseq/%d" % n, two_block(nxt(), ones(n), some[:n + 64]))
        add("nseq/%d/near" % n, two_block(nxt(), ones(n, 40), some[:n + 64], src_hi=NEAR))
        add("nseq/%d/single" % n, single(nxt(), [(0, 64)] * n, b""), skip=0)
    # around 0x7F00: 32 760 copies of 4 bytes, nothing between them (a raw block below lazy: the writes beyond the cap)
    add("nseq/0x7F00", two_block(nxt(), [(0, 4)] * 32760, b"", total=K), raw_ok=True)
    add("nseq/0x7F00/5", two_block(nxt(), [(0, 5)] * 26000, b"", total=K), raw_ok=True)
    # all codes of a table equal, at 2 and 3 sequences (predefined against RLE) and more
    for n in (2, 3, 64, 300):
        add("rle-tables/%d" % n, two_block(nxt(), [(1, 16)] * n, few, pad="tail", of_code=16))
    # code histograms on both sides of dyn_min (LL, ML: 64 * (10 - strategy) / 8 = 72, 64, 56; OF: 36, 32, 28) and of `most`
    for n in (27, 28, 29, 31, 32, 33, 35, 36, 37, 55, 56, 57, 71, 72, 73):
        sq = [(int(rng.integers(0, 12)), int(rng.integers(64, 90))) for _ in range(n)]
        add("dyn-min/%d" % n, single(nxt(), sq, rng.integers(0, 64, 12 * n).astype(np.uint8)), skip=0)
    for n, share in ((400, 2), (400, 40), (400, 12), (400, 13), (400, 14)):     # most >= nseq >> 5 (LL, ML), >> 4 (OF)
        nb = n // share
        sq = [(3, 70)] * nb + [(int(rng.integers(0, 16)), int(rng.integers(64, 96))) for _ in range(n - nb)]
        sq = [sq[i] for i in rng.permutation(n)]
        add("most/%d/%d" % (n, share), two_block(nxt(), sq, rng.integers(0, 64, 16 * n).astype(np.uint8), total=K, pad="tail"))
    # every match length code of 35 as often as every other: the largest count is below nseq >> 5
    flat_ml = [6 + i for i in range(29)] + [35, 37, 39, 41, 43, 47]
    for k in (5, 10, 40, 100):               # 5, 10: a table of 128 cells for 35 codes; rounding each up overshoots it
        sq = [(1, m) for m in flat_ml] * k
        sq = [sq[i] for i in rng.permutation(len(sq))]
        add("most/flat-ml/%d" % k, two_block(nxt(), sq, rng.integers(0, 64, len(sq)).astype(np.uint8), total=K, pad="tail"))
    # one code in front and many rare ones: the first normalisation overshoots, the secondary one takes over
    for i, (dom, rare, each) in enumerate(((500, 30, 1), (900, 30, 2), (2000, 33, 3), (4000, 33, 2), (300, 25, 1), (1500, 30, 1))):
        sq = [(1, 10)] * dom + [(1, 12 + j) for j in range(rare)] * each
        sq = [sq[i2] for i2 in rng.permutation(len(sq))]
        add("norm-m2/%d" % i, two_block(nxt(), ends_long(sq), rng.integers(0, 64, len(sq)).astype(np.uint8), total=K, pad="tail"))

    # two consecutive blocks of the same (ll, ml) statistics: repeat is cheapest
    def random_seqs(r, n, ll_hi, ml_lo, ml_hi):
        return [(int(a), int(b)) for a, b in zip(r.integers(0, ll_hi, n), r.integers(ml_lo, ml_hi, n))]

    for n, llh, mlo, mlh in ((5000, 4, 8, 24), (3000, 8, 16, 40), (1500, 16, 32, 80), (2500, 2, 30, 50)):
        r = np.random.default_rng(nxt())
        s1, s2 = random_seqs(r, n, llh, mlo, mlh), random_seqs(r, n, llh, mlo, mlh)
        l1, l2 = skewed(r, sum(a for a, _ in s1), 24), skewed(r, sum(a for a, _ in s2), 24)
        add("repeat/%d" % n, skip=2, frame=chain(nxt(), [dict(seqs=ends_long(s1), lits=l1), dict(seqs=ends_long(s2), lits=l2)], total=K))
    # n1 >= 2048 against below it (the low-probability symbols)
    for n in (2046, 2047, 2048, 2049, 2050):
        r = np.random.default_rng(nxt())
        sq = random_seqs(r, n, 40, 8, 60)
        add("lowprob/%d" % n, two_block(nxt(), sq, skewed(r, sum(a for a, _ in sq), 24), total=K))
    # a long literal length and a long match length, as the first, a middle and the last sequence
    bg = [(2, 20)] * 40
    for where in (0, 20, 39):
        sq = list(bg)
        sq[where] = (65536 + where, 20)
        for alphabet in (128, 256):             # few enough chance matches inside the run; 256: raw literals
            add("long-ll/%d/%d" % (where, alphabet),
                two_block(nxt(), ends_long(sq), rng.integers(0, alphabet, 65536 + where + 78).astype(np.uint8), total=K), raw_ok=True)
        sq = list(bg)
        sq[where] = (2, 65539 + where)
        add("long-ml/%d" % where, two_block(nxt(), sq, few, total=K, pad="tail"))
    # 64 fat sequences: hundreds of literals, matches of thousands of bytes, offsets above 64 KiB
    r = np.random.default_rng(nxt())
    sq = [(int(a), int(b)) for a, b in zip(r.integers(300, 600, 64), r.integers(1000, 1500, 64))]
    add("fat/64", two_block(nxt(), ends_long(sq), r.integers(0, 128, sum(a for a, _ in sq)).astype(np.uint8), total=K, src_hi=50000))
    sq = [(int(a), int(b)) for a, b in zip(r.integers(16, 64, 128), r.integers(600, 900, 128))]
    add("fat/128", two_block(nxt(), ends_long(sq), r.integers(0, 128, sum(a for a, _ in sq)).astype(np.uint8), total=K, src_hi=50000))
    # One sequence of more than 64 bits in the stream: 9 bits of literal length, 16 of a long match length, 17 of an offset of
    # 128 KiB or more, and 9 + 9 + 8 bits of the three states, because its three codes are rare among 2048 and more short
    # sequences (tables of log 9, 9, 8), whose copies come from the first block's upper half and so from nearer than 128 KiB.
    # One to four short sequences follow it (the block's last sequence gives up no state bits): their number and lengths move
    # its first bit within a 32-bit word, and where that lies beyond bit 96 - width, the bits spread over four words.  Of 48
    # variants v these eight got there at some level, 33 at a level of every class.
    for v in (1, 6, 10, 11, 33, 37, 41, 46):
        r = np.random.default_rng(9000 + v)
        n = 2048 + v
        sq = [(1, 24 + v % 3)] * n + [(520 + 11 * v, 65539)] + [(1 + v % 5, 35 + (v * 3) % 11)] * (1 + v % 4)
        add("wide/%d" % v, two_block(7000 + v, ends_long(sq), r.integers(0, 256, sum(a for a, _ in sq)).astype(np.uint8), total=K,
                                     src_lo=K // 2 + 8, of_codes={n: 17}))
    # the two-byte side of 0x7F00, from near: what the parsers leave of so many copies of 4 bytes differs by a few hundred
    for n in (32500, 32600, 32680):
        add("nseq/0x7F00/below/%d" % n, two_block(nxt(), [(0, 4)] * n, b"", total=K), raw_ok=True)
    # zero runs of 3 or more and of 24 or more in a written table description: literal lengths 0 and 30 000, matches of 3 + {0, 40 000}
    sq = ([(0, 8)] * 150 + [(300, 2100)] * 6 + [(0, 2100)] * 6)
    sq = [sq[i] for i in rng.permutation(len(sq))]
    add("zero-runs", two_block(nxt(), sq, skewed(rng, 1800, 24), total=K, pad="tail"))
    return tuple(out)


# The optimal parsers take about a second of CPU time (oracle and libzstd) per ten of these frames, so at btopt, btultra and
# btultra2 the GPU test runs this part of the list: a cover, cheapest frames first, of every property reached at those
# levels.  tests/test_zstd_entropy_craft_cpu.py checks that it loses none of them.  On the device these parsers take about
# half a second per 128 KiB block of a frame, random ones included, and the frames of a call run side by side, so a call
# costs what its longest frame costs: the chains of several dictated blocks (five size groups of 3 to 5 blocks) go through
# one of the three strategies only, btultra.
OPT_CASES = frozenset((
    'lits/31/near', 'lits/32', 'lits/63', 'lits/255', 'lits/1023', 'lits/4095', 'lits/4096', 'lits/4096/near',
    'lits/5119', 'lits/5120', 'lits/16383', 'lits/16384', 'lits/16385', 'lits/4095/runs', 'lits/4096/runs',
    'lits/4097/runs', 'lits/5120/runs', 'lits/5121/runs', 'lits/16385/runs', 'stream/63', 'stream/64/near',
    'stream/64/of-four', 'stream/65', 'stream/65/of-four', 'stream/127', 'stream/128', 'stream/129',
    'stream/129/of-four', 'rle/200', 'two-symbols/200', 'mingain/150', 'mingain/250', 'mingain/300',
    'huf2/same/5000-200', 'huf2/same/5000-255', 'huf2/same/1024-200', 'huf2/other/1024-1024', 'huf2/lacks/1024-1024',
    'huf3/raw-block', 'huf3/rle-block', 'huf3/raw-lits', 'huf3/rle-lits', 'nseq/0/short', 'cap/random', 'nseq/1',
    'nseq/1/single', 'nseq/2', 'nseq/2/single', 'nseq/3', 'nseq/63/single', 'nseq/127/single', 'nseq/128/single',
    'nseq/129/single', 'nseq/192/near', 'nseq/192/single', 'nseq/193/near', 'nseq/193/single', 'nseq/0x7F00',
    'dyn-min/35', 'dyn-min/55', 'most/flat-ml/40', 'norm-m2/1', 'norm-m2/2', 'repeat/1500', 'long-ml/0',
    'long-ll/20/256', 'long-ml/20', 'long-ml/39', 'fat/64', 'fat/128', 'wide/37', 'nseq/0x7F00/below/32500'))
OPT_STRATEGY = 7                # btopt: from here up the shorter list


def by_size(strategy=1, part="all"):
    """{frame size: [Case]} of the list a strategy gets.  part: "all", "single" (one dictated block: frames of at most
    256 KiB) or "chains" (several)"""
    groups = {}
    for c in cases():
        if (strategy < OPT_STRATEGY or c.name in OPT_CASES) and (part == "all" or (part == "chains") == (c.frame.nbytes > 2 * K)):
            groups.setdefault(c.frame.nbytes, []).append(c)
    return groups


# ---------------- what a case reaches ----------------
def strategy_class(strategy):
    """the entropy stage's three classes: preferRepeat and threshold selection below `lazy`; selection by cost and repeat
    tables from `lazy` to `btopt`; the other ZSTD_minGain at `btultra` and `btultra2`"""
    return "low" if strategy < 4 else ("mid" if strategy < 8 else "high")


def levels(oracle, n):
    """{level: strategy}: -5, and the lowest level of every strategy for a frame of n bytes (the oracle's parameter table)"""
    out, seen = {-5: oracle.zstd_enc_strategy(-5, n)}, set()
    for lv in range(1, 23):
        s = oracle.zstd_enc_strategy(lv, n)
        if s not in seen:
            seen.add(s)
            out[lv] = s
    return out


ALL, LOW, COST = ("low", "mid", "high"), ("low",), ("mid", "high")


def _lit(blocks, pred):
    return any(b["type"] == "compressed" and pred(b) for b in blocks)


def _regen(*ns):
    return lambda blocks, t, name: _lit(blocks, lambda b: b["regen"] in ns and (b["regen"] <= 63 or b["lit"] != "raw"))


def _streams(m):
    """a Huffman stream of m symbols: the only one, one of the first three of four, or the fourth"""
    return lambda blocks, t, name: _lit(blocks, lambda b: (b["streams"] == 1 and b["regen"] == m) or (
        b["streams"] == 4 and m in ((b["regen"] + 3) // 4, b["regen"] - 3 * ((b["regen"] + 3) // 4))))


def _nseq(*ns):
    return lambda blocks, t, name: _lit(blocks, lambda b: b["nseq"] in ns)


def _mode(i, m):
    return lambda blocks, t, name: _lit(blocks, lambda b: b["modes"] is not None and b["modes"][i] == m)


def _hit(*names):
    return lambda blocks, t, name: all(t[n] > 0 for n in names) and any(b["type"] == "compressed" for b in blocks)


def _hit_any_block(*names):
    return lambda blocks, t, name: all(t[n] > 0 for n in names)


PROPERTIES = collections.OrderedDict()
for _n in SMALL_LIT_COUNTS + LIT_COUNTS:
    PROPERTIES["literals: %d" % _n] = (ALL, _regen(_n))
for _n in (1, 2, 3):
    PROPERTIES["literals: 4k+%d" % _n] = (ALL, lambda blocks, t, name, d=_n: _lit(blocks, lambda b: b["streams"] == 4 and b["regen"] & 3 == d))
for _m in STREAM_COUNTS:
    PROPERTIES["stream of %d symbols" % _m] = (ALL, _streams(_m))
PROPERTIES.update({
    "literals: one stream": (ALL, lambda blocks, t, name: _lit(blocks, lambda b: b["streams"] == 1)),
    "literals: RLE": (ALL, lambda blocks, t, name: _lit(blocks, lambda b: b["lit"] == "rle") and t["lit_rle"] > 0),
    "literals: flat histogram, raw": (ALL, _hit("lit_flat_raw")),
    "literals: gain short of minGain, raw": (ALL, _hit_any_block("lit_mingain_raw")),
    "literals: disabled (negative level)": (("negative",), _hit_any_block("lit_disabled")),
    "huffman: depth clip": (ALL, _hit("huf_clip", "lit_compressed")),
    "huffman: depth clip by two levels or more": (ALL, _hit("huf_clip_by_2_or_more", "lit_compressed")),
    "huffman: depth clip overshoots": (ALL, _hit("huf_clip_overshoot", "lit_compressed")),
    "huffman: direct weights": (ALL, lambda blocks, t, name: _lit(blocks, lambda b: b["tree"] is not None and b["tree"] >= 128)),
    "huffman: FSE-compressed weights": (ALL, lambda blocks, t, name: _lit(blocks, lambda b: b["tree"] is not None and b["tree"] < 128)),
    "huffman: top symbol above 128, described": (ALL, _hit("huf_weights_fse_above_128", "lit_compressed")),
    "huffman: treeless by preferRepeat": (LOW, lambda blocks, t, name: t["huf_prefer_repeat"] > 0 and _lit(blocks, lambda b: b["lit"] == "treeless")),
    "huffman: treeless by cost": (ALL, lambda blocks, t, name: t["huf_treeless_by_cost"] > 0 and _lit(blocks, lambda b: b["lit"] == "treeless")),
    "huffman: treeless, one stream": (ALL, lambda blocks, t, name: _lit(blocks, lambda b: b["lit"] == "treeless" and b["streams"] == 1)),
    "huffman: new table over a usable old one": (ALL, _hit("huf_new_table_over_old")),
    "huffman: old table lacks a symbol": (ALL, _hit("huf_validate_fail")),
    "sequences: count in two bytes": (ALL, lambda blocks, t, name: _lit(blocks, lambda b: b["nseq_bytes"] == 2)),
    "sequences: count just below 0x7F00, two bytes": (COST, lambda blocks, t, name: _lit(blocks, lambda b: 0x7F00 - 256 <= b["nseq"] < 0x7F00)),
    "sequences: more than 64 bits for one": (ALL, _hit("seq_bits_over_64")),
    "sequences: one spread over three words": (ALL, _hit("seq_bits_3_dwords")),
    "sequences: one spread over four words": (ALL, _hit("seq_bits_4_dwords")),
    "sequences: count in three bytes": (COST, lambda blocks, t, name: _lit(blocks, lambda b: b["nseq_bytes"] == 3)),
    # only where minMatch is 3: a sequence of a longer match costs less than it saves, so the stream cannot outgrow its block
    "sequences: stream beyond the cap, raw block": (("high",), _hit_any_block("seq_over_cap", "block_mingain_raw")),
    "tables: one code, predefined (2 sequences)": (ALL, _hit("sel_one_code_basic")),
    "tables: one code, RLE": (ALL, _hit("sel_one_code_rle")),
    "tables: below dyn_min": (LOW, _hit("sel_below_dyn_min")),
    "tables: below most": (LOW, _hit("sel_below_most")),
    "tables: over both thresholds": (LOW, _hit("sel_threshold_compressed")),
    "tables: predefined by cost": (COST, _hit("sel_cost_basic")),
    "tables: compressed by cost": (COST, _hit("sel_cost_compressed")),
    "tables: repeat LL": (COST, _mode(0, "repeat")),
    "tables: repeat OF": (COST, _mode(1, "repeat")),
    "tables: repeat ML": (COST, _mode(2, "repeat")),
    "tables: low-probability symbols (n1 >= 2048)": (ALL, _hit("tab_low_prob")),
    "tables: n1 < 2048": (ALL, _hit("tab_no_low_prob")),
    "tables: secondary normalisation": (ALL, _hit("tab_norm_m2")),
    "tables: zero run of 3 or more": (ALL, _hit("tab_zero_run_3")),
    "tables: zero run of 24 or more": (ALL, _hit("tab_zero_run_24")),
    "sequences: long literal length": (("low", "mid"), _hit("seq_long_ll")),
    "sequences: long match length": (ALL, _hit("seq_long_ml")),
})


def _named(prefix, pred):
    """of the cases of one family: what only the dictated input tells (two symbols, where the long length stands)"""
    return lambda blocks, t, name: name.startswith(prefix) and pred(blocks, t)


def _pure(prefix):
    """of the cases <prefix><n>[/near]: Huffman literals of exactly the dictated count n"""
    return lambda blocks, t, name: name.startswith(prefix) and _lit(blocks, lambda b: b["lit"] in ("compressed", "treeless")
                                                                    and b["regen"] == int(name[len(prefix):].split("/")[0]))


def _between(prefix, middle, strict):
    """huf3/...: [first, the block or literals between, last]; strict: the last block's literals are treeless"""
    return _named(prefix, lambda blocks, t: middle(blocks[1]) and blocks[2].get("lit") in (("treeless",) if strict else ("treeless", "compressed")))


PROPERTIES.update({
    # btultra and btultra2 leave 8 to 140 bytes more as literals in these blocks: no pure section there
    "literals: all but one equal": (("low", "mid"), _pure("all-but-one/")),
    "literals: two symbols": (ALL, _pure("two-symbols/")),
    "sequences: a full batch of fat ones": (ALL, _named("fat/", lambda blocks, t: _lit(blocks, lambda b: b["nseq"] >= 64))),
})
for _what, _prefix, _mid in (("a raw block", "huf3/raw-block", lambda b: b["type"] == "raw"),
                             ("an RLE block", "huf3/rle-block", lambda b: b["type"] == "rle"),
                             ("raw literals", "huf3/raw-lits", lambda b: b.get("lit") == "raw"),
                             ("RLE literals", "huf3/rle-lits", lambda b: b.get("lit") == "rle")):
    PROPERTIES["huffman: %s between two blocks of one distribution" % _what] = (ALL, _between(_prefix, _mid, False))
    # at btultra and btultra2 the gain that decides for the old table is another: what they reach here is not asked of them
    PROPERTIES["huffman: table kept across %s" % _what] = (("low", "mid"), _between(_prefix, _mid, True))
for _w, _at in (("first", 0), ("a middle", 20), ("the last", 39)):
    # not at minMatch 3: 65 536 bytes that hold no match of 3 bytes are not to be had behind 128 KiB of history
    PROPERTIES["sequences: long literal length in %s sequence" % _w] = (("low", "mid"), _named("long-ll/%d/" % _at, lambda blocks, t: t["seq_long_ll"] > 0
                                                                               and blocks[0]["type"] == "compressed"))
    PROPERTIES["sequences: long match length in %s sequence" % _w] = (ALL, _named("long-ml/%d" % _at, lambda blocks, t: t["seq_long_ml"] > 0
                                                                             and blocks[0]["type"] == "compressed"))
for _n in (0,) + NSEQ:
    PROPERTIES["sequences: %d" % _n] = (ALL, _nseq(_n))
