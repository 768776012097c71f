"""Bounded search on the CPU for the entropy-stage branches that no case of tests/zstd_entropy_craft.py reaches (not collected
by pytest: `python tests/hunt_entropy.py [candidates] [seed]`, defaults 600 and 20250921, a few minutes).

Random literal distributions and sequence lists go through zstd_entropy_craft.dictated() into frames of 128 KiB of random
bytes and one dictated block; every frame is compressed by the oracle at every level of zstd_entropy_craft.levels() and the
oracle's branch counters (oracle/cryo_oracle.h), counted over the dictated block, are asked for the branches in TARGETS.
The families aim at them:
    weights     130 to 160 symbols, about as many of every Huffman weight: a table description that does not compress
    tiny        64 to 90 literals over wide alphabets: hsz + 12 >= n
    few         2 to 12 sequences of nearly equal codes: fewer than 4 bytes behind the last table description
    tables      20 to 3000 sequences with flat, peaked and two-level code histograms: a failing normalisation
    anything    random lists and distributions
What it finds belongs into zstd_entropy_craft.cases(); what it does not find is named in that module's docstring with the
candidate count.  Exit status 0 either way: it is a search, not a test."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle_lib
import zstd_entropy_craft as ze

TARGETS = ("huf_undescribable", "seq_last_ncount_raw", "huf_hsz12_raw", "huf_hsz12_treeless", "tab_norm_fail",
           "sel_default_disallowed")
FAMILIES = ("weights", "tiny", "few", "tables", "anything")


def candidate(rng, family):
    """(description, seqs, lits, keyword arguments of two_block)"""
    if family == "weights":
        top = int(rng.integers(129, 161))
        per = int(rng.integers(8, 13))
        classes = int(rng.integers(9, 12))
        symbols = rng.permutation(top)[:per * classes - 1].tolist() + [top]
        counts = [1 << (k % classes) for k in range(len(symbols))]
        lits = ze.by_counts(rng, counts, np.array(symbols))
        ll = int(rng.integers(4, 12))
        n = len(lits) // ll
        return "top %d, %d x %d weights" % (top, per, classes), [(ll, 8)] * n, lits, dict(total=ze.K)
    if family == "tiny":
        n = int(rng.integers(64, 91))
        top = int(rng.choice([40, 64, 100, 127, 128, 129, 200, 255]))
        big = int(rng.integers(5, 30))
        rest = rng.permutation(top)[:n - big] if top >= n - big else rng.integers(0, top, n - big)
        lits = rng.permutation(np.concatenate([np.full(big, top), rest]).astype(np.uint8))
        return "%d literals up to %d, one of them %d times" % (n, top, big), ze.ends_long(ze.ones(n)), lits, dict(total=ze.PAD_SMALL)
    if family == "few":
        n = int(rng.integers(2, 13))
        ll, ml = int(rng.integers(0, 4)), int(rng.integers(4, 40))
        seqs = [(ll + int(rng.integers(0, 2)), ml + int(rng.integers(0, 2))) for _ in range(n)]
        lits = rng.integers(0, 64, sum(a for a, _ in seqs) + int(rng.integers(0, 80))).astype(np.uint8)
        return "%d sequences near (%d, %d)" % (n, ll, ml), seqs, lits, dict(total=None, of_code=int(rng.integers(14, 18)))
    if family == "tables":
        n = int(rng.choice([20, 33, 64, 100, 257, 350, 600, 1100, 2047, 2048, 3000]))
        kind = int(rng.integers(0, 3))
        codes = int(rng.integers(2, 36))
        if kind == 0:       # flat
            mls = 6 + rng.integers(0, codes, n)
        elif kind == 1:     # one code in front
            mls = np.where(rng.random(n) < rng.uniform(0.5, 0.98), 10, 11 + rng.integers(0, codes, n))
        else:               # two levels
            mls = np.where(rng.random(n) < 0.5, 6 + rng.integers(0, 3, n), 12 + rng.integers(0, codes, n))
        lls = rng.integers(0, int(rng.choice([2, 4, 17, 40])), n)
        seqs = ze.ends_long([(int(a), int(b)) for a, b in zip(lls, mls)])
        lits = rng.integers(0, 64, int(lls.sum())).astype(np.uint8)
        return "%d sequences, kind %d, %d codes" % (n, kind, codes), seqs, lits, dict(total=ze.K, pad="tail")
    n = int(rng.integers(1, 4000))
    seqs = ze.ends_long([(int(a), int(b)) for a, b in zip(rng.integers(0, int(rng.choice([2, 8, 64])), n), rng.integers(4, 30, n))])
    nsym = int(rng.integers(2, 256))
    w = rng.random(nsym) ** int(rng.integers(1, 12))
    lits = rng.choice(nsym, size=sum(a for a, _ in seqs) + 1, p=w / w.sum()).astype(np.uint8)
    return "%d sequences, %d symbols" % (n, nsym), seqs, lits, dict(total=ze.K, pad="tail")


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 600
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else ze.SEED
    oracle = oracle_lib.Oracle()
    rng = np.random.default_rng(seed)
    found = {t: [] for t in TARGETS}
    seen = dict.fromkeys(oracle.zstd_enc_trace_names, 0)
    for i in range(count):
        family = FAMILIES[i % len(FAMILIES)]
        what, seqs, lits, kw = candidate(rng, family)
        while sum(a + b for a, b in seqs) + 8 > ze.K - 4096:      # too much for a block: fewer sequences
            seqs = ze.ends_long(seqs[:len(seqs) * 3 // 4])
        lits = lits[:max(sum(a for a, _ in seqs), min(len(lits), 2048))]
        frame = ze.two_block(seed + 1 + i, seqs, lits, **kw)
        for level in ze.levels(oracle, frame.nbytes):
            _, trace = oracle.zstd_compress_traced(frame, level, from_block=1)
            for k, v in trace.items():
                seen[k] += v
            for t in TARGETS:
                if trace[t]:
                    found[t].append((i, family, what, level))
    for t in TARGETS:
        print("%-24s %s" % (t, "%d hits, first: candidate %d (%s: %s) at level %d" % ((len(found[t]),) + found[t][0])
                            if found[t] else "not reached"))
    print("%d candidates, seed %d; counters never hit: %s" % (count, seed, sorted(k for k, v in seen.items() if v == 0)))


if __name__ == "__main__":
    main()
