"""CPU proof that the dictated frames of tests/zstd_entropy_craft.py reach the branches they are there for.

tests/test_gpu_zstd_entropy_craft.py holds the device encoders to the oracle, byte for byte, on these frames.  That says
something about the encoder's entropy stage only where the frames drive it: so every property named in
zstd_entropy_craft.PROPERTIES -- a literal count at an edge of the header's size formats or of the wave's rounds, a Huffman
stream of 63, 64, 65 ... symbols, RLE and treeless literals, the depth clip, each table mode, each selection rule, the long
lengths, the three-byte sequence count ... -- must be reached by at least one case at a level of every strategy class the
property names (below `lazy`; `lazy` to `btopt`; `btultra` and `btultra2`), in a block that goes out compressed unless raw is
the property.  What is reached is read off the oracle's branch counters (oracle/cryo_oracle.h), counted over the dictated
blocks alone, and off the frames' headers (zstd_craft.walk_entropy): neither decodes a bit of entropy-coded data.  A
property with no case fails the test; run with -s for the table of properties, cases and levels.

And the oracle is pinned on these very inputs: its frame is libzstd 1.4.8's on every case and level where the library
loads, and its decoder returns the input.  The counters change no byte: tests/test_oracle_golden.py and the other craft
tests run against the same library.

The branches no case reaches are named in zstd_entropy_craft's docstring with the search that looked for them
(tests/hunt_entropy.py); test_unreached_branches_are_the_named_ones keeps that list honest."""
import numpy as np
import pytest

import oracle_lib
import zstd_craft
import zstd_entropy_craft as ze

UNREACHED = {"huf_undescribable", "seq_last_ncount_raw", "huf_hsz12_raw", "huf_hsz12_treeless", "tab_norm_fail",
             "sel_default_disallowed"}


@pytest.fixture(scope="module")
def runs(oracle):
    """[(case, level, class, frame, dictated blocks' header fields, counters over the dictated blocks)], computed once"""
    out = []
    for c in ze.cases():
        for level, strategy in ze.levels(oracle, c.frame.nbytes).items():
            f, trace = oracle.zstd_compress_traced(c.frame, level, from_block=c.skip)
            f.setflags(write=False)
            blocks = zstd_craft.walk_entropy(f)["blocks"][c.skip:]
            out.append((c, level, "negative" if level < 0 else ze.strategy_class(strategy), f, blocks, trace))
    return out


# ---------------- the generator ----------------
def test_case_list_is_fixed_and_grouped():
    cases = ze.cases()
    assert len({c.name for c in cases}) == len(cases) >= 250
    a, b = ze.two_block(7, ze.ones(5), b"abcde"), ze.two_block(7, ze.ones(5), b"abcde")
    assert np.array_equal(a, b) and not np.array_equal(a, ze.two_block(8, ze.ones(5), b"abcde"))
    sizes = ze.by_size()
    assert sum(len(g) for g in sizes.values()) == len(cases) and len(sizes) <= 12      # a compress call per size and level
    for c in cases:
        assert c.frame.dtype == np.uint8 and not c.frame.flags.writeable
        assert c.frame.nbytes <= c.skip * ze.K + 3 * ze.K and (c.skip == 0 or c.frame.nbytes > c.skip * ze.K)


def test_dictated_block_is_as_dictated():
    """literals and copies lie where the lists say, the copies' sources are disjoint, and no copy can grow at either end"""
    rng = np.random.default_rng(11)
    hist = ze.first_block(rng)
    seqs = [(int(a), int(b)) for a, b in zip(rng.integers(0, 5, 300), rng.integers(4, 60, 300))]
    lits = rng.integers(0, 24, sum(a for a, _ in seqs) + 9).astype(np.uint8)
    blk = ze.dictated(rng, hist, seqs, lits)
    assert blk.nbytes == sum(a + b for a, b in seqs) + 9
    h = hist.tobytes()
    pos, lp, used = 0, 0, np.zeros(ze.K, bool)
    for ll, ml in seqs:
        assert np.array_equal(blk[pos:pos + ll], lits[lp:lp + ll])
        pos, lp = pos + ll, lp + ll
        s = h.find(blk[pos:pos + ml].tobytes())
        assert s >= 1 and (ml < 8 or not used[s:s + ml].any())           # short copies may occur by chance elsewhere
        if ml >= 8:
            used[s:s + ml] = True
            assert pos == 0 or hist[s - 1] != blk[pos - 1]
            assert hist[s + ml] != blk[pos + ml]
        pos += ml
    assert np.array_equal(blk[pos:], lits[lp:])
    # padding: stretched copies, or a tail behind the last literal
    assert ze.dictated(rng, hist, seqs, lits, total=40000).nbytes == 40000
    t = ze.dictated(rng, hist, seqs, lits, total=40000, pad="tail")
    assert t.nbytes == 40000 and np.array_equal(t[blk.nbytes - 9:blk.nbytes], lits[-9:]) and (t[blk.nbytes:] < 128).all()
    # one offset code
    o = ze.dictated(rng, hist, [(1, 16)] * 50, lits, of_code=16)
    pos = 0
    for _ in range(50):
        s = h.find(o[pos + 1:pos + 17].tobytes())
        assert (1 << 16) <= ze.K + pos + 1 - s + 3 < (2 << 16)
        pos += 17


def test_levels_cover_every_strategy_and_a_negative_level(oracle):
    for n in ze.by_size():
        lv = ze.levels(oracle, n)
        assert sorted(lv.values()) == [1] + list(range(1, 10)) and min(lv) < 0
        assert {ze.strategy_class(s) for s in lv.values()} == {"low", "mid", "high"}
    stock = oracle_lib.StockLibs()
    if stock.zstd is not None:                                      # the oracle's parameter table is the library's
        import seg_craft
        for n in ze.by_size():
            for level in range(-5, 23):
                if level:
                    assert seg_craft.zstd_cparams(stock, level, n)[1] == oracle.zstd_enc_strategy(level, n), (level, n)


# ---------------- the header reader ----------------
def test_walk_entropy_reads_every_field(runs):
    """against what the counters say of the same frame (single dictated block: one literal section, one sequence section)"""
    seen = set()
    for c, level, cls, f, blocks, t in runs:
        if len(blocks) != 1 or blocks[0]["type"] != "compressed":
            continue
        b = blocks[0]
        seen.add((b["lit"], b["lit_header"], b["streams"], b["nseq_bytes"]))
        assert (b["lit"] == "rle") == (t["lit_rle"] == 1 and t["lit_huf_raw"] + t["lit_mingain_raw"] == 0), (c.name, level)
        assert (b["lit"] == "compressed") == (t["lit_compressed"] == 1) and (b["lit"] == "treeless") == (t["lit_treeless"] == 1)
        assert (b["streams"] == 1) == (t["lit_single_stream"] == 1) and (b["streams"] == 4) == (t["lit_four_streams"] == 1)
        assert b["nseq_bytes"] == 1 * t["seq_count_1byte"] + 2 * t["seq_count_2bytes"] + 3 * t["seq_count_3bytes"]
        assert (b["nseq"] < 128, b["nseq"] >= 0x7F00) == (b["nseq_bytes"] == 1, b["nseq_bytes"] == 3)
        if b["lit"] == "compressed":
            assert (b["tree"] >= 128) == (t["huf_weights_direct"] >= 1 and t["huf_weights_fse"] == 0), (c.name, level)
            assert b["lit_header"] == 3 + (b["regen"] >= 1024) + (b["regen"] >= 16384) and b["lit_csize"] < b["regen"]
        if b["lit"] in ("raw", "rle"):
            assert b["lit_header"] == 1 + (b["regen"] > 31) + (b["regen"] > 4095)
        if b["modes"] is not None:
            for i, tab in enumerate(("ll", "of", "ml")):
                mode = {"predefined": "basic", "rle": "rle", "fse": "compressed", "repeat": "repeat"}[b["modes"][i]]
                assert t["%s_%s" % (tab, mode)] == 1, (c.name, level, tab, mode)
    assert {s[0] for s in seen} == {"raw", "rle", "compressed"} and {s[1] for s in seen} == {1, 2, 3, 4, 5}
    assert {s[2] for s in seen} == {None, 1, 4} and {s[3] for s in seen} == {1, 2, 3}


# ---------------- every property is reached ----------------
def test_every_property_is_reached_in_every_class_it_names(runs):
    reach = {name: {} for name in ze.PROPERTIES}
    for c, level, cls, f, blocks, t in runs:
        for name, (classes, pred) in ze.PROPERTIES.items():
            if pred(blocks, t, c.name):
                reach[name].setdefault(cls, []).append((c.name, level))
    for name, (classes, _) in ze.PROPERTIES.items():
        print("%-62s %s" % (name, "; ".join("%s: %d, first %s at level %d" % (k, len(v), v[0][0], v[0][1])
                                            for k, v in sorted(reach[name].items()))))
    missing = [(name, k) for name, (classes, _) in ze.PROPERTIES.items() for k in classes if k not in reach[name]]
    assert missing == [], missing


def test_the_optimal_parsers_shorter_list_loses_no_property(oracle, runs):
    names = {c.name for c in ze.cases()}
    assert ze.OPT_CASES <= names and len(ze.OPT_CASES) <= len(names) // 3
    for strategy in range(ze.OPT_STRATEGY, 10):
        assert {c.name for g in ze.by_size(strategy).values() for c in g} == ze.OPT_CASES
        parts = {c.name for g in ze.by_size(strategy, "single").values() for c in g}, {c.name for g in ze.by_size(strategy, "chains").values() for c in g}
        assert parts[0] | parts[1] == ze.OPT_CASES and not parts[0] & parts[1] and len(parts[1]) >= 8
        for chains in (False, True):            # what the GPU test runs in one piece: frames of one dictated block | of several
            full, short = set(), set()
            for c, level, cls, f, blocks, t in runs:
                if level < 0 or ze.levels(oracle, c.frame.nbytes)[level] != strategy or (c.frame.nbytes > 2 * ze.K) != chains:
                    continue
                hit = {name for name, (classes, pred) in ze.PROPERTIES.items() if cls in classes and pred(blocks, t, c.name)}
                full |= hit
                if c.name in ze.OPT_CASES:
                    short |= hit
            assert full - short == set() and len(short) >= (8 if chains else 65), (strategy, chains, sorted(full - short))
    assert {c.name for g in ze.by_size(ze.OPT_STRATEGY - 1).values() for c in g} == names


def test_no_case_hides_in_a_raw_block(runs):
    """at some level of every class (negative levels aside) a case's last dictated block goes out compressed, and every case
    is a reason for some property at some level: none is dead weight"""
    ok, useful = {}, set()
    for c, level, cls, f, blocks, t in runs:
        if cls != "negative":
            ok.setdefault(c.name, set())
            if blocks[-1]["type"] == "compressed":
                ok[c.name].add(cls)
        if any(pred(blocks, t, c.name) for _, pred in ze.PROPERTIES.values()):
            useful.add(c.name)
    raw_ok = {c.name for c in ze.cases() if c.raw_ok}
    hidden = sorted(n for n, classes in ok.items() if n not in raw_ok and not n.endswith("/near") and classes != {"low", "mid", "high"})
    assert hidden == [], hidden
    # the "/near" variants are there for `fast` and `dfast`: compressed below `lazy`
    assert [n for n, classes in ok.items() if n.endswith("/near") and n not in raw_ok and "low" not in classes] == []
    assert sorted({c.name for c in ze.cases()} - useful) == []


def test_unreached_branches_are_the_named_ones(oracle, runs):
    total = dict.fromkeys(oracle.zstd_enc_trace_names, 0)
    for _, _, _, _, _, t in runs:
        for k, v in t.items():
            total[k] += v
    assert {k for k, v in total.items() if v == 0} == UNREACHED
    for k in UNREACHED:
        assert k in ze.__doc__


# ---------------- the oracle on these inputs ----------------
def test_oracle_decodes_its_frames(oracle, runs):
    for c, level, cls, f, blocks, t in runs:
        r, out = oracle.zstd_decompress(f, c.frame.nbytes)
        assert r == c.frame.nbytes and np.array_equal(out, c.frame), (c.name, level)


def test_oracle_is_libzstd_on_every_case(runs):
    stock = oracle_lib.StockLibs()
    if stock.zstd is None:
        pytest.skip("libzstd.so.1 not loadable")
    assert stock.zstd.ZSTD_versionNumber() == 10408
    bad = [(c.name, level) for c, level, cls, f, blocks, t in runs if not np.array_equal(stock.zstd_compress(c.frame, level), f)]
    assert bad == [], (len(bad), bad[:10])


def test_counters_change_no_byte_and_count_from_the_block_asked(oracle):
    c = next(x for x in ze.cases() if x.name == "huf2/same/1024-1024")
    plain = oracle.zstd_compress(c.frame, 7)
    f0, t0 = oracle.zstd_compress_traced(c.frame, 7)
    f2, t2 = oracle.zstd_compress_traced(c.frame, 7, from_block=2)
    f3, t3 = oracle.zstd_compress_traced(c.frame, 7, from_block=3)
    assert np.array_equal(plain, f0) and np.array_equal(plain, f2) and np.array_equal(plain, f3)
    assert t0["block_mingain_raw"] == 2 and t2["block_mingain_raw"] == 0           # the two random blocks in front
    assert t2["block_compressed"] == 2 and t3["block_compressed"] == 1 and t3["lit_treeless"] == 1 and t2["lit_compressed"] == 1
    oracle.zstd_enc_trace_reset()
    assert not any(oracle.zstd_enc_trace().values())
    assert len(set(oracle.zstd_enc_trace_names)) == len(oracle.zstd_enc_trace_names) == oracle.L.cryo_oracle_zstd_enc_trace_count()
    assert oracle.L.cryo_oracle_zstd_enc_trace_name(-1) is None
    assert oracle.L.cryo_oracle_zstd_enc_trace_name(len(oracle.zstd_enc_trace_names)) is None
