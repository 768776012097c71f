"""CPU tests: the oracle decoders against the stock liblz4 1.9.3 / libzstd 1.4.8 on crafted LZ4 streams
(tests/lz4_craft.py), non-default zstd frames (tests/zstd_craft.py) and hand-assembled zstd frames (tests/zstd_asm.py), and
the corpora hold what they claim.  The same corpora run through every device decode route in
tests/test_gpu_decode_conformance.py."""
import hashlib

import numpy as np
import pytest

import lz4_craft
import oracle_lib
import zstd_asm
import zstd_craft

LZ4_SIZES = [(4096, 300), (32768, 300), (131072, 300), (300001, 150), (1 << 20, 12)]
LZ4_SEED = 1
ZSTD_SEED = 5
CRAFT_SEED = 11


@pytest.fixture(scope="module")
def stock():
    s = oracle_lib.StockLibs()
    if s.lz4 is None or s.zstd is None:
        pytest.skip("stock liblz4/libzstd not present")
    return s


def _digest(items):
    h = hashlib.sha256()
    for it in items:
        for x in it:
            h.update(x.tobytes() if isinstance(x, np.ndarray) else repr(x).encode())
    return h.hexdigest()


@pytest.mark.parametrize("B,n", LZ4_SIZES)
def test_lz4_oracle_equals_liblz4_on_crafted_streams(oracle, stock, B, n):
    streams = lz4_craft.corpus(B, n, LZ4_SEED)
    ok = heavy = one_walker = 0
    for name, m in streams:
        r1, o1 = stock.lz4_decompress(m, B, fill=0xA5)
        r2, o2 = oracle.lz4_decompress(m, B, fill=0xA5)
        assert (r1 == B) == (r2 == B), (B, name)
        if r2 == B:
            assert np.array_equal(o1, o2), (B, name)
            ok += 1
            heavy += abs(len(m) - (B - B // 16)) <= 1
            one_walker += len(m) in (16383, 16384)
    # about a third accepted; the steered sizes hit the hand-off thresholds with accepted streams
    assert n // 5 <= ok <= n // 2, (B, ok, n)
    assert heavy >= (1 if B == 1 << 20 else 6), (B, heavy)
    if 16384 < B < (1 << 20):
        assert one_walker >= 4, (B, one_walker)


def test_lz4_crafted_streams_cover_the_decoder_rules(oracle):
    """each end the generator writes gets the verdicts the decoder rules give it: a last match may end 5 or more bytes
    before the block end, not 4 or 0; a tail one byte short or long is rejected"""
    B = 32768
    verdicts = {}
    for name, m in lz4_craft.corpus(B, 300, LZ4_SEED):
        r, _ = oracle.lz4_decompress(m, B)
        verdicts.setdefault(name.split("/")[0], set()).add(r == B)
    for end in ("tail_exact", "match_end_12", "match_end_6", "match_end_5"):
        assert True in verdicts[end], end
    for end in ("match_end_4", "match_end_0", "tail_short", "tail_long"):
        assert verdicts[end] == {False}, end
    assert verdicts["tail_exact"] == {True, False}


def test_lz4_corpus_is_deterministic():
    for B, n in LZ4_SIZES[:3]:
        assert _digest(lz4_craft.corpus(B, n, LZ4_SEED)) == _digest(lz4_craft.corpus(B, n, LZ4_SEED)), B
    assert _digest(lz4_craft.corpus(4096, 50, 2)) != _digest(lz4_craft.corpus(4096, 50, 3))


@pytest.fixture(scope="module")
def zcorpus(oracle, stock):
    return zstd_craft.zstd_corpus(stock, oracle, ZSTD_SEED)


def test_zstd_oracle_equals_libzstd_on_nondefault_frames(oracle, stock, zcorpus):
    n_ok = n_bad = 0
    for name, B, f in zcorpus:
        r1, o1 = stock.zstd_decompress(f, B, fill=0xA5)
        r2, o2 = oracle.zstd_decompress(f, B, fill=0xA5)
        assert (r1 == B) == (r2 == B), (name, B, r1, r2)
        if r2 == B:
            assert np.array_equal(o1, o2), (name, B)
            n_ok += 1
        else:
            n_bad += 1
    assert n_ok >= 200 and n_bad >= 60, (n_ok, n_bad)
    verdict = {name: None for name, _, _ in zcorpus}
    for name, B, f in zcorpus:
        ok = oracle.zstd_decompress(f, B)[0] == B
        verdict[name] = ok if verdict[name] in (None, ok) else "both"
    assert all(verdict[k] is False for k in verdict if k.startswith(("checksum_bitflip", "checksum_of_other_data")))
    assert all(verdict[k] is True for k in verdict if k.startswith(("checksum/", "wlog", "no_content_size", "litmode",
                                                                  "minmatch3", "ldm", "few_sequences")))


def test_zstd_corpus_coverage(oracle, zcorpus):
    """what the corpus claims, counted on frames the oracle accepts"""
    cov = {"treeless": 0, "checksum": 0, "nbmax": 0, "nbmax+1": 0, "no_content_size": 0,
           "repeat": [0, 0, 0], "rle": [0, 0, 0], "raw_lits": 0, "min_window_log": 99}
    for name, B, f in zcorpus:
        if oracle.zstd_decompress(f, B)[0] != B:
            continue
        w = zstd_craft.walk(f)
        assert w is not None and w["end"] == len(f), name
        cov["checksum"] += w["checksum"]
        cov["no_content_size"] += not w["content_size"]
        if w["window_log"] is not None:
            cov["min_window_log"] = min(cov["min_window_log"], w["window_log"])
        nb, nm = len(w["blocks"]), zstd_craft.zstd_nbmax(B)
        cov["nbmax"] += nb == nm
        cov["nbmax+1"] += nb == nm + 1
        for blk in w["blocks"]:
            cov["treeless"] += blk.get("lit") == "treeless"
            cov["raw_lits"] += blk.get("lit") == "raw"
            for k, mode in enumerate(blk.get("modes") or ()):
                cov["repeat"][k] += mode == "repeat"
                cov["rle"][k] += mode == "rle"
    assert cov["treeless"] >= 50, cov
    assert min(cov["repeat"]) >= 20, cov
    assert sum(cov["rle"]) >= 5, cov
    assert cov["checksum"] >= 15, cov
    assert cov["nbmax"] >= 2 and cov["nbmax+1"] >= 2, cov
    assert cov["no_content_size"] >= 4 and cov["raw_lits"] >= 20 and cov["min_window_log"] == 10, cov


def test_zstd_walker_on_known_frames(oracle, stock):
    """the walker against frames whose structure is known: block counts follow the window, the checksum flag is read"""
    raw = oracle.synth(0, 1, 262145, 0)
    f = stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_WINDOWLOG: 16, oracle_lib.ZSTD_C_CHECKSUM_FLAG: 1})
    w = zstd_craft.walk(f)
    assert w["checksum"] and w["window_log"] == 16 and len(w["blocks"]) == 5 and w["end"] == len(f)
    f = stock.zstd_compress(raw[:131072], 3)
    w = zstd_craft.walk(f)
    assert not w["checksum"] and len(w["blocks"]) == 1 and w["end"] == len(f)
    assert zstd_craft.walk(f[:len(f) - 1]) is None


def test_zstd_corpus_is_deterministic(oracle, stock, zcorpus):
    assert _digest(zcorpus) == _digest(zstd_craft.zstd_corpus(stock, oracle, ZSTD_SEED))


# ---------------- hand-assembled zstd frames (tests/zstd_asm.py) ----------------
@pytest.fixture(scope="module")
def crafted():
    return zstd_asm.crafted_cases(CRAFT_SEED)


def test_crafted_zstd_frames_library_oracle_and_model_agree(oracle, stock, crafted):
    """libzstd's verdict is the declared one, the oracle's is libzstd's, and an accepted frame's bytes are the same from
    libzstd, the oracle and the assembler's model"""
    for name, B, f, declared, fr in crafted:
        r1, o1 = stock.zstd_decompress(f, B, fill=0xA5)
        r2, o2 = oracle.zstd_decompress(f, B, fill=0xA5)
        assert (r1 == B) == declared, (name, B, r1, declared)
        assert (r2 == B) == (r1 == B), (name, B, r1, r2)
        if declared:
            assert np.array_equal(o1, o2), (name, B)
            if fr is not None:
                assert np.array_equal(o1, fr.content), (name, B)
    # the two cases made of more than one frame: the model is the content of the parts
    two = [c for c in crafted if c[0] == "E/two_frames"][0]
    assert two[4] is None and stock.zstd_decompress(two[2], two[1])[0] == two[1]


def test_crafted_zstd_corpus_coverage(crafted):
    """what the corpus claims, from the assembler's bookkeeping and the structure walk of the bytes it wrote"""
    names = [c[0] for c in crafted]
    assert len(set(names)) == len(names)
    accepted = [c for c in crafted if c[3]]
    rejected = [c for c in crafted if not c[3]]
    assert 0.55 <= len(accepted) / len(crafted) <= 0.80, (len(accepted), len(crafted))
    for fam in zstd_asm.FAMILIES:
        assert any(c[0].startswith(fam) for c in accepted), fam
    for letter in "ABCDE":
        assert any(c[0].startswith(letter + "/") for c in accepted) and any(c[0].startswith(letter + "/") for c in rejected)
    for edge in zstd_asm.REJECT_EDGES:
        assert any(c[0].startswith(edge) for c in rejected), edge
    for c in rejected:                     # the rejected cases are the named edges and nothing else
        assert c[0].startswith(zstd_asm.REJECT_EDGES), c[0]
    forms, floor = set(), 0
    modes = {"rle": [0, 0, 0], "repeat": [0, 0, 0], "fse": [0, 0, 0], "predefined": [0, 0, 0]}
    lit = {t: 0 for t in zstd_craft.LIT_TYPES}
    for name, B, f, _, fr in accepted:
        if fr is None:
            continue
        w = zstd_craft.walk(f)
        assert w is not None and w["end"] == len(f) and len(w["blocks"]) == fr.stats["nblocks"], name
        forms |= fr.stats["count_forms"]
        floor += fr.stats["floor"]
        for blk in w["blocks"]:
            assert not blk.get("broken"), name
            if blk["type"] == "compressed":
                lit[blk["lit"]] += 1
            for k, mode in enumerate(blk.get("modes") or ()):
                modes[mode][k] += 1
        for k in range(3):                 # the walk of the bytes sees the modes the assembler says it wrote
            seen = set(blk["modes"][k] for blk in w["blocks"] if blk.get("modes"))
            assert seen == fr.stats["modes"][k], (name, k, seen, fr.stats["modes"][k])
    assert forms == {1, 2, 3}, forms
    assert min(modes["rle"]) >= 1 and min(modes["repeat"]) >= 1 and min(modes["fse"]) >= 1, modes
    assert min(lit.values()) >= 1, lit
    assert floor >= 50, floor
    by_name = {c[0]: c for c in crafted}
    # k_zlat_count's edges: the totals the names state, from the formula of make_layout
    nmax = zstd_asm.lat_nmax(32768)
    assert nmax == (32768 // 4 + 2 * zstd_craft.zstd_nbmax(32768) + 255) // 256 * 256
    for total in (511, 512, nmax, nmax + 1):
        c = by_name["B/lat_total/%d" % total]
        assert c[1] == 32768 and c[3] and c[4].stats["lat_total"] == total
    assert 511 * 64 < 32768 <= 512 * 64
    for j in range(2):
        assert by_name["B/wide_sequences/%d" % j][4].stats["max_seq_bits"] > 57
    for size in (131071, 131072):          # the compressed block behind the RLE block states this size, and has it
        w = zstd_craft.walk(by_name["B/full_block_%d" % size][2])
        assert [b["size"] for b in w["blocks"]] == [131072, size] and w["end"] == len(by_name["B/full_block_%d" % size][2])
    assert by_name["B/third_of_B/0"][4].stats["lat_total"] == 4096 // 3 + 1
    nbm = zstd_craft.zstd_nbmax(4096)
    assert sum(c[0].startswith("E/order%d/" % nbm) for c in accepted) == 3 ** nbm
    assert sum(c[0].startswith("E/order%d/" % (nbm + 1)) for c in accepted) == 3 ** (nbm + 1)
    assert sorted(set(c[1] for c in crafted)) == [255, 256, 4096, 8192, 32768, 65791, 131072, 262144]
    assert [c[0] for c in crafted if c[1] == 262144] == ["B/full_block_131071", "B/full_block_131072"]


def test_crafted_family_a_reaches_the_floor_and_the_shift(stock, crafted):
    """the model without the "rep0 - 1 = 0 -> 1" floor, and without the ll = 0 shift of the repeat codes, each disagrees with
    libzstd on family-A frames: the family reaches both rules"""
    no_floor = no_shift = 0
    for name, B, f, declared, fr in crafted:
        if not (name.startswith("A/") and declared):
            continue
        r, o = stock.zstd_decompress(f, B)
        assert r == B and np.array_equal(fr.model(), o), name
        for kw in ({"floor": False}, {"shift": False}):
            m = fr.model(**kw)
            differs = m is None or len(m) != B or not np.array_equal(m, o)
            if "floor" in kw:
                assert differs == (fr.stats["floor"] > 0), name
                no_floor += differs
            else:
                no_shift += differs
    assert no_floor >= 11 and no_shift >= 11, (no_floor, no_shift)


def test_crafted_zstd_corpus_is_deterministic(crafted):
    a = [c[:4] for c in crafted]
    assert _digest(a) == _digest(zstd_asm.crafted_corpus(CRAFT_SEED))
    assert _digest(a) != _digest(zstd_asm.crafted_corpus(CRAFT_SEED + 1))

