"""CPU tests of the pattern scan keys (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE): the reference tests/like_ref.py against the hand-written
expectations of tests/like_cases.py; the greedy statement of the match -- what the kernels compute -- against the backtracking
one on seeded random pairs; cryo_filter_like_check of host/filter.h; the descriptors the Python wrapper makes; and the header's
text.  No GPU."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np

import like_cases as lc
import like_ref as lr
from like_ref import P
from pg_cryogen_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference and the hand-written expectations ----
def test_reference_says_what_the_cases_say():
    cases = lc.cases()
    assert len(cases) > 100
    for name, B, atts, blk, keys, truth, matches, bad in cases:
        assert lr.desc_ok(atts, keys, lr.tr.TRUTH if truth is not None else 0, truth or 0), name
        table, recs, packed, total = lr.filter_call([blk], atts, keys, 0, truth)
        assert [int(r["pos"]) for r in recs if r["status"] == 0] == matches, name
        assert {int(r["pos"]): int(r["status"]) for r in recs if r["status"]} == bad, name
        assert (table["n_match"][0], table["n_bad"][0]) == (len(matches), len(bad)), name
        rows, cells = lr.agg_call([blk], atts, keys, [(1, lr.INT4)], truth)
        assert (rows["n_match"][0], rows["n_bad"][0], cells["n"][0, 0]) == (len(matches), len(bad), len(matches)), name


def test_both_ops_are_false_on_null_and_each_other_s_negation_elsewhere():
    for name, B, atts, blk, keys, truth, matches, bad in lc.cases():
        if len(keys) != 1 or truth is not None or name == "290 items":
            continue
        att, typ, op, p = keys[0]
        other = [(att, typ, lr.LIKE + lr.NOT_LIKE - op, p)]
        a, b = lr.filter_call([blk], atts, keys)[1], lr.filter_call([blk], atts, other)[1]
        hit_a, hit_b = set(a["pos"][a["status"] == 0].tolist()), set(b["pos"][b["status"] == 0].tolist())
        assert not hit_a & hit_b, name
        assert a["pos"][a["status"] != 0].tolist() == b["pos"][b["status"] != 0].tolist(), name     # the same values are undecided


def test_the_two_character_rules():
    assert lr.match("é".encode(), b"_", True) and not lr.match("é".encode(), b"_", False) and lr.match("é".encode(), b"__", False)
    assert lr.step(b"\xe2\x82\xacx", 0, True) == 3 and lr.step(b"\xe2\x82\xacx", 0, False) == 1
    assert lr.step(b"\x80\x80\x80", 1, True) == 3                            # from where it stands, whatever stands there
    assert lr.step(b"\xc3", 0, True) == 1                                    # never past the end
    assert lr.tokens(b"a\\%_%") == [(lr.LIT, 97), (lr.LIT, 37), (lr.ANY, None), (lr.RUN, None)]
    assert lr.tokens(b"abc\\") is None and lr.tokens(b"\\\\") == [(lr.LIT, 92)] and lr.tokens(b"\\\\\\") is None


# ---- greedy by segments is the same relation ----
def random_pair(rnd, utf8):
    """(text, pattern): texts over a small alphabet with the bytes of 'é' and '€' loose in it -- most are no valid UTF-8 --;
    patterns of '%', '_', escapes and literals.  Under the flag a pattern's literals are whole characters, as a database's own
    text is; without it any byte is a character and the pattern takes the same loose bytes"""
    loose = [0xC3, 0xA9, 0x80, 0xE2, 0x82, 0xAC]
    text = bytes(rnd.choice([97, 98, 97, 98, 99] + loose + [37, 95, 92]) for _ in range(rnd.randrange(12)))
    pat = bytearray()
    for _ in range(rnd.randrange(8)):
        r = rnd.randrange(12)
        if r < 3:
            pat += b"%"
        elif r < 5:
            pat += b"_"
        elif r < 6:
            pat += b"\\" + bytes([rnd.choice(b"%_\\a")])
        elif r < 8:
            pat += rnd.choice(["é".encode(), "€".encode()]) if utf8 else bytes([rnd.choice(loose)])
        else:
            pat += bytes([rnd.choice(b"abc")])
    return text, bytes(pat)


def test_greedy_by_segments_agrees_with_backtracking():
    rnd = random.Random(20261021)
    n, hits, invalid = 60000, 0, 0
    for i in range(n):
        utf8 = bool(i & 1)
        text, pat = random_pair(rnd, utf8)
        want = lr.match(text, pat, utf8)
        assert lr.greedy(text, pat, utf8) == want, (text, pat, utf8, want)
        hits += want
        try:
            text.decode("utf-8")
        except UnicodeDecodeError:
            invalid += 1
    print("pairs %d, matching %d (%.1f %%), texts that are no valid UTF-8 %d" % (n, hits, 100.0 * hits / n, invalid))
    assert 0.02 * n <= hits <= 0.60 * n                                      # neither answer dominates
    assert invalid > n // 4


def test_greedy_on_the_hand_made_values():
    for text, pat, utf8, want in ((b"abab", b"%ab%ab", True, True), (b"ab", b"%ab%ab", True, False), (b"aaab", b"%aab", True, True),
                                  (b"", b"", True, True), (b"", b"%", False, True), (b"x", b"", False, False), (b"\x80\x80", b"_", True, True),
                                  (b"\x80\x80", b"_", False, False), (b"xayaz", b"x%ay", True, False)):
        assert lr.greedy(text, pat, utf8) == lr.match(text, pat, utf8) == want, (text, pat, utf8)


def test_a_pattern_that_splits_a_character_has_the_greedy_answer():
    """under the flag a '%' between the two bytes of a character: the first segment's leftmost place ends inside the first
    character, from where the second is not found at a character start; trying every run would place it in the second.  The
    header defines the greedy answer; without the flag, where every byte is a start, the two agree"""
    text, pat = b"\xc3\x80\xc3\x80x", b"%\xc3%\x80x"
    assert lr.greedy(text, pat, True) is False and lr.match(text, pat, True) is True
    assert lr.greedy(text, pat, False) is True and lr.match(text, pat, False) is True


# ---- the binder's check ----
def test_like_check_of_the_host_header(tmp_path):
    """cryo_filter_like_check of host/filter.h in a small program of its own: hex patterns in, reasons out"""
    src = tmp_path / "check.c"
    src.write_text("""
#include "filter.h"
#include <stdio.h>
#include <stdlib.h>
int main(void)
{
    static char line[4096];
    static unsigned char pat[2048];
    while (fgets(line, sizeof line, stdin)) {
        uint32_t n = 0;
        unsigned int b;
        char *p = line;
        while (sscanf(p, "%2x", &b) == 1) { pat[n++] = (unsigned char)b; p += 2; }
        printf("%d\\n", cryo_filter_like_check(pat, n));
    }
    printf("%d %d %d\\n", cryo_filter_like_check(0, 0), cryo_filter_like_check(0, 1), cryo_filter_like_check("x", 257));
    return 0;
}
""")
    exe = tmp_path / "check"
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "pg_cryogen_amd", "host"),
                    "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    pats = [b"", b"abc", b"%", b"a\\", b"\\", b"\\\\", b"\\\\\\", b"a\\%", b"x" * 256, b"x" * 257, b"x" * 255 + b"\\", b"x" * 254 + b"\\\\",
            b"\\" * 256, b"\\" * 255]
    out = subprocess.run([str(exe)], input="".join(p.hex() + "\n" for p in pats), capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    assert out[len(pats)] == "0 1 1"
    for p, got in zip(pats, out):
        want = 1 if len(p) > lr.PATTERN_MAX else 2 if lr.tokens(p) is None else 0
        assert int(got) == want, (p, got)
    assert [int(x) for x in out[:7]] == [0, 0, 0, 2, 2, 0, 2]               # as written by hand


# ---- the descriptor ----
def test_descriptor_rules():
    for name, atts, keys, key_rsv, ok in lc.descriptors():
        assert lr.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
        n = len(keys)
        assert lr.desc_ok(atts, keys, lr.tr.TRUTH, (1 << (1 << min(n, 4))) - 1, key_rsv) == (ok and n >= 1), name
    names = [d[0] for d in lc.descriptors()]
    assert {"op 11 on an integer key", "op 9 on a byte-string key", "rsv bit 17", "a trailing escape", "257 bytes"} <= set(names)


def test_wrapper_descriptors_host_and_device_form():
    keys = [(3, codec.KEY_BYTES, codec.OP_LIKE, codec.like("%é_")), (1, codec.KEY_INT4, codec.OP_EQ, 7),
            (5, codec.KEY_BYTES, codec.OP_NOT_LIKE, codec.like(b"bot%", utf8=False)), (3, codec.KEY_BYTES, codec.OP_EQ, b"de")]
    f, a, k = codec.filter_desc(lc.ATTS, keys, truth=0xFFFE)
    assert (f.natts, f.nkeys, f.flags, f.rsv) == (5, 4, codec.FILTER_TRUTH, 0xFFFE)
    assert k["op"].tolist() == [11, codec.OP_EQ, 12, codec.OP_EQ]
    assert k["type"].tolist() == [16, codec.KEY_INT4, 16, 16]
    assert k["rsv"].tolist() == [4 | codec.LIKE_UTF8, 0, 4, 2]              # '%é_' is four bytes
    assert C.string_at(int(k["value"][0]), 4) == "%é_".encode() and C.string_at(int(k["value"][2]), 4) == b"bot%"
    assert C.string_at(int(k["value"][3]), 2) == b"de" and k["value"][1] == 7
    assert bytes(f.consts[:10]) == "%é_".encode() + b"bot%" + b"de"          # back to back, in key order
    a, k, consts, rebase = codec.filter_desc_device(lc.ATTS, keys)
    assert bytes(consts[:10]) == "%é_".encode() + b"bot%" + b"de"
    assert rebase(4096) is k and k["value"].tolist() == [4096, 7, 4100, 4104]
    assert rebase(8193)["value"].tolist() == [8193, 7, 8197, 8201]          # any alignment
    # the empty pattern and the null pattern keep a null address; rsv as given goes through untouched
    f, a, k = codec.filter_desc(lc.ATTS, [(3, 16, 11, codec.like(b"")), (3, 16, 11, codec.like(None, rsv=3)), (3, 16, 12, codec.like(b"ab", rsv=1 << 17 | 2))])
    assert k["value"][0] == 0 and k["value"][1] == 0 and k["value"][2] != 0
    assert k["rsv"].tolist() == [codec.LIKE_UTF8, 3, 1 << 17 | 2]
    assert len(codec.like("é")) == 2 and codec.like("é").pattern == b"\xc3\xa9" and codec.like(b"x", utf8=False).rsv == 1
    assert (codec.OP_LIKE, codec.OP_NOT_LIKE, codec.LIKE_UTF8, codec.LIKE_TEXT_MAX) == (lr.LIKE, lr.NOT_LIKE, lr.UTF8, lr.TEXT_MAX)
    assert P is codec.like


# ---- the header ----
def test_header_states_the_rule():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"\bCRYO_OP_LIKE = 11, CRYO_OP_NOT_LIKE = 12\b", txt)
    assert re.search(r"^#define CRYO_LIKE_UTF8 0x10000u\b", txt, flags=re.M) and re.search(r"^#define CRYO_LIKE_TEXT_MAX 2048u\b", txt, flags=re.M)
    assert re.search(r"^#define CRYO_KEY_BYTES_MAX 256u\b", txt, flags=re.M)
    flat = " ".join(txt.replace("\n *", " ").split())
    for phrase in ("Pattern keys.", "CRYO_OP_LIKE (11) and CRYO_OP_NOT_LIKE (12)", "bit 16 of rsv is CRYO_LIKE_UTF8",
                   "'%' matches any run of characters, the empty run included", "'_' matches exactly one character",
                   "one byte plus every byte 10xxxxxx (0x80 .. 0xBF) that directly follows it", "'%' tries character starts only",
                   "longer than CRYO_LIKE_TEXT_MAX (2048) bytes", "cannot stall a shared machine", "a pattern whose last byte is an unescaped",
                   "deterministic collation", "iff the database encoding is UTF8", "no ILIKE, no SIMILAR TO, no regular expressions",
                   "cryo_filter_like_check"):
        assert phrase in flat, phrase
    helper = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "filter.h")).read()
    assert "cryo_filter_like_check(const void *pattern, uint32_t n)" in helper
    walk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "filter_walk.h")).read()
    assert "kLikeTextMax = 2048u" in walk and "kOpLike = 11, kOpNotLike = 12" in walk


def test_cases_cover_what_the_issue_names():
    names = " | ".join(c[0] for c in lc.cases())
    for part in ("the empty pattern", "'%' matches every value", "'%%' is '%'", "'%_%'", "anchored at both ends", "a leading '%' alone",
                 "a trailing '%' alone", "occurs twice", "the overlap trap", "escaped '%', '_' and backslash", "256 bytes", "255 bytes",
                 "128 one-byte segments", "7, 8, 9, 126 and 127", "a 4-byte header", "2047 and 2048", "the pad is not read",
                 "the next column is not read", "2, 3 and 4 bytes", "continuation bytes and a truncated lead", "without the flag",
                 "NULL, external, compressed: LIKE AND", "NULL, external, compressed: LIKE OR", "NOT LIKE", "two pattern keys on one column",
                 "a pattern key on each of two columns"):
        assert part in names, part
    sizes = {c[1] for c in lc.cases()}
    assert {4096, 131072} <= sizes
    assert np.array_equal(np.frombuffer(lc.SEGMENTS_128, np.uint8)[1::2], np.full(127, 37, np.uint8)) and len(lc.SEGMENTS_128) == 255
