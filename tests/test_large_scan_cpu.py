"""The cases of tests/large_scan_cases.py against the references alone (no GPU): what tests/test_gpu_large_scan.py compares the
kernels with is pinned here by expectations written out by hand -- the OVERLAP verdicts of the aliased blocks and the two
congruences mod 2^32 they stand on, the per-position verdicts of mixed() -- and every reference call is timed."""
import struct

import numpy as np
import pytest

import bytes_key_ref
import fetch_ref
import filter_ref
import float_ref as fl
import large_scan_cases as ls
import layout_ref
from large_scan_cases import TWO24, TWO32

CALLS = ["filter", "count", "agg", "group", "project"]
SECONDS = 5.0                                             # "a few seconds": the most one reference call on one block may take


def same(got, want, what):
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what
        else:
            assert tuple(np.atleast_1d(g).tolist()) == tuple(np.atleast_1d(w).tolist()), what


def header(block):
    return struct.unpack_from("<II", block, 0)


# ---- the aliased blocks ----
@pytest.mark.parametrize("n", [256, 257])
def test_the_aliased_sums_wrap_to_fits(oracle, n):
    """the construction: n items on one tuple whose MAXALIGNed length is 2^24, in a block with B - upper = 2^24"""
    c = ls.case(oracle, "aliased%d" % n)
    lower, upper = header(c.block)
    assert (lower, upper, c.B) == (8 + 8 * n, 8 + 8 * n, 8 + 8 * n + TWO24)
    items = c.block[8:lower].view("<u4").reshape(n, 2)
    assert (items[:, 0] == upper).all() and (items[:, 1] == TWO24 - 6).all()
    total = sum(layout_ref.maxalign(int(ln)) for ln in items[:, 1])
    room = c.B - upper
    assert total > room                                                   # the rule: OVERLAP
    if n == 256:
        assert total == TWO32 and total % TWO32 == 0                      # a 32-bit sum is 0: "fits"
    else:
        assert total == TWO32 + TWO24 and total % TWO32 == room           # a 32-bit sum is B - upper exactly: "fits"
    assert total % TWO32 <= room


@pytest.mark.parametrize("n,status", [(256, 7), (257, 7), (1, 0)])
def test_aliased_verdicts(oracle, n, status):
    c = ls.case(oracle, "aliased%d" % n)
    table, recs, packed, total = ls.expected(c, "int", "filter")
    assert status == (fl.OVERLAP if n > 1 else fl.OK)
    assert int(table["status"][0]) == status and int(table["n_items"][0]) == n and int(table["n_bad"][0]) == 0
    if n > 1:
        assert int(table["n_match"][0]) == 0 and recs.size == 0 and packed.size == 0 and total == (0, 0)
    else:
        assert int(table["n_match"][0]) == 1 and total == (TWO24, 1) and tuple(recs[0]) == (1, 0, TWO24 - 6)
        assert packed[:TWO24 - 6].tobytes() == ls.long_tuple() and not packed[TWO24 - 6:].any()
    # filter_ref itself, which knows integer keys alone, says the same
    same(ls.integer_only(c, "int", "filter"), (table, recs, packed, total), "filter_ref")
    # the count, the aggregate, the grouping and the projection do not apply OVERLAP: n matches
    assert tuple(ls.expected(c, "int", "count")[0][0])[:4] == (0, n, n, 0)
    rows, cells = ls.expected(c, "int", "agg")
    assert tuple(rows[0]) == (0, n, n, 0)
    k, x, g = cells[0]
    assert int(k["n"]) == n and (int(k["sum_hi"]) << 64) + int(k["sum_lo"]) == n * ls.LONG_K and int(k["min"]) == int(k["max"]) == ls.LONG_K
    assert int(x["n"]) == 0 and x.tobytes() == bytes(40)                                    # x is NULL in the long tuple
    assert int(g["n"]) == n and int(g["sum_lo"]) == 3 * n
    rows, grecs, gcells, groups = ls.expected(c, "int", "group")
    assert groups == 1 and int(rows["n_groups"][0]) == 1 and int(grecs["n_rows"][0]) == n and int(grecs["key"][0][0]) == 3
    assert (int(gcells[0, 0]["sum_hi"]) << 64) + int(gcells[0, 0]["sum_lo"]) == n * ls.LONG_K
    ptable, precs, prows, ptotal = ls.expected(c, "int", "project")
    assert ptotal == (n, n) and int(ptable["status"][0]) == 0 and prows.shape == (n, 32)
    one = struct.pack("<qh6xqi4x", ls.LONG_K, 3, 0, 7)                                      # k, g, x (NULL: zero), id
    assert all(r.tobytes() == one for r in prows) and (precs["nulls"] == 4).all() and precs["pos"].tolist() == list(range(1, n + 1))
    for call in ("count", "agg", "group", "project"):
        want = ls.expected(c, "int", call)
        got = ls.integer_only(c, "int", call)
        if call in ("agg", "group"):                                                        # the integer columns: k and g
            cells = want[1] if call == "agg" else want[2]
            want = (want[0], cells[:, [0, 2]]) if call == "agg" else (want[0], want[1], cells[:, [0, 2]], want[3])
        same(got, want, ("integer-only reference", call))
    # the fetch of every position: OVERLAP for each request, nothing packed
    rec, packed, total = ls.fetch_expected(c, list(range(1, n + 1)))
    if n > 1:
        assert (rec["status"] == fetch_ref.OVERLAP).all() and total == 0 and packed.size == 0 and not rec["len"].any()
    else:
        assert tuple(rec[0]) == (0, TWO24 - 6, 0) and total == TWO24


# ---- mixed() ----
def test_mixed_construction(oracle):
    c = ls.case(oracle, "mixed")
    b = c.block
    lower, upper = header(b)
    assert c.B == 4 * ls.MIB + 24 and lower == 8 + 8 * ls.MIXED_N
    items = [struct.unpack_from("<II", b, 8 + 8 * i) for i in range(ls.MIXED_N)]
    w = [bytes_key_ref.walk(b[off:off + ln].tobytes(), ls.ATTS, 5) for off, ln in items[:12]]
    assert all(x is not None for x in w)
    sizes = [x[1][2] for x in w[:9]]                                     # the varlena's size, header included
    assert sizes == [1, 127, 131, 260, 65535, 65536, 65537, ls.MIB + 5, 5 * ls.MIB // 2 + 4]
    heads = [int(b[items[i][0] + w[i][1][1]]) & 1 for i in range(9)]
    assert heads == [1, 1, 0, 0, 0, 0, 0, 0, 0]                          # 126 payload bytes is the last 1-byte header
    assert [x[2][1] for x in w[4:9]] == [65568, 65568, 65568, ls.MIB + 40, 5 * ls.MIB // 2 + 32]   # k above 2^16 and 2^20
    assert [x[4][1] for x in w[4:9]] == [65584, 65584, 65584, ls.MIB + 56, 5 * ls.MIB // 2 + 48]   # x as well
    assert w[9][1][0] and w[10][1][2] == 18 and w[11][3][0] and w[11][4][0]  # NULL body; TOAST; g and x beyond the attributes
    off, ln = items[12]
    assert (struct.unpack_from("<I", b, off + 28)[0] >> 2) - (ln - 28) == 4  # 4 bytes short
    off, ln = items[13]
    assert struct.unpack_from("<I", b, off + 28)[0] >> 2 == 0x3FFFFFFF
    assert items[0][0] + layout_ref.maxalign(items[0][1]) == c.B
    assert items[14][0] + layout_ref.maxalign(items[14][1]) == c.B + 8 and items[14][0] >= upper
    assert upper == items[13][0]


@pytest.mark.parametrize("keyset", list(ls.KEYSETS))
def test_mixed_verdicts_by_hand(oracle, keyset):
    c = ls.case(oracle, "mixed")
    hand = ls.MIXED_VERDICTS[keyset]
    assert len(hand) == ls.MIXED_N and "M" in hand and "-" in hand
    if keyset in ("int", "bytes_gt", "float"):                               # both among the tuples above 2^16 bytes; the byte
        assert "M" in hand[4:9] and "-" in hand[4:9]                         # strings tell them from the short ones instead
    table, recs, packed, total = ls.expected(c, keyset, "filter")
    code = {0: "M", fl.ITEM: "I", fl.TUPLE: "T", fl.UNDECIDED: "U"}
    got = ["-"] * ls.MIXED_N
    for r in recs:
        got[int(r["pos"]) - 1] = code[int(r["status"])]
    assert "".join(got) == hand
    assert tuple(table[0])[:4] == (0, ls.MIXED_N, hand.count("M"), ls.MIXED_N - hand.count("M") - hand.count("-"))
    # the bytes: every match whole, in position order
    at = 0
    for r in recs[recs["status"] == 0]:
        off, ln = struct.unpack_from("<II", c.block, 8 * int(r["pos"]))
        assert int(r["len"]) == ln and packed[at:at + ln].tobytes() == c.block[off:off + ln].tobytes()
        at += layout_ref.maxalign(ln)
    assert at == total[0] == packed.size
    # the other calls walk to x: the short tuple stays good (its g and x are NULL), nothing else changes
    n_bad = hand.count("T") + hand.count("I") + hand.count("U")
    assert tuple(ls.expected(c, keyset, "count")[0][0])[:4] == (0, ls.MIXED_N, hand.count("M"), n_bad)
    assert tuple(ls.expected(c, keyset, "agg")[0][0]) == (0, ls.MIXED_N, hand.count("M"), n_bad)
    ptable, precs, prows, ptotal = ls.expected(c, keyset, "project")
    assert ptotal == (hand.count("M"), hand.count("M") + n_bad)
    ks = [r[1] for r in ls.MIXED_ROWS] + [-8, -9, -10]
    want_k = [ks[i] for i in range(12) if hand[i] == "M"]
    assert [struct.unpack_from("<q", r.tobytes(), 0)[0] for r in prows] == want_k
    rows, cells = ls.expected(c, keyset, "agg")
    assert int(cells[0, 0]["n"]) == len(want_k)
    assert (int(cells[0, 0]["sum_hi"]) << 64) + int(cells[0, 0]["sum_lo"]) == sum(want_k)


def test_a_longer_constant_is_refused(oracle):
    """why the constants are 256 bytes: CRYO_KEY_BYTES_MAX; one byte more is no valid descriptor"""
    assert len(ls.PREFIX) == len(ls.NEAR_LOW) == len(ls.NEAR_HIGH) == bytes_key_ref.BYTES_MAX == 256
    assert fl.desc_ok(ls.ATTS, [(ls.BODY, fl.BYTES, fl.GT, ls.PREFIX)])
    assert not fl.desc_ok(ls.ATTS, [(ls.BODY, fl.BYTES, fl.GT, ls.text(257))])
    assert not fl.desc_ok(ls.ATTS, [(ls.BODY, fl.BYTES, fl.GT, ls.text(4000))])
    assert ls.text(4000)[:256] == ls.PREFIX and ls.NEAR_LOW[:255] == ls.PREFIX[:255] == ls.NEAR_HIGH[:255]
    assert ls.NEAR_LOW[255] + 1 == ls.PREFIX[255] == ls.NEAR_HIGH[255] - 1


# ---- every block ----
CHECKS = {"aliased256": (layout_ref.ITEM, 16), "aliased257": (layout_ref.ITEM, 16), "aliased1": (layout_ref.OK, layout_ref.NONE),
          "mixed": (layout_ref.ITEM, 8 + 8 * 14), "wide1m": (layout_ref.OK, layout_ref.NONE), "wide4m": (layout_ref.OK, layout_ref.NONE)}


@pytest.mark.parametrize("name", ls.NAMES)
def test_layout_check_and_descriptors(oracle, name):
    """the stored-block check's word on every block (the second alias breaks the chain rule; mixed()'s last item does), the
    neighbours are well formed, and every descriptor is one the rules accept"""
    c = ls.case(oracle, name)
    assert layout_ref.check_block(c.block) == CHECKS[name]
    nb = ls.neighbour(oracle, c)
    assert nb.B == c.B and layout_ref.check_block(nb.block) == (layout_ref.OK, layout_ref.NONE)
    for keys, W in c.keysets.values():
        assert fl.desc_ok(c.atts, keys, 0 if W is None else 4, 0 if W is None else W)
    assert all(fl.col_ok(c.atts, col) for col in c.agg_cols) and all(fl.col_ok(c.atts, col, True) for col in c.group_by)


@pytest.mark.parametrize("name", ls.NAMES)
def test_reference_calls_are_quick_and_compose(oracle, name):
    """every reference call a GPU test makes, on the case and on its neighbour, within a few seconds each; a call of three blocks
    put together from the per-block results equals the references' own word on the three (where that is cheap: not on 256
    aliases of 16 MiB); every key set of the case has a match, and the neighbour has matches and misses"""
    c = ls.case(oracle, name)
    nb = ls.neighbour(oracle, c)
    for keyset in ls.CASE_KEYSETS[name]:
        for call in CALLS:
            for x in (c, nb):
                ls.expected(x, keyset, call)
                assert ls.seconds[(x.name, keyset, call)] < SECONDS, (x.name, keyset, call, ls.seconds[(x.name, keyset, call)])
            if name not in ("aliased256", "aliased257"):
                same(ls.call_of([c, nb, c], keyset, call), ls.direct([c, nb, c], keyset, call), (name, keyset, call))
        assert int(ls.expected(c, keyset, "count")[0]["n_match"][0]) > 0, (name, keyset)
        if keyset == "int" or (keyset != "truth" and c.atts is ls.ATTS):     # the generator's neighbour: by its ids
            t = ls.expected(nb, keyset, "count")[0][0]
            assert 0 < int(t["n_match"]) < int(t["n_items"]), (nb.name, keyset)
    for keyset in ls.FILTER_ONLY.get(name, []):                              # OVERLAP under a set key and under a float key too
        for x in (c, nb):
            for call in ("filter", "count"):
                ls.expected(x, keyset, call)
                assert ls.seconds[(x.name, keyset, call)] < SECONDS, (x.name, keyset, call, ls.seconds[(x.name, keyset, call)])
        n = int(name[7:])
        assert tuple(ls.expected(c, keyset, "filter")[0][0])[:4] == (7, n, 0, 0) and ls.expected(c, keyset, "filter")[3] == (0, 0)
        assert tuple(ls.expected(c, keyset, "count")[0][0])[:4] == (0, n, n, 0)
    # a batch behind an OVERLAP block: the neighbour's row starts at 0 and its bytes are the call's first
    if name in ("aliased256", "aliased257"):
        table, recs, packed, total = ls.call_of([c, nb, c], "int", "filter")
        alone = ls.expected(nb, "int", "filter")
        assert table["status"].tolist() == [7, 0, 7] and table["off"].tolist() == [0, 0, total[0]]
        assert table["rec_first"].tolist() == [0, 0, total[1]] and total == alone[3]
        assert packed.tobytes() == alone[2].tobytes() and recs.tobytes() == alone[1].tobytes()


def test_many_copies_expectation(oracle):
    """260 copies of aliased(1): the totals pass 2^32 in block 256"""
    c = ls.case(oracle, "aliased1")
    total = ls.expected(c, "int", "filter")[3]
    assert total == (TWO24, 1) and 255 * total[0] < TWO32 <= 256 * total[0] and 260 * total[0] == 260 * TWO24
