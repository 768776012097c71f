"""GPU tests of the bucketed group columns (CRYO_GROUP_BUCKETS) in cryo_codec_group_batch, cryo_codec_group_blocks and
cryo_multi_group_blocks.

Every row, record and cell is compared, byte for byte, with tests/bucket_ref.py -- the statement of the rules of
include/cryo_codec.h ("Bucketed group columns") in Python integers -- applied to the blocks the ORACLE encoded.  The device
buffers are filled with a sentinel before every call: nothing beyond the rows, the records and the cells of the call may be
written, and the caller's bucket array and lists are read back afterwards: the library only reads them."""
import ctypes as C
import random

import numpy as np
import pytest

import bucket_ref as bk
import group_ref as gr
import scan_calls
import tuple_craft as tc
from bucket_ref import I64_MAX, I64_MIN
from filter_ref import EQ, GE, HEADER, INT2, INT4, INT8, LT, STREAM
from float_ref import BYTES, FLOAT8, IN
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import SENTINEL, Encoder, same_group

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
B = 16384                                               # 290 tuples of 48 bytes and their items fit
ATTS = [(8, 8), (4, 4), (2, 2), (8, 8)]                 # (ts int8, d int4, s int2, x int8)
WIDE = ATTS + [(-1, 4), (8, 8)]                         # ... t text, f float8
TS, D, S, X = (1, INT8), (2, INT4), (3, INT2), (4, INT8)
US_PER_DAY = 86_400_000_000
PG_EPOCH_US = 946_684_800_000_000
DAY = bk.width(0, US_PER_DAY)


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def block(rows, atts=ATTS):
    return tc.build_block(B, [tc.form_tuple(atts, list(r)) for r in rows])


def clip(values):
    return sorted({v for v in values if I64_MIN <= v <= I64_MAX})


# ---- the three call forms ----
def batch(codec, method, comps, atts, keys, by, cols, buckets, cap=None, truth=None, shift=1):
    """cryo_codec_group_batch on device copies of everything, the lists of boundaries at ptr + shift"""
    n, nc = len(comps), len(cols)
    cap = 290 * n if cap is None else cap
    with scan_calls.Device(codec, comps, atts, keys) as d:
        b, g = d.put(cc.group_desc(by)[1]), d.put(cc.agg_desc(cols)[1])
        arr, lists, rebase = cc.bucket_array(buckets)
        d_lists = d.alloc(lists.nbytes + 8)
        d_lists.upload(lists, shift)
        arr = rebase(d_lists.ptr + shift).copy()
        d_bk = d.put(arr)
        rows, recs, cells, total = (d.alloc(32 * n + 64, SENTINEL), d.alloc(24 * cap + 64, SENTINEL),
                                    d.alloc(40 * cap * nc + 64, SENTINEL), d.alloc(8, SENTINEL))
        codec.group_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, len(by), b, nc,
                          g if nc else None, rows, recs, cap, cells if nc else None, total, truth=truth, buckets=d_bk)
        codec.sync()
        d.keys_untouched()
        assert np.array_equal(d_bk.download(arr.nbytes).view(cc.BUCKET), arr), "the caller's bucket array was written"
        assert np.array_equal(d_lists.download(lists.nbytes + shift)[shift:], lists), "the caller's lists were written"
        r, q, c = rows.download(), recs.download(), cells.download()
        tot = int(total.download().view("<u8")[0])
        wrote = min(tot, cap)
        assert (r[32 * n:] == SENTINEL).all() and (q[24 * wrote:] == SENTINEL).all() and (c[40 * wrote * nc:] == SENTINEL).all()
        return (r[:32 * n].view(cc.GROUP_BLOCK).copy(), q[:24 * wrote].view(cc.GROUP_REC).copy(),
                c[:40 * wrote * nc].view(cc.AGG_CELL).reshape(wrote, nc).copy(), tot)


def hosted(codec, method, comps, atts, keys, by, cols, buckets, cap=None, truth=None):
    return codec.group_blocks(method, comps, B, cc.filter_desc(atts, keys, 0, truth), cc.group_desc(by), cc.agg_desc(cols) if cols else None,
                              cap, buckets=buckets)


def multi(devices, method, comps, atts, keys, by, cols, buckets, cap=None):
    return scan_calls.multi_call(devices, lambda L, h, chk: cc.group_blocks_call(
        L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.group_desc(by, buckets),
        cc.agg_desc(cols) if cols else None, cap))


def both(codec, enc, blocks, atts, keys, by, cols, buckets, what, methods=(METHOD_LZ4,), truth=None):
    """device buffers and host buffers against bucket_ref on `blocks`; returns the expectation"""
    want = bk.group_call(blocks, atts, keys, by, cols, buckets, truth)
    for method in methods:
        comps = [enc(method, b) for b in blocks]
        same_group(batch(codec, method, comps, atts, keys, by, cols, buckets, truth=truth), want, (what, method, "device buffers"))
        same_group(hosted(codec, method, comps, atts, keys, by, cols, buckets, truth=truth), want, (what, method, "host buffers"))
    return want


# ---- block shapes ----
def day_rows(m, start=-3 * US_PER_DAY // 2, step=US_PER_DAY // 7):
    """m rows whose ts ascends across day boundaries on both sides of the origin; d the row's number, s of three values"""
    return [(start + p * step, p, p % 3 - 1, 1000 * p) for p in range(m)]


def test_block_shapes(dev, enc):
    """1, 63, 64, 65 and 290 tuples per block -- the turn boundaries and the item maximum --, a block without a tuple, a block
    whose tuples all fail the key, a stream the decoders reject and a bad header, in one call per method"""
    blocks = [block(day_rows(m)) for m in (1, 63, 64, 65, 290)] + [block([]), block([(5, 1, 1, -1)] * 9)]
    header = block(day_rows(3))
    header[0:4] = np.frombuffer((12).to_bytes(4, "little"), np.uint8)      # lower = 12: not 8 + 8 n
    blocks += [header, None, block(day_rows(65, step=US_PER_DAY // 64))]
    keys = [(4, INT8, GE, 0)]
    want = bk.group_call(blocks, ATTS, keys, [TS, S], [X, TS], [DAY, bk.RAW])
    assert want[0]["status"].tolist() == [0] * 7 + [HEADER, STREAM, 0] and want[0]["n_match"].tolist() == [1, 63, 64, 65, 290, 0, 0, 0, 0, 65]
    assert 100 < want[0]["n_groups"][4] < 290 and want[0]["n_groups"][9] == 2 * 3 and not want[0]["n_bad"].any()
    for method in METHODS:
        comps = [enc(method, blocks[0] if b is None else b) for b in blocks]
        comps[8] = comps[8][:len(comps[8]) - 5]
        same_group(batch(dev, method, comps, ATTS, keys, [TS, S], [X, TS], [DAY, bk.RAW]), want, (method, "device buffers"))
        same_group(hosted(dev, method, comps, ATTS, keys, [TS, S], [X, TS], [DAY, bk.RAW]), want, (method, "host buffers"))


# ---- WIDTH ----
WIDTHS = (1, 2, 3, 1 << 32, US_PER_DAY, I64_MAX)
ORIGINS = (0, -1, PG_EPOCH_US, I64_MIN, I64_MAX)


def width_values(o, w):
    """o, o +- 1, exact multiples and multiples +- 1 on both sides of o, the far ends of the type"""
    out = [I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX, 0, -1, 1]
    for k in (-3, -2, -1, 0, 1, 2, 3):
        out += [o + k * w - 1, o + k * w, o + k * w + 1]
    return clip(out)


@pytest.mark.parametrize("o", ORIGINS)
def test_width(dev, enc, o):
    """every width at this origin: the six widths are the six blocks' calls, the values lie around the origin and the multiples"""
    underflows = 0
    for w in WIDTHS:
        values = width_values(o, w)
        rows = [(v, p, p, v) for p, v in enumerate(values)]
        want = both(dev, enc, [block(rows), block(rows[::-1])], ATTS, [], [TS], [X], [bk.width(o, w)], ("width", o, w))
        underflows += int(want[0]["n_bad"][0])
        assert int(want[0]["n_match"][0]) + int(want[0]["n_bad"][0]) == len(values)
        assert int(want[1]["n_rows"].sum()) == int(want[0]["n_match"].sum())                # a block's n_rows sum to its n_match
    if o == I64_MAX:
        assert underflows > 0                                             # keys below INT64_MIN: counted in n_bad, in no group
    if o == I64_MIN:
        assert underflows == 0                                            # nothing lies below this origin


def test_width_needs_64_unsigned_bits(dev, enc):
    rows = [(I64_MAX, 0, 0, 1), (I64_MAX - 1, 0, 0, 2), (I64_MIN, 0, 0, 3), (-1, 0, 0, 4), (0, 0, 0, 5)]
    _, recs, _, _ = both(dev, enc, [block(rows)], ATTS, [], [TS], [X], [bk.width(I64_MIN, I64_MAX)], "the whole range", METHODS)
    assert recs["key"][:, 0].tolist() == [I64_MIN, -1, I64_MAX - 1] and recs["n_rows"].tolist() == [1, 2, 2]


def test_width_on_narrow_columns(dev, enc):
    """int2 and int4 group columns with negative values: sign-extended before the bucket; the key is not clamped to the type"""
    rows = [(0, d, s, d) for d, s in zip([-(1 << 31), -(1 << 31) + 1, -86401, -86400, -1, 0, 1, 86399, 86400, (1 << 31) - 1] * 2,
                                         [-(1 << 15), -(1 << 15) + 1, -8, -7, -1, 0, 1, 6, 7, (1 << 15) - 1] * 2)]
    both(dev, enc, [block(rows)], ATTS, [], [D, S], [X], [bk.width(0, 86400), bk.width(0, 7)], "day of an int4, week of an int2", METHODS)
    _, recs, _, _ = both(dev, enc, [block(rows)], ATTS, [], [S, D], [], [bk.width(5, 1 << 40), bk.width(-3, 1 << 33)], "wider than the type")
    assert set(recs["key"][:, 0].tolist()) == {5 - (1 << 40), 5} and set(recs["key"][:, 1].tolist()) == {-3 - (1 << 33), -3}


# ---- BOUNDS ----
def bound_list(n, rnd, duplicates):
    """n entries, unsorted, spread over the whole range; duplicates: a quarter of them repeat others"""
    distinct = set()
    while len(distinct) < (max(1, n - n // 4) if duplicates else n):
        distinct.add(rnd.randrange(I64_MIN + 2000, I64_MAX - 1))
    distinct = sorted(distinct)
    out = distinct + [distinct[(5 * i) % len(distinct)] for i in range(n - len(distinct))]
    rnd.shuffle(out)
    assert len(out) == n
    return out


@pytest.mark.parametrize("duplicates", [False, True])
@pytest.mark.parametrize("n", [1, 8, 9, 1024])
def test_bounds(dev, enc, n, duplicates):
    """a list of n boundaries given unsorted, all distinct or with duplicates, scanned (up to 8 distinct) or searched: values
    equal to a boundary, one below and one above it, below the smallest (undecided), at and above the largest"""
    rnd = random.Random(n)
    members = bound_list(n, rnd, duplicates)
    distinct = sorted(set(members))
    probe = distinct if n <= 9 else [distinct[i] for i in (0, 1, 2, 255, 256, 257, 383, 384, 385, 511, 512, 513, len(distinct) - 2, len(distinct) - 1)]
    values = clip([v + d for v in probe for d in (-1, 0, 1)] + [I64_MIN, I64_MAX, distinct[0] - 1000])
    rows = [(v, p, p, v) for p, v in enumerate(values)]
    want = both(dev, enc, [block(rows), block(rows[::-1])], ATTS, [], [TS], [X, TS], [bk.bounds(members)], ("bounds", n), METHODS)
    below = sum(v < distinct[0] for v in values)
    assert below >= 3 and want[0]["n_bad"].tolist() == [below, below]
    assert set(want[1]["key"][:, 0].tolist()) <= set(distinct) and want[1]["key"][-1, 0] == distinct[-1]


def test_bounds_with_int64_min_catch_everything(dev, enc):
    rows = [(v, 0, 0, 1) for v in (I64_MIN, I64_MIN + 1, -1, 0, 99, 100, 101, I64_MAX)]
    rows_, recs, _, _ = both(dev, enc, [block(rows)], ATTS, [], [TS], [X], [bk.bounds([100, I64_MIN, 100, 0])], "catch-all")
    assert rows_["n_bad"][0] == 0 and recs["key"][:, 0].tolist() == [I64_MIN, 0, 100] and recs["n_rows"].tolist() == [3, 2, 3]
    # the same column twice: nine boundaries searched beside eight scanned
    nine = list(range(-40, 50, 10))
    both(dev, enc, [block([(v, 0, 0, v) for v in range(-45, 50)])], ATTS, [], [TS, TS], [X], [bk.bounds(nine), bk.bounds(nine[1:])], "9 and 8")


# ---- INFINITE ----
def test_infinite(dev, enc):
    """with both kinds on an int4 and an int8 column that hold the type's extremes; a finite value whose key is an extreme is
    undecided; the same data without the flag"""
    i4lo, i4hi = -(1 << 31), (1 << 31) - 1
    rows = [(I64_MIN, i4lo, 0, 1), (I64_MAX, i4hi, 0, 2), (I64_MIN + 3, i4lo + 3, 0, 3), (I64_MAX - 1, i4hi - 1, 0, 4), (7, 7, 0, 5),
            (I64_MIN, 0, 0, 6), (0, i4hi, 0, 7), (-8, -8, 0, 8)]
    blocks = [block(rows)]
    for flag in (bk.INFINITE, 0):
        w = both(dev, enc, blocks, ATTS, [], [TS, D], [X], [bk.width(I64_MIN, 5, flag), bk.width(i4lo, 5, flag)], ("width", flag), METHODS)
        b = both(dev, enc, blocks, ATTS, [], [TS, D], [X], [bk.bounds([I64_MIN, 0, I64_MAX], flag), bk.bounds([i4hi, 0, i4lo], flag)],
                 ("bounds", flag))
        # row 3's keys are the minima: undecided under the flag; so is row 8 among the lists (its keys are the first boundaries)
        assert (w[0]["n_bad"][0], b[0]["n_bad"][0]) == ((1, 2) if flag else (0, 0))
        assert (I64_MAX, i4hi) in [tuple(k) for k in w[1]["key"].tolist()]                    # +infinity is its own bucket
    # the int4 column under an int8-wide width: its extremes stay, by the column's type
    both(dev, enc, blocks, ATTS, [], [D], [], [bk.width(0, 1 << 40, bk.INFINITE)], "the column's type decides")


# ---- two group columns, NULLs, roles ----
def test_two_columns_and_nulls(dev, enc):
    rnd = random.Random(4)
    rows = []
    for p in range(200):
        ts = rnd.randrange(-2 * US_PER_DAY, 3 * US_PER_DAY)
        rows.append((None if p % 11 == 0 else ts, None if p % 13 == 0 else p % 50 - 25, p % 3, None if p % 17 == 0 else ts))
    rows += [(5,), ()]                                                    # natts 1 and 0: the columns beyond are NULL
    blocks = [block(rows)]
    hour = bk.width(0, US_PER_DAY // 24)
    both(dev, enc, blocks, ATTS, [], [TS, D], [X], [DAY, bk.RAW], "bucket + raw", METHODS)
    both(dev, enc, blocks, ATTS, [], [D, TS], [X], [bk.RAW, DAY], "raw + bucket")
    both(dev, enc, blocks, ATTS, [], [TS, D], [X], [DAY, bk.width(-25, 10)], "bucket + bucket", METHODS)
    w = both(dev, enc, blocks, ATTS, [], [TS, TS], [X], [DAY, hour], "the same column twice: day and hour")
    assert ((w[1]["nulls"] == 0) | (w[1]["nulls"] == 3)).all() and (w[1]["key"][:, 0] <= w[1]["key"][:, 1]).all()
    assert 3 in w[1]["nulls"].tolist()                                    # the NULL group, after every value
    # a bucketed column that is also a raw aggregate column and a key: min(ts), max(ts) per day of a range
    keys = [(1, INT8, GE, -US_PER_DAY), (1, INT8, LT, 2 * US_PER_DAY)]
    w = both(dev, enc, blocks, ATTS, keys, [TS], [TS, X], [DAY], "group, aggregate and key column", METHODS)
    assert w[1]["key"][:, 0].tolist() == [-US_PER_DAY, 0, US_PER_DAY]
    assert (w[2]["min"][:, 0] >= w[1]["key"][:, 0]).all() and (w[2]["max"][:, 0] < w[1]["key"][:, 0] + US_PER_DAY).all()
    # undecided in either column
    w = both(dev, enc, blocks, ATTS, [], [TS, D], [X], [bk.bounds([0]), bk.bounds([0, -10])], "undecided in either column")
    assert w[0]["n_bad"][0] > 50 and int(w[1]["n_rows"].sum()) == int(w[0]["n_match"][0])


# ---- beside the other kinds of key and a float aggregate column ----
def wide_block():
    rnd = random.Random(6)
    texts = [b"alpha", b"beta", b"", b"gamma" * 9]
    rows = []
    for p in range(120):
        f = np.float64(rnd.uniform(-1e6, 1e6)).view(np.int64)
        rows.append((rnd.randrange(-US_PER_DAY, 2 * US_PER_DAY), p % 9, p % 4, p, texts[p % 4], None if p % 10 == 0 else int(f)))
    return block(rows, WIDE)


def test_beside_other_features(dev, enc):
    blocks = [wide_block()]
    by, bks = [TS, S], [DAY, bk.RAW]
    both(dev, enc, blocks, WIDE, [(5, BYTES, EQ, b"alpha")], by, [X], bks, "a byte-string key", METHODS)
    both(dev, enc, blocks, WIDE, [(2, INT4, IN, [1, 3, 5, 7, 8, 100])], by, [X], bks, "a set key")
    both(dev, enc, blocks, WIDE, [(2, INT4, IN, list(range(-5, 6)))], by, [X], [bk.bounds(range(-100, 100), 0), bk.RAW], "a searched set key")
    keys = [(1, INT8, LT, 0), (3, INT2, EQ, 2), (5, BYTES, GE, b"b")]
    both(dev, enc, blocks, WIDE, keys, by, [X], bks, "a truth table", METHODS, truth=cc.truth_dnf([1, 6], 3))
    w = both(dev, enc, blocks, WIDE, [], by, [(6, FLOAT8), X], bks, "a float8 aggregate column", METHODS)
    assert w[2]["n"][:, 0].sum() == 108                                   # the float kernel: the NULLs add nothing
    both(dev, enc, blocks, WIDE, [(6, FLOAT8, GE, 0.0)], by, [(6, FLOAT8)], [bk.bounds([0, -US_PER_DAY, US_PER_DAY]), bk.RAW], "a float key")


# ---- every bucket NONE ----
def test_all_none_is_the_plain_call(dev, enc):
    blocks = [block(day_rows(65)), block(day_rows(290)), None]
    keys = [(4, INT8, GE, 3000)]
    for method in METHODS:
        comps = [enc(method, blocks[0] if b is None else b) for b in blocks]
        comps[2] = comps[2][:20]
        for by, cols in (([TS], [X]), ([S, D], []), ([D, TS], [X, (2, INT4), (3, INT2), (1, INT8)])):
            plain = dev.group_blocks(method, comps, B, cc.filter_desc(ATTS, keys), cc.group_desc(by), cc.agg_desc(cols) if cols else None)
            for got in (hosted(dev, method, comps, ATTS, keys, by, cols, [bk.RAW] * len(by)),
                        batch(dev, method, comps, ATTS, keys, by, cols, [bk.RAW] * len(by))):
                assert got[3] == plain[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], plain[:3])), (method, by)
            same_group(plain, gr.group_call(blocks, ATTS, keys, by, cols), (method, by))


# ---- cut-off, chunks, stale copies ----
def test_group_cap(dev, enc):
    blocks = [block(day_rows(65)), block(day_rows(290)), block(day_rows(64))]
    want = bk.group_call(blocks, ATTS, [], [TS], [X], [DAY])
    need = want[3]
    assert want[0]["n_groups"].tolist() == [10, 42, 10] and need == 62
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    same_group(hosted(dev, METHOD_LZ4, comps, ATTS, [], [TS], [X], [DAY], need), want, "exactly the need")
    for cap in (need - 1, 12, 0):
        with pytest.raises(CryoError) as e:
            hosted(dev, METHOD_LZ4, comps, ATTS, [], [TS], [X], [DAY], cap)
        assert e.value.code == cc.E_DSTSIZE, cap
        rows, recs, cells, total = batch(dev, METHOD_LZ4, comps, ATTS, [], [TS], [X], [DAY], cap)
        assert total == need and recs.shape[0] == cap                      # *total in full; the sentinel from group_cap on (batch)
        same_group((rows, recs, cells, need), (want[0], want[1][:cap], want[2][:cap], need), ("cut at", cap))


def test_chunks(dev, enc):
    """40 blocks of 16 KiB under a budget that holds a few of them: the bucket table serves every chunk of the call"""
    rnd = random.Random(8)
    months = [k * 30 * US_PER_DAY for k in range(-3, 4)]
    blocks = [block([(rnd.randrange(-100 * US_PER_DAY, 100 * US_PER_DAY), p, k % 5, p) for p in range(40 + k)]) for k in range(40)]
    want = bk.group_call(blocks, ATTS, [], [TS, S], [X], [bk.bounds(months), bk.RAW])
    assert want[0]["n_bad"].sum() > 0
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        whole = batch(dev, method, comps, ATTS, [], [TS, S], [X], [bk.bounds(months), bk.RAW])
        same_group(whole, want, (method, "one chunk"))
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 1 << 20)
        same_group(batch(dev, method, comps, ATTS, [], [TS, S], [X], [bk.bounds(months), bk.RAW]), want, (method, "small budget"))
        same_group(hosted(dev, method, comps, ATTS, [], [TS, S], [X], [bk.bounds(months), bk.RAW]), want, (method, "host, small budget"))
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


def test_consecutive_calls_with_different_lists(dev, enc):
    """two calls on one handle whose lists differ in length and content, then a width: a stale device copy would show"""
    blocks = [block([(v, 0, 0, v) for v in range(-60, 60)])]
    for buckets in ([bk.bounds(range(-50, 50, 10))], [bk.bounds([-60, 7])], [bk.bounds(range(-64, 64))], [bk.width(1, 9)], [bk.bounds([0, -60])]):
        both(dev, enc, blocks, ATTS, [], [TS], [X], buckets, buckets)


# ---- the call forms agree ----
@pytest.mark.parametrize("devices", [(0,), (0, 0)])
def test_call_forms_agree(dev, enc, devices):
    """group_batch, group_blocks and cryo_multi_group_blocks -- one handle, and two handles on one GPU, each of which stages its
    own table -- byte for byte"""
    rnd = random.Random(9)
    blocks = [block([(rnd.randrange(-9 * US_PER_DAY, 9 * US_PER_DAY), p % 7, p % 2, p) for p in range(30 + 20 * k)]) for k in range(7)]
    buckets = [bk.bounds([k * US_PER_DAY for k in range(-8, 9, 2)]), bk.width(1, 3)]
    want = bk.group_call(blocks, ATTS, [], [TS, D], [X, TS], buckets)
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        one = hosted(dev, method, comps, ATTS, [], [TS, D], [X, TS], buckets)
        same_group(one, want, (method, "host buffers"))
        for got in (batch(dev, method, comps, ATTS, [], [TS, D], [X, TS], buckets), multi(devices, method, comps, ATTS, [], [TS, D], [X, TS], buckets)):
            assert got[3] == one[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], one[:3])), (method, devices)


# ---- refusals ----
REFUSED = [
    ("an unknown kind", [(3, 0, 0, 0)]), ("kind 255", [(255, 0, 0, 0)]),
    ("width 0", [bk.width(0, 0)]), ("a negative width", [bk.width(0, -86400)]), ("a width with n", [(bk.WIDTH, 0, 0, 5)], ("n", 0, 1)),
    ("no boundary", [bk.bounds([])]), ("1 025 boundaries", [bk.bounds(range(1025))]), ("a null list", [bk.bounds([1])], ("value", 0, 0)),
    ("a list with an origin", [(bk.BOUNDS, 0, 7, [1])]),
    ("NONE with a flag", [(bk.NONE, bk.INFINITE, 0, 0)]), ("NONE with an origin", [(bk.NONE, 0, 1, 0)]), ("NONE with a value", [(bk.NONE, 0, 0, 1)]),
    ("NONE with n", [bk.RAW], ("n", 0, 1)),
    ("an unknown flag", [bk.width(0, 1, 2)]), ("an unknown flag beside the known", [bk.bounds([1], 3)]),
    ("a bucket's reserved field", [bk.width(0, 1)], ("rsv", 0, 1)),
    ("a bad bucket behind a good one", [bk.width(0, 1), bk.width(0, 0)]),
]


def test_refusals(dev, enc):
    """every CRYO_E_ARG rule of the bucket array, on host arrays (refused before a device is touched: the transfer counters
    stand still) and on device arrays; and the rules of the struct: rsv, a null and a misaligned buckets pointer"""
    comps = [enc(METHOD_LZ4, block(day_rows(5)))]
    arr = np.ascontiguousarray(comps[0])
    src, szs = (C.c_void_p * 1)(arr.ctypes.data), (C.c_uint32 * 1)(arr.nbytes)
    rows, recs, cells, total = np.zeros(1, cc.GROUP_BLOCK), np.zeros(290, cc.GROUP_REC), np.zeros(290, cc.AGG_CELL), C.c_uint64()
    f = cc.filter_desc(ATTS, [])
    a = cc.agg_desc([X])

    def host_rc(g):
        before = dev.transfer_counters()
        rc = dev.L.cryo_codec_group_blocks(dev.h, METHOD_LZ4, src, szs, 1, B, C.byref(f[0]), C.byref(g), C.byref(a[0]), rows.ctypes.data,
                                           recs.ctypes.data, 290, cells.ctypes.data, C.byref(total))
        if rc != cc.OK:
            assert dev.transfer_counters() == before
        return rc

    with scan_calls.Device(dev, comps, ATTS, []) as d:
        d_cols = d.put(a[1])
        d_rows, d_recs, d_cells, d_total = d.alloc(32), d.alloc(24 * 290), d.alloc(40 * 290), d.alloc(8)
        d_lists = d.alloc(8 * 1025 + 8)

        def device_rc(by_arr, bucket_arr, rsv=cc.GROUP_BUCKETS, ptr=None):
            d_by, d_bk = d.put(by_arr), d.put(bucket_arr)
            fd = cc.CryoFilter(len(ATTS), 0, 0, 0, d.atts.ptr, None)
            g = cc.CryoGroupB(len(by_arr), rsv, d_by.ptr, d_bk.ptr if ptr is None else ptr(d_bk.ptr))
            ad = cc.CryoAgg(1, 0, d_cols.ptr)
            rc = dev.L.cryo_codec_group_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(fd), C.byref(g), C.byref(ad),
                                              d_rows.ptr, d_recs.ptr, 290, d_cells.ptr, d_total.ptr)
            dev.sync()
            return rc

        for name, buckets, *patch in REFUSED:
            by = [TS, D][:len(buckets)]
            assert not bk.buckets_ok(buckets, len(by), rsv=[1] if patch and patch[0][0] == "rsv" else None) or patch, name
            g, by_arr = cc.group_desc(by, buckets)
            for field, index, value in patch:
                g.bucket_arr[field][index] = value
            assert host_rc(g) == cc.E_ARG, (name, "host arrays")
            arr_d, _, rebase = cc.bucket_array(buckets)
            arr_d = rebase(d_lists.ptr).copy()
            for field, index, value in patch:
                arr_d[field][index] = value
            assert device_rc(by_arr, arr_d) == cc.E_ARG, (name, "device arrays")
        # the struct's own rules
        good, by_arr = cc.group_desc([TS], [DAY])
        assert host_rc(good) == cc.OK and total.value == 2
        assert device_rc(by_arr, good.bucket_arr) == cc.OK
        for rsv in (2, 3, 0x80000001, 0xFFFFFFFF):
            g, _ = cc.group_desc([TS], [DAY])
            g.rsv = rsv
            assert host_rc(g) == cc.E_ARG, rsv
            assert device_rc(by_arr, good.bucket_arr, rsv=rsv) == cc.E_ARG, rsv
        g, _ = cc.group_desc([TS], [DAY])
        g.buckets = None
        assert host_rc(g) == cc.E_ARG and device_rc(by_arr, good.bucket_arr, ptr=lambda p: None) == cc.E_ARG
        shifted = np.zeros(32, np.uint8)
        at = shifted.ctypes.data + (-shifted.ctypes.data) % 8 + 4
        C.memmove(at, good.bucket_arr.ctypes.data, 24)
        g, _ = cc.group_desc([TS], [DAY])
        g.buckets = at
        assert host_rc(g) == cc.E_ARG and device_rc(by_arr, good.bucket_arr, ptr=lambda p: p + 4) == cc.E_ARG
        # rsv == 0: the struct is a cryo_group, and what lies behind it is not looked at
        g, _ = cc.group_desc([TS], [(9, 9, 9, 9)])
        g.rsv = 0
        assert host_rc(g) == cc.OK and total.value == 5
