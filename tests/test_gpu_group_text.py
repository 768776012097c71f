"""GPU tests of the text group columns (CRYO_GROUP_TEXT) in cryo_codec_group_batch, cryo_codec_group_blocks and
cryo_multi_group_blocks.

Every row, record, cell and key cell is compared, byte for byte, with tests/group_text_ref.py -- the statement of the rules of
include/cryo_codec.h ("Text group columns") in plain Python -- applied to the blocks the ORACLE encoded.  The device buffers are
filled with a sentinel before every call: nothing beyond the rows, the records and the cells of the call may be written."""
import ctypes as C
import random

import numpy as np
import pytest

import group_text_cases as gc
import group_text_ref as gt
import scan_calls
import tuple_craft as tc
from filter_ref import EQ, GE, HEADER, INT4, INT8, LT, STREAM
from float_ref import FLOAT8
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import SENTINEL, Encoder, same_fields
from test_group_text_cpu import RULES
from tuple_craft import Long, Toast

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
B = 16384                                               # 290 tuples of 48 bytes and their items fit
ATTS = gc.ATTS                                          # (id int4, t text, x int8, u text, d int4, f float8)
T_, X, U, D, F = gc.T_, gc.X, gc.U, gc.D, (6, FLOAT8)
BYTES = gt.BYTES


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def block(rows, size=B):
    return tc.build_block(size, [tc.form_tuple(ATTS, list(r)) for r in rows])


def ntext(by):
    return sum(1 for _, typ in by if typ == BYTES)


# ---- the three call forms ----
def batch(codec, method, comps, keys, by, cols, cap=None, truth=None, size=B, text=True):
    """cryo_codec_group_batch on device copies of everything; text False: the descriptor's rsv is 0"""
    n, nc = len(comps), len(cols)
    nt = ntext(by) if text else 0
    cpg = nc + nt
    cap = 290 * n if cap is None else cap
    with scan_calls.Device(codec, comps, ATTS, keys) as d:
        b, g = d.put(cc.group_desc(by)[1]), d.put(cc.agg_desc(cols)[1])
        rows, recs, cells, total = (d.alloc(32 * n + 64, SENTINEL), d.alloc(24 * cap + 64, SENTINEL),
                                    d.alloc(40 * cap * cpg + 64, SENTINEL), d.alloc(8, SENTINEL))
        codec.group_batch(method, d.src, d.off, d.sz, size, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, len(by), b, nc,
                          g if nc else None, rows, recs, cap, cells if cpg else None, total, truth=truth, text=text)
        codec.sync()
        d.keys_untouched()
        r, q, c = rows.download(), recs.download(), cells.download()
        tot = int(total.download().view("<u8")[0])
        wrote = min(tot, cap)
        assert (r[32 * n:] == SENTINEL).all() and (q[24 * wrote:] == SENTINEL).all() and (c[40 * wrote * cpg:] == SENTINEL).all()
        agg, key = cc.group_cells_split(c[:40 * wrote * cpg].reshape(wrote, cpg * 40), nc, nt)
        return r[:32 * n].view(cc.GROUP_BLOCK).copy(), q[:24 * wrote].view(cc.GROUP_REC).copy(), agg, tot, key


def hosted(codec, method, comps, keys, by, cols, cap=None, truth=None, size=B):
    return codec.group_blocks(method, comps, size, cc.filter_desc(ATTS, keys, 0, truth), cc.group_desc(by, text=True),
                              cc.agg_desc(cols) if cols else None, cap)


def multi(devices, method, comps, keys, by, cols, cap=None, truth=None, size=B):
    return scan_calls.multi_call(devices, lambda L, h, chk: cc.group_blocks_call(
        L.cryo_multi_group_blocks, h, chk, method, comps, size, cc.filter_desc(ATTS, keys, 0, truth), cc.group_desc(by, text=True),
        cc.agg_desc(cols) if cols else None, cap))


def all_devices():
    return tuple(range(cc.device_count())) if cc.device_count() > 1 else (0, 0)


def same_text(got, want, what=""):
    assert len(got) == 5 and got[3] == want[3], (what, got[3], want[3])
    for j in (0, 1, 2, 4):
        same_fields(got[j], want[j], (what, j))


def three(codec, enc, blocks, keys, by, cols, what, methods=METHODS, truth=None, size=B, populated=False):
    """device buffers, host buffers and the multi-handle call against group_text_ref on `blocks`; returns the expectation.
    populated: the reference alone finds matches and groups in every block"""
    want = gt.group_call(blocks, ATTS, keys, by, cols, truth)
    if populated:
        assert (want[0]["n_match"] > 0).all() and (want[0]["n_groups"] > 0).all(), what
    for method in methods:
        comps = [enc(method, b) for b in blocks]
        same_text(batch(codec, method, comps, keys, by, cols, truth=truth, size=size), want, (what, method, "device buffers"))
        same_text(hosted(codec, method, comps, keys, by, cols, truth=truth, size=size), want, (what, method, "host buffers"))
        same_text(multi(all_devices(), method, comps, keys, by, cols, truth=truth, size=size), want, (what, method, "multi"))
    return want


# ---- the hand-made blocks ----
CASES = gc.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made_blocks(dev, enc, case):
    name, blk, keys, by, cols, groups, n_bad = case
    want = three(dev, enc, [blk], keys, by, cols, name, size=gc.B)
    assert gt.groups_of(want, by, 0) == groups and int(want[0]["n_bad"][0]) == n_bad


def test_hand_made_blocks_in_one_call(dev, enc):
    """every hand-made block under one descriptor of two text columns, a multi-handle share per block"""
    blocks = [c[1] for c in CASES]
    want = three(dev, enc, blocks, [], [T_, U], [X, D], "all cases", size=gc.B, populated=True)
    assert want[0]["n_bad"].sum() > 0


# ---- block shapes ----
def key3(i):
    return bytes([107, i % 251, i // 251])


def shape_rows(m, distinct):
    return [(p, key3(p) if distinct else b"one", 1000 * p - 7) for p in range(m)]


@pytest.mark.parametrize("distinct", [False, True], ids=["all keys equal", "all keys distinct"])
def test_block_shapes(dev, enc, distinct):
    """0, 1, 63, 64, 65 and 290 matches per block -- the turn boundaries and the item maximum --, a block whose tuples all fail
    the key, a stream the decoders reject and a bad header, in one call per method and form"""
    blocks = [block(shape_rows(m, distinct)) for m in (0, 1, 63, 64, 65, 290)] + [block([(5, b"x", -100)] * 9)]
    header = block(shape_rows(3, distinct))
    header[0:4] = np.frombuffer((12).to_bytes(4, "little"), np.uint8)      # lower = 12: not 8 + 8 n
    blocks += [header, None]
    keys = [(3, INT8, GE, -7)]
    want = gt.group_call(blocks, ATTS, keys, [T_], [X])
    assert want[0]["status"].tolist() == [0] * 7 + [HEADER, STREAM] and want[0]["n_match"].tolist() == [0, 1, 63, 64, 65, 290, 0, 0, 0]
    assert want[0]["n_groups"].tolist() == ([0, 1, 63, 64, 65, 290, 0, 0, 0] if distinct else [0, 1, 1, 1, 1, 1, 0, 0, 0])
    for method in METHODS:
        comps = [enc(method, blocks[1] if b is None else b) for b in blocks]
        comps[8] = comps[8][:len(comps[8]) - 5]
        same_text(batch(dev, method, comps, keys, [T_], [X]), want, (method, "device buffers"))
        same_text(hosted(dev, method, comps, keys, [T_], [X]), want, (method, "host buffers"))
        same_text(multi(all_devices(), method, comps, keys, [T_], [X]), want, (method, "multi"))


# ---- a random case ----
def random_blocks(seed, nblocks, per_block, grow=7):
    """tuples over all six columns: t and u from pools of values of every length 0 .. 32, one in eight NULL; one t in ten is
    made undecided -- a pointer, or 33 .. 40 bytes under either header"""
    rnd = random.Random(seed)
    pool = [bytes(rnd.randrange(256) for _ in range(n)) for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 32)]
    pool += [pool[9][:-1] + b"\x00", pool[12][:31] + bytes([pool[12][31] ^ 0x80])]
    upool = [b"", b"de", b"fr", b"de\x00", b"\xc3\xa9t\xc3\xa9"]
    blocks = []
    for k in range(nblocks):
        rows = []
        for p in range(per_block + grow * k):
            t = rnd.choice(pool)
            if rnd.random() < 0.5:
                t = Long(t)
            if p % 10 == 3:
                t = rnd.choice([Toast(), b"q" * rnd.randrange(33, 41), Long(b"q" * rnd.randrange(33, 41))])
            elif rnd.random() < 0.125:
                t = None
            f = int(np.float64(rnd.uniform(-1e6, 1e6)).view(np.int64))
            rows.append((p, t, rnd.randrange(-1 << 40, 1 << 40), rnd.choice(upool + [None]), rnd.randrange(4), None if p % 10 == 0 else f))
        blocks.append(block(rows))
    return blocks


@pytest.fixture(scope="module")
def rblocks():
    return random_blocks(20, 5, 60)


def test_random(dev, enc, rblocks):
    want = three(dev, enc, rblocks, [], [T_], [X], "one text column", populated=True)
    assert (want[0]["n_bad"] == (want[0]["n_items"] + 6) // 10).all()       # the one in ten, and nothing else
    three(dev, enc, rblocks, [(5, INT4, LT, 3)], [T_, U], [X, D], "two text columns", populated=True)
    three(dev, enc, rblocks, [], [D, T_], [], "int, then text, no cell", (METHOD_LZ4,), populated=True)
    three(dev, enc, rblocks, [], [U, D], [X, D, X, D], "text, then int, four cells", (METHOD_LZ4,), populated=True)


def test_beside_other_features(dev, enc, rblocks):
    w = three(dev, enc, rblocks, [], [T_], [F, X], "a float8 aggregate column", populated=True)
    assert 0 < w[2]["n"][:, 0].sum() < w[2]["n"][:, 1].sum()               # the float kernel: the NULLs add nothing
    three(dev, enc, rblocks, [(6, FLOAT8, GE, 0.0)], [T_, D], [F], "a float key", (METHOD_LZ4,), populated=True)
    three(dev, enc, rblocks, [(2, BYTES, GE, b"\x40")], [T_], [X], "a byte-string key on the group column", populated=True)
    three(dev, enc, rblocks, [(2, BYTES, EQ, b"")], [T_, U], [X], "the key picks one value", (METHOD_LZ4,), populated=True)
    keys = [(5, INT4, LT, 2), (2, BYTES, GE, b"\x80"), (3, INT8, GE, 0)]
    three(dev, enc, rblocks, keys, [T_], [X], "a truth table", truth=cc.truth_dnf([1, 6], 3), populated=True)


# ---- integer columns under the flag ----
def test_integer_columns_are_the_plain_call(dev, enc, rblocks):
    keys = [(3, INT8, GE, 0)]
    for method in METHODS:
        comps = [enc(method, b) for b in rblocks]
        for by, cols in (([D], [X]), ([D, X], []), ([X, D], [X, D, F])):
            plain = dev.group_blocks(method, comps, B, cc.filter_desc(ATTS, keys), cc.group_desc(by), cc.agg_desc(cols) if cols else None)
            assert plain[3] > 0
            for got in (hosted(dev, method, comps, keys, by, cols), batch(dev, method, comps, keys, by, cols),
                        multi(all_devices(), method, comps, keys, by, cols)):
                assert got[3] == plain[3] and all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], plain[:3])), (method, by)
                assert got[4].shape == (plain[3], 0)
            zero = batch(dev, method, comps, keys, by, cols, text=False)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(zero[:3], plain[:3]))


# ---- cut-off and chunks ----
def test_group_cap(dev, enc, rblocks):
    by, cols = [T_, D], [X]
    want = gt.group_call(rblocks, ATTS, [], by, cols)
    need = want[3]
    first = int(want[0]["first_group"][2])
    assert int(want[0]["n_groups"][2]) > 4
    comps = [enc(METHOD_LZ4, b) for b in rblocks]
    same_text(hosted(dev, METHOD_LZ4, comps, [], by, cols, need), want, "exactly the need")
    for cap in (need - 1, first + 3, first, 0):                            # inside the last block, inside block 2, at its start
        with pytest.raises(CryoError) as e:
            hosted(dev, METHOD_LZ4, comps, [], by, cols, cap)
        assert e.value.code == cc.E_DSTSIZE, cap
        rows, recs, cells, total, key = batch(dev, METHOD_LZ4, comps, [], by, cols, cap)
        assert total == need and recs.shape[0] == cap                      # *total in full; the sentinel from group_cap on (batch)
        same_text((rows, recs, cells, need, key), (want[0], want[1][:cap], want[2][:cap], need, want[4][:cap]), ("cut at", cap))


def test_chunks(dev, enc):
    """48 blocks of 16 KiB under a budget of 1 MiB: a block takes its 16 KiB decoded and 290 * (24 + 40 * 4) bytes of side area,
    so a chunk holds fewer than 16 384 / (16 + 52) = 15 of them and the call has more than three chunks"""
    blocks = random_blocks(21, 48, 20, 1)
    by, cols = [T_, U], [X, D]
    want = gt.group_call(blocks, ATTS, [], by, cols)
    assert (want[0]["n_match"] > 0).all() and (want[0]["n_groups"] > 0).all() and want[0]["n_bad"].sum() > 0
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        same_text(batch(dev, method, comps, [], by, cols), want, (method, "one chunk"))
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 1 << 20)
        same_text(batch(dev, method, comps, [], by, cols), want, (method, "small budget"))
        same_text(hosted(dev, method, comps, [], by, cols), want, (method, "host, small budget"))
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- refusals ----
def test_refusals(dev, enc, rblocks):
    """every rule of the contract that refuses a descriptor, on host arrays (refused before a device is touched: the transfer
    counters stand still) and on device arrays; the descriptors it allows are accepted"""
    comps = [enc(METHOD_LZ4, rblocks[0])]
    arr = np.ascontiguousarray(comps[0])
    src, szs = (C.c_void_p * 1)(arr.ctypes.data), (C.c_uint32 * 1)(arr.nbytes)
    rows, recs, cells, total = np.zeros(1, cc.GROUP_BLOCK), np.zeros(290, cc.GROUP_REC), np.zeros(290 * 6, cc.AGG_CELL), C.c_uint64()
    f = cc.filter_desc(ATTS, [])

    def host_rc(g, a, cells_ptr=cells.ctypes.data):
        before = dev.transfer_counters()
        rc = dev.L.cryo_codec_group_blocks(dev.h, METHOD_LZ4, src, szs, 1, B, C.byref(f[0]), C.byref(g), C.byref(a) if a else None,
                                           rows.ctypes.data, recs.ctypes.data, 290, cells_ptr, C.byref(total))
        if rc != cc.OK:
            assert dev.transfer_counters() == before
        return rc

    with scan_calls.Device(dev, comps, ATTS, []) as d:
        d_rows, d_recs, d_cells, d_total = d.alloc(32), d.alloc(24 * 290), d.alloc(40 * 290 * 6), d.alloc(8)

        def device_rc(by_arr, nby, rsv, col_arr, ncols, cells_ptr=d_cells.ptr):
            d_by = d.put(by_arr)
            d_cols = d.put(col_arr) if ncols else None
            fd = cc.CryoFilter(len(ATTS), 0, 0, 0, d.atts.ptr, None)
            g = cc.CryoGroup(nby, rsv, d_by.ptr)
            ad = cc.CryoAgg(ncols, 0, d_cols.ptr if d_cols else None)
            rc = dev.L.cryo_codec_group_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(fd), C.byref(g), C.byref(ad),
                                              d_rows.ptr, d_recs.ptr, 290, cells_ptr, d_total.ptr)
            dev.sync()
            return rc

        for name, by, cols, rsv, ok in RULES:
            assert gt.desc_ok(ATTS, [], by, cols, rsv) == ok, name
            expect = cc.OK if ok else cc.E_ARG
            g, by_arr = cc.group_desc(by)
            g.rsv = rsv
            a = cc.agg_desc(cols) if cols is not None else None
            assert host_rc(g, a[0] if a else None) == expect, (name, "host arrays")
            col_arr = a[1] if a else np.zeros(1, cc.AGG_COL)
            assert device_rc(by_arr, len(by), rsv, col_arr, len(cols or ())) == expect, (name, "device arrays")
        # a group column's reserved fields
        for field in ("rsv", "rsv2"):
            g, by_arr = cc.group_desc([T_], text=True)
            by_arr[field][0] = 1
            a = cc.agg_desc([X])
            assert host_rc(g, a[0]) == cc.E_ARG and device_rc(by_arr, 1, cc.GROUP_TEXT, a[1], 1) == cc.E_ARG, field
        # the key cells need the cells array although there is no aggregate column
        g, by_arr = cc.group_desc([T_], text=True)
        assert host_rc(g, None, None) == cc.E_ARG and device_rc(by_arr, 1, cc.GROUP_TEXT, None, 0, None) == cc.E_ARG
        assert host_rc(g, None) == cc.OK and device_rc(by_arr, 1, cc.GROUP_TEXT, None, 0) == cc.OK
        g, by_arr = cc.group_desc([D], text=True)                          # no text column after all: no cell, no cells array
        assert host_rc(g, None, None) == cc.OK and device_rc(by_arr, 1, cc.GROUP_TEXT, None, 0, None) == cc.OK
