"""GPU tests of the float scan keys and float aggregate columns (CRYO_KEY_FLOAT4, CRYO_KEY_FLOAT8) in the device-resident calls
cryo_codec_filter_batch / _agg_batch / _group_batch / _project_batch.

Every row, record, cell and byte is compared with tests/float_ref.py, the plain-Python statement of the rules in
include/cryo_codec.h, applied to the blocks the ORACLE encoded; the hand-made blocks of tests/float_cases.py also carry their
expectations written out by hand.  Outputs are filled with a sentinel before every call, and after every call the caller's key
array is read back: the library must not have written it.  The host-buffer forms are test_gpu_float_host.py's."""
import ctypes as C

import numpy as np
import pytest

import agg_ref
import float_cases as fc
import float_ref as fl
import group_ref
import scan_calls
import truth_calls as tcall
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import Encoder, same_agg, same_filter, same_group, same_project

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
COLS = [(2, fl.FLOAT8), (6, fl.INT8), (3, fl.FLOAT4), (5, fl.FLOAT4)]     # float8, an integer beside it, float4 on (4, 4) and on (4, 8)
BY = [(7, fl.INT2)]
PCOLS = [2, 1, 3, 5]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def other_block(B):
    return tc.build_block(B, [fc.row(i, 0.5 * i - 7.0, None if i % 5 == 0 else 1.0 / i, -0.25 * i, k=i % 4, g=i % 3) for i in range(1, 31)])


def batch(idx, blk, B, sizes=(1, 4, 5, 9)):
    """a lone wave, a full workgroup, one over, two over (the group: two waves per workgroup), alternating with other tuples"""
    return [blk if j % 2 == 0 else other_block(B) for j in range(sizes[idx % len(sizes)])]


# ---- the hand-made vectors ----
def test_crafted_blocks_filter_and_project(dev, enc):
    """every hand-made block in batches of 1, 4, 5 and 9 blocks, the methods alternating: the filter, COUNT_ONLY for every third
    case, and the projection, which brings the float columns back bit for bit"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(fc.cases()):
        method = METHODS[idx % 2]
        blocks = batch(idx, blk, B)
        comps = [enc(method, b) for b in blocks]
        want = fl.filter_call(blocks, atts, keys, 0, W)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name       # block 0's, as written by hand
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        got = tcall.filter_batch(dev, method, comps, B, atts, keys, 0, W)
        same_filter(got, want, name)
        first = got[1][:len(matches) + len(bad)]
        assert {int(r["pos"]): int(r["status"]) for r in first if r["status"]} == bad, name
        if idx % 3 == 0:
            cwant = fl.filter_call(blocks, atts, keys, fl.COUNT_ONLY, W)
            same_filter(tcall.filter_batch(dev, method, comps, B, atts, keys, fl.COUNT_ONLY, W), cwant, (name, "count only"))
        if idx % 2 == 0:
            same_project(tcall.project_batch(dev, method, comps, B, atts, keys, PCOLS, W), fl.project_call(blocks, atts, keys, PCOLS, W), name)


def test_crafted_blocks_agg_and_group(dev, enc):
    """the same blocks through the aggregate (1, 4, 5, 9 blocks) and the grouped scan (1, 2, 3 blocks) with mixed integer and float
    aggregate columns"""
    for idx, (name, B, atts, blk, keys, W, matches, bad) in enumerate(fc.cases()):
        if idx % 2:
            continue
        method = METHODS[(idx // 2) % 2]
        blocks = batch(idx, blk, B)
        comps = [enc(method, b) for b in blocks]
        want = fl.agg_call(blocks, atts, keys, COLS, W)
        assert want[0]["n_match"][0] == len(matches), name
        same_agg(tcall.agg_batch(dev, method, comps, B, atts, keys, COLS, W), want, name)
        blocks = batch(idx, blk, B, (1, 2, 3))
        comps = [enc(method, b) for b in blocks]
        same_group(tcall.group_batch(dev, method, comps, B, atts, keys, BY, COLS, W), fl.group_call(blocks, atts, keys, BY, COLS, W), name)


def cell_words(cell):
    return tuple(int(w) for w in np.frombuffer(cell.tobytes(), "<u8"))


def test_crafted_sums(dev, enc):
    """the sums written out by hand -- cancellation in a lane and across lanes, the infinities, NaN, overflow, all NULL --
    through the aggregate and, as one group, through the grouped scan; a float key and no key at all beside the integer key"""
    for idx, (name, values, expect) in enumerate(fc.SUM_CASES):
        method = METHODS[idx % 2]
        blk = fc.sum_block(values)
        comps = [enc(method, blk)]
        rows, cells = tcall.agg_batch(dev, method, comps, fc.SUM_B, fc.ATTS, fc.SUM_KEYS, fc.SUM_COLS)
        assert cell_words(cells[0, 0]) == fc.words(expect), (name, [hex(w) for w in cell_words(cells[0, 0])])
        same_agg((rows, cells), fl.agg_call([blk], fc.ATTS, fc.SUM_KEYS, fc.SUM_COLS), name)
        got = tcall.group_batch(dev, method, comps, fc.SUM_B, fc.ATTS, fc.SUM_KEYS, [(6, fl.INT8)], fc.SUM_COLS)
        gexp = fc.words(expect[:3] + fc.GROUP_SUMS.get(name, expect[3:]))
        assert got[3] == 1 and cell_words(got[2][0, 0]) == gexp, (name, [hex(w) for w in cell_words(got[2][0, 0])])
        same_group(got, fl.group_call([blk], fc.ATTS, fc.SUM_KEYS, [(6, fl.INT8)], fc.SUM_COLS), name)
    # no key: every tuple matches, the float column alone asks for the float kernel
    blk = fc.sum_block(fc.SUM_CASES[0][1])
    comps = [enc(METHOD_LZ4, blk)] * 5
    same_agg(tcall.agg_batch(dev, METHOD_LZ4, comps, fc.SUM_B, fc.ATTS, [], [(2, fl.FLOAT8)]), fl.agg_call([blk] * 5, fc.ATTS, [], [(2, fl.FLOAT8)]), "no key")
    same_group(tcall.group_batch(dev, METHOD_LZ4, comps, fc.SUM_B, fc.ATTS, [], BY, [(2, fl.FLOAT8)]),
               fl.group_call([blk] * 5, fc.ATTS, [], BY, [(2, fl.FLOAT8)]), "no key")


@pytest.mark.parametrize("n", fc.SIZES)
def test_block_sizes_all_four(dev, enc, n):
    """blocks of 1, 63, 64, 65 and 290 items (five turns, the last partial), matches and misses in every turn, both methods"""
    blk = fc.sized_block(n, n)
    atts, keys, B = fc.ATTS, fc.SIZED_KEYS, fc.SIZED_B
    want = fl.filter_call([blk], atts, keys)
    pos = set(want[1]["pos"][want[1]["status"] == 0].tolist())
    if n >= 63:
        for turn in range((n + 63) // 64):
            inside = set(range(64 * turn + 1, min(64 * turn + 64, n) + 1))
            assert len(inside) == 1 or (inside & pos and inside - pos), turn      # a turn of one item cannot hold both
    for method in METHODS:
        comps = [enc(method, blk)]
        same_filter(tcall.filter_batch(dev, method, comps, B, atts, keys), want, n)
        same_agg(tcall.agg_batch(dev, method, comps, B, atts, keys, fc.SIZED_COLS), fl.agg_call([blk], atts, keys, fc.SIZED_COLS), n)
        same_group(tcall.group_batch(dev, method, comps, B, atts, keys, fc.SIZED_BY, fc.SIZED_COLS),
                   fl.group_call([blk], atts, keys, fc.SIZED_BY, fc.SIZED_COLS), n)
        same_project(tcall.project_batch(dev, method, comps, B, atts, keys, PCOLS), fl.project_call([blk], atts, keys, PCOLS), n)


# ---- a seeded property test ----
@pytest.fixture(scope="module")
def random_blocks():
    return fc.random_blocks()


def test_random_tuples_all_four(dev, enc, random_blocks):
    """24 blocks of random tuples -- zeros of both signs, infinities, NaNs, subnormals, NULLs, cut tuples --, random float keys
    under random truth tables, one to four mixed integer / float aggregate columns: bit-exact against the reference, and two
    identical calls return identical bytes"""
    blocks, atts = random_blocks, fc.ATTS
    matches = 0
    for turn, (keys, W, cols) in enumerate(fc.random_descriptors()):
        method = METHODS[turn % 2]
        comps = [enc(method, b) for b in blocks]
        want = fl.filter_call(blocks, atts, keys, 0, W)
        matches += int(want[0]["n_match"].sum())
        same_filter(tcall.filter_batch(dev, method, comps, fc.B, atts, keys, 0, W), want, keys)
        awant = fl.agg_call(blocks, atts, keys, cols, W)
        got = tcall.agg_batch(dev, method, comps, fc.B, atts, keys, cols, W)
        same_agg(got, awant, (keys, cols))
        again = tcall.agg_batch(dev, method, comps, fc.B, atts, keys, cols, W)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
        gwant = fl.group_call(blocks, atts, keys, BY, cols, W)
        got = tcall.group_batch(dev, method, comps, fc.B, atts, keys, BY, cols, W)
        same_group(got, gwant, (keys, cols))
        again = tcall.group_batch(dev, method, comps, fc.B, atts, keys, BY, cols, W)
        assert all(g.tobytes() == a.tobytes() for g, a in zip(got[:3], again[:3]))
        if turn % 2 == 0:
            same_project(tcall.project_batch(dev, method, comps, fc.B, atts, keys, PCOLS, W), fl.project_call(blocks, atts, keys, PCOLS, W), keys)
    assert matches > 300, matches


def test_integer_only_descriptors_are_what_they_were(dev, enc, random_blocks):
    """a descriptor without a float type returns what agg_ref and group_ref expect, and the same bytes as its integer columns
    return beside a float column"""
    blocks, atts = random_blocks[:9], fc.ATTS
    keys, cols = [(6, fl.INT8, fl.GE, -2), (1, fl.INT4, fl.NE, 3)], [(6, fl.INT8), (7, fl.INT2), (1, fl.INT4)]
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    got = scan_calls.agg_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, cols)
    same_agg(got, agg_ref.agg_call(blocks, atts, keys, cols), "integer only")
    mixed = tcall.agg_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, cols + [(2, fl.FLOAT8)])
    assert got[0].tobytes() == mixed[0].tobytes() and got[1].tobytes() == mixed[1][:, :3].tobytes()
    ggot = scan_calls.group_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, BY, cols)
    same_group(ggot, group_ref.group_call(blocks, atts, keys, BY, cols), "integer only")
    gmixed = tcall.group_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, BY, [(2, fl.FLOAT8)] + cols)
    assert ggot[1].tobytes() == gmixed[1].tobytes() and ggot[2].tobytes() == gmixed[2][:, 1:].tobytes()


# ---- chunks ----
def test_chunks(dev, enc, random_blocks):
    """CRYO_OPT_WORKSPACE_MAX_BYTES so low that the 24 blocks run in several chunks: the library's one copy of the mapped keys
    serves them all"""
    blocks, atts = random_blocks, fc.ATTS
    keys, cols = [(2, fl.FLOAT8, fl.GT, -1.0), (3, fl.FLOAT4, fl.NE, fc.NAN)], COLS
    comps = [enc(METHOD_LZ4, b) for b in blocks]
    want = fl.filter_call(blocks, atts, keys)
    assert want[0]["n_match"][12:].sum() > 0
    dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 64 << 10)                          # at most 15 decoded blocks fit: two chunks or more
    same_filter(tcall.filter_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys), want, "small budget")
    same_agg(tcall.agg_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, cols), fl.agg_call(blocks, atts, keys, cols), "small budget")
    same_group(tcall.group_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, BY, cols), fl.group_call(blocks, atts, keys, BY, cols), "small budget")
    same_project(tcall.project_batch(dev, METHOD_LZ4, comps, fc.B, atts, keys, PCOLS), fl.project_call(blocks, atts, keys, PCOLS), "small budget")


# ---- arguments ----
def test_descriptor_rules(dev, enc):
    """the descriptor table of a float key on host arrays and, through the device-resident call, on device arrays; a float
    aggregate column's rules, and a float group column refused"""
    B = fc.B
    comp = np.ascontiguousarray(enc(METHOD_LZ4, fc.specials_block()))
    L = dev.L
    src, szs = (C.c_void_p * 1)(comp.ctypes.data), (C.c_uint32 * 1)(comp.nbytes)
    dst, rec, table, tot = np.zeros(B, np.uint8), np.zeros(290, cc.FILTER_REC), np.zeros(1, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
    for name, atts, keys, key_rsv, ok in fc.descriptors():
        f, a, k = cc.filter_desc(atts, keys)
        if key_rsv:
            k["rsv"][:len(key_rsv)] = key_rsv
        rc = L.cryo_codec_filter_blocks(dev.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), dst.ctypes.data, dst.nbytes, rec.ctypes.data,
                                        rec.size, table.ctypes.data, tot)
        assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
        with scan_calls.Device(dev, [comp], atts, keys, shift=1) as d:
            if key_rsv:
                d.k["rsv"][:len(key_rsv)] = key_rsv
                d.keys.upload(d.k)
            d_dst, d_rec, d_tab, d_tot = d.alloc(B), d.alloc(8 * 290), d.alloc(32), d.alloc(16)
            g = cc.CryoFilter(len(atts), len(keys), 0, 0, d.atts.ptr, d.keys.ptr)
            rc = L.cryo_codec_filter_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(g), d_dst.ptr, B, d_rec.ptr,
                                           290, d_tab.ptr, d_tot.ptr)
            dev.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    comps, atts = [comp], fc.ATTS
    tcall.agg_batch(dev, METHOD_LZ4, comps, B, atts, [], [(5, fl.FLOAT4), (3, fl.FLOAT4), (2, fl.FLOAT8)])       # (4, 8), (4, 4), (8, 8)
    for call in (lambda: tcall.agg_batch(dev, METHOD_LZ4, comps, B, atts, [], [(6, fl.FLOAT4)]),                 # an int8 column
                 lambda: tcall.agg_batch(dev, METHOD_LZ4, comps, B, atts, [], [(3, fl.FLOAT8)]),                 # a float4 column
                 lambda: tcall.agg_batch(dev, METHOD_LZ4, comps, B, atts, [], [(4, fl.FLOAT8)]),                 # a varlena
                 lambda: tcall.agg_batch(dev, METHOD_LZ4, comps, B, [(4, 4), (8, 4)], [], [(2, fl.FLOAT8)]),     # attalign 4
                 lambda: tcall.group_batch(dev, METHOD_LZ4, comps, B, atts, [], [(2, fl.FLOAT8)], []),           # a float group column
                 lambda: tcall.group_batch(dev, METHOD_LZ4, comps, B, atts, [], [(7, fl.INT2), (3, fl.FLOAT4)], [(2, fl.FLOAT8)]),
                 lambda: tcall.group_batch(dev, METHOD_LZ4, comps, B, atts, [(2, fl.FLOAT8, fl.IN, [1])], BY, []),
                 lambda: tcall.project_batch(dev, METHOD_LZ4, comps, B, atts, [(3, fl.FLOAT8, fl.LT, 1.0)], [1])):
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
