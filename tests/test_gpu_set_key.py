"""GPU tests of the set scan keys (CRYO_OP_IN, CRYO_OP_NOT_IN) in cryo_codec_filter_batch / _agg_batch / _group_batch /
_project_batch, their host-buffer forms and cryo_multi_*_blocks.

Every row, record, cell and byte is compared with tests/set_key_ref.py, the plain-Python statement of the rules in
include/cryo_codec.h, applied to the blocks the ORACLE encoded; the hand-made blocks of tests/set_key_cases.py also carry their
expectations written out by hand.  Outputs are filled with a sentinel before every call, and after every device-resident call the
caller's key array and its lists are read back: the library must not have written them."""
import ctypes as C
import random

import numpy as np
import pytest

import scan_calls
import set_key_cases as sc
import set_key_ref as sr
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import (REC_SENTINEL, SENTINEL, Encoder, agg_batch, agg_host, filter_batch, filter_host, group_batch, group_host,
                        multi_call, project_batch, project_host, same_agg, same_fields, same_filter, same_group, same_project)

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]


class Device(scan_calls.Device):
    """scan_calls.Device, which after every device-resident call reads the caller's lists back beside the key array"""

    def __init__(self, codec, comps, atts, keys, shift=0):
        super().__init__(codec, comps, atts, keys, shift)
        self.shift, self.lists = shift, cc.filter_desc_device(atts, keys)[2]

    def keys_untouched(self):
        super().keys_untouched()
        assert np.array_equal(self.consts.download(self.shift + self.lists.nbytes)[self.shift:], self.lists), "the caller's lists were written"


@pytest.fixture(autouse=True)
def lists_read_back(monkeypatch):
    monkeypatch.setattr(scan_calls, "Device", Device)


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def columns(atts):
    """(aggregate columns, group columns, projected columns) of a descriptor of the cases: the set keys' columns among each"""
    if len(atts) == 2:
        return [(2, sr.INT4), (1, sr.INT4)], [(2, sr.INT4)], [2, 1]
    return [(5, sr.INT4), (3, sr.INT8), (4, sr.INT2)], [(5, sr.INT4)], [5, 3, 1, 4]


def other_block(B, atts):
    if len(atts) == 2:
        return tc.build_block(B, [tc.form_tuple(atts, [i, i % 7 - 3]) for i in range(1, 40)])
    return tc.build_block(B, [sc.T(i, b"r" * (i % 5), 7 * (i % 9) - 21, i % 4 - 1, None if i % 13 == 0 else 7 * (i % 11) - 35) for i in range(1, 31)])


def batch(idx, blk, B, atts, sizes=(1, 4, 5, 9)):
    """a lone wave, a full workgroup, one over, two over (the group: two waves per workgroup), alternating with other tuples"""
    return [blk if j % 2 == 0 else other_block(B, atts) for j in range(sizes[idx % len(sizes)])]


# ---- the hand-made vectors ----
@pytest.mark.parametrize("method", METHODS)
def test_crafted_blocks_filter(dev, enc, method):
    """every hand-made block in batches of 1, 4, 5 and 9 blocks; device buffers, and for every third case host buffers and
    COUNT_ONLY"""
    for idx, (name, B, atts, blk, keys, matches, bad) in enumerate(sc.cases()):
        blocks = batch(idx, blk, B, atts)
        comps = [enc(method, b) for b in blocks]
        want = sr.filter_call(blocks, atts, keys)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name       # block 0's, as written by hand
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        got = filter_batch(dev, method, comps, B, atts, keys)
        same_filter(got, want, name)
        first = got[1][:len(matches) + len(bad)]
        assert {int(r["pos"]): int(r["status"]) for r in first if r["status"]} == bad, name
        if idx % 3 == 0:
            same_filter(filter_host(dev, method, comps, B, atts, keys), want, (name, "host buffers"))
            cwant = sr.filter_call(blocks, atts, keys, sr.COUNT_ONLY)
            same_filter(filter_batch(dev, method, comps, B, atts, keys, sr.COUNT_ONLY), cwant, (name, "count only"))
        if idx % 3 == 1:
            cwant = sr.filter_call(blocks, atts, keys, sr.COUNT_ONLY)
            same_filter(filter_host(dev, method, comps, B, atts, keys, sr.COUNT_ONLY), cwant, (name, "count only, host buffers"))


def test_crafted_blocks_agg_group_and_project(dev, enc):
    """the same blocks through the aggregate and the projection (1, 4, 5, 9 blocks) and the grouped scan (1, 2, 3 blocks) with
    the case's keys; the set key's column is an aggregate, the group and a projected column"""
    for idx, (name, B, atts, blk, keys, matches, bad) in enumerate(sc.cases()):
        method = METHODS[idx % 2]
        cols, by, pcols = columns(atts)
        host = (idx // 2) % 3 == 0
        blocks = batch(idx, blk, B, atts)
        comps = [enc(method, b) for b in blocks]
        want = sr.agg_call(blocks, atts, keys, cols)
        assert want[0]["n_match"][0] == len(matches), name
        if max(k[0] for k in keys) >= max(c[0] for c in cols):              # else the walk goes further than the keys' and may fail there
            assert want[0]["n_bad"][0] == len(bad), name
        got = agg_host(dev, method, comps, B, atts, keys, cols) if host else agg_batch(dev, method, comps, B, atts, keys, cols)
        same_agg(got, want, (name, host))
        want = sr.project_call(blocks, atts, keys, pcols)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name
        same_project((project_host if host else project_batch)(dev, method, comps, B, atts, keys, pcols), want, (name, host))
        blocks = batch(idx, blk, B, atts, (1, 2, 3))
        comps = [enc(method, b) for b in blocks]
        want = sr.group_call(blocks, atts, keys, by, cols[1:])
        same_group((group_host if host else group_batch)(dev, method, comps, B, atts, keys, by, cols[1:]), want, (name, host))


def test_big_block_all_four(dev, enc):
    """one block of 290 items at B = 16 384: hits and misses in each of the five turns"""
    atts, blk = sc.big_block()
    keys, ids = sc.BIG_KEYS, sc.BIG_MATCHES
    cols, by, pcols = columns(atts)
    for method in METHODS:
        comps = [enc(method, blk)]
        got = filter_batch(dev, method, comps, 16384, atts, keys)
        same_filter(got, sr.filter_call([blk], atts, keys), method)
        assert (got[0]["n_match"][0], got[0]["n_bad"][0]) == (len(ids), 0) and got[1]["pos"][:len(ids)].tolist() == ids
        for turn in range(5):
            inside = set(range(64 * turn + 1, min(64 * turn + 64, 290) + 1))
            assert inside & set(ids) and inside - set(ids), turn
        same_agg(agg_batch(dev, method, comps, 16384, atts, keys, cols), sr.agg_call([blk], atts, keys, cols), method)
        same_group(group_batch(dev, method, comps, 16384, atts, keys, by, cols[1:]), sr.group_call([blk], atts, keys, by, cols[1:]), method)
        same_project(project_batch(dev, method, comps, 16384, atts, keys, pcols), sr.project_call([blk], atts, keys, pcols), method)
        same_project(project_host(dev, method, comps, 16384, atts, keys, pcols), sr.project_call([blk], atts, keys, pcols), (method, "host"))


# ---- the lists of the device-resident calls ----
def test_device_lists_at_any_address(dev, enc):
    """a list at every device address mod 8; two lists adjacent in one buffer, behind a byte-string constant of odd length; the
    caller's key array and lists unchanged (checked in every device-resident call of this file)"""
    rows = [sc.T(i, b"p" * (i % 4), 100 + i, i % 3, i - 6) for i in range(1, 13)]
    blk = tc.build_block(sc.B, rows)
    keys = [(5, sr.INT4, sr.IN, [5, -5, 3, -1, 0, 2, 4, 77, -77, 1 << 35]), (3, sr.INT8, sr.NOT_IN, [106, 111, 106])]
    want = sr.filter_call([blk] * 5, sc.ATTS, keys)
    assert want[1]["pos"][:5].tolist() == [1, 5, 8, 9, 10]                   # app -5, -1, 2, 3, 4; rows 6 and 11 fall to the second key
    comps = [enc(METHOD_LZ4, blk)] * 5
    for shift in range(8):
        same_filter(filter_batch(dev, METHOD_LZ4, comps, sc.B, sc.ATTS, keys, shift=shift), want, shift)
    odd = [(2, sr.BYTES, sr.GE, b"ppp"), (5, sr.INT4, sr.IN, list(range(-5, 7, 2)) * 3), (4, sr.INT2, sr.NOT_IN, [1, 1 << 20])]
    cols, by, pcols = columns(sc.ATTS)
    for shift in (0, 3, 5):
        same_agg(agg_batch(dev, METHOD_ZSTD, [enc(METHOD_ZSTD, blk)] * 2, sc.B, sc.ATTS, odd, cols, shift=shift),
                 sr.agg_call([blk] * 2, sc.ATTS, odd, cols), shift)
        same_group(group_batch(dev, METHOD_LZ4, comps[:3], sc.B, sc.ATTS, odd, by, cols[1:], shift=shift),
                   sr.group_call([blk] * 3, sc.ATTS, odd, by, cols[1:]), shift)
    want = sr.project_call([blk] * 4, sc.ATTS, odd, pcols)
    assert want[3][0] == 4 * 2                                               # rows 3 and 11: 'ppp', app -3 and 5, small 0 and 2
    same_project(project_batch(dev, METHOD_LZ4, comps[:4], sc.B, sc.ATTS, odd, pcols), want, "adjacent lists")


# ---- a seeded property test ----
@pytest.fixture(scope="module")
def random_blocks():
    return sc.random_blocks()


def test_random_tuples_all_four(dev, enc, random_blocks):
    """64 blocks of random tuples over a small value range, the seeded key sets of set_key_cases (every size class leads one; the
    CPU test proves their coverage): the four calls against the reference, device buffers and host buffers"""
    blocks, atts = random_blocks, sc.ATTS
    cols, by, pcols = columns(atts)
    matches = 0
    for turn, keys in enumerate(sc.random_key_sets()):
        method = METHODS[turn % 2]
        comps = [enc(method, b) for b in blocks]
        want = sr.filter_call(blocks, atts, keys)
        matches += int(want[0]["n_match"].sum())
        same_filter(filter_batch(dev, method, comps, sc.B, atts, keys), want, keys)
        same_filter(filter_host(dev, method, comps, sc.B, atts, keys), want, (keys, "host buffers"))
        awant, gwant, pwant = sr.agg_call(blocks, atts, keys, cols), sr.group_call(blocks, atts, keys, by, cols[1:]), sr.project_call(blocks, atts, keys, pcols)
        same_agg(agg_batch(dev, method, comps, sc.B, atts, keys, cols), awant, keys)
        same_agg(agg_host(dev, method, comps, sc.B, atts, keys, cols), awant, (keys, "host buffers"))
        same_group(group_batch(dev, method, comps, sc.B, atts, keys, by, cols[1:]), gwant, keys)
        same_group(group_host(dev, method, comps, sc.B, atts, keys, by, cols[1:]), gwant, (keys, "host buffers"))
        same_project(project_batch(dev, method, comps, sc.B, atts, keys, pcols), pwant, keys)
        same_project(project_host(dev, method, comps, sc.B, atts, keys, pcols), pwant, (keys, "host buffers"))
    assert matches > 500, matches


# ---- chunks ----
def test_chunks_keep_the_lists(dev, enc, random_blocks):
    """CRYO_OPT_WORKSPACE_MAX_BYTES so low that the 64 blocks run in several chunks: the library's one copy of keys and lists
    serves them all, in the four calls and both buffer forms"""
    blocks, atts = random_blocks, sc.ATTS
    rng = random.Random(5)
    keys = [(5, sr.INT4, sr.IN, sc.random_set(rng, 1024)), (3, sr.INT8, sr.NOT_IN, sc.random_set(rng, 9)), (2, sr.BYTES, sr.NE, b"ab")]
    cols, by, pcols = columns(atts)
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        want = sr.filter_call(blocks, atts, keys)
        assert want[0]["n_match"].sum() > 20 and want[0]["n_match"][40:].sum() > 0
        same_filter(filter_batch(dev, method, comps, sc.B, atts, keys), want, "one chunk")
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 128 << 10)                    # at most 31 decoded blocks fit: three chunks or more
        same_filter(filter_batch(dev, method, comps, sc.B, atts, keys), want, "small budget")
        same_filter(filter_host(dev, method, comps, sc.B, atts, keys), want, "small budget, host buffers")
        awant = sr.agg_call(blocks, atts, keys, cols)
        same_agg(agg_batch(dev, method, comps, sc.B, atts, keys, cols), awant, "small budget")
        same_agg(agg_host(dev, method, comps, sc.B, atts, keys, cols), awant, "small budget, host")
        gwant = sr.group_call(blocks, atts, keys, by, cols[1:])
        same_group(group_batch(dev, method, comps, sc.B, atts, keys, by, cols[1:]), gwant, "small budget")
        same_group(group_host(dev, method, comps, sc.B, atts, keys, by, cols[1:]), gwant, "small budget, host")
        pwant = sr.project_call(blocks, atts, keys, pcols)
        same_project(project_batch(dev, method, comps, sc.B, atts, keys, pcols), pwant, "small budget")
        same_project(project_host(dev, method, comps, sc.B, atts, keys, pcols), pwant, "small budget, host")
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- several handles ----
def test_multi_handles(dev, enc, random_blocks):
    """one handle, two handles on one device, and two devices where the machine has them"""
    blocks = random_blocks[:11]
    B, atts = sc.B, sc.ATTS
    keys = [(5, sr.INT4, sr.IN, list(range(-48, 49, 3)) + [1 << 40]), (4, sr.INT2, sr.NOT_IN, [0, 1, -1])]
    cols, by, pcols = columns(atts)
    rb = sr.pr.row_layout(atts, pcols)[1]
    for devices in [(0,), (0, 0)] + ([(0, 1)] if cc.device_count() > 1 else []):
        G = len(devices)
        for method in METHODS:
            comps = [enc(method, b) for b in blocks]
            n = len(comps)
            table, recs, dst, total = multi_call(devices, lambda L, h, chk: cc.filter_blocks_call(
                L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys),
                np.full(n * B, SENTINEL, np.uint8), np.full(n * 290, REC_SENTINEL, cc.FILTER_REC)))
            if G == 1:
                same_filter((table, recs, dst, total), sr.filter_call(blocks, atts, keys), devices)
            else:
                etable, regions, etotal = sr.multi_filter_call(blocks, atts, keys, G, B)
                same_fields(table, etable, devices)
                assert total == etotal
                wb, wr = np.zeros(dst.size, bool), np.zeros(recs.size, bool)
                for b0, packed, r0, rs in regions:
                    assert np.array_equal(dst[b0:b0 + packed.size], packed) and np.array_equal(recs[r0:r0 + rs.size], rs)
                    wb[b0:b0 + packed.size] = True
                    wr[r0:r0 + rs.size] = True
                assert (dst[~wb] == SENTINEL).all() and (recs[~wr].view(np.uint8) == SENTINEL).all()
            ctab = multi_call(devices, lambda L, h, chk: cc.filter_blocks_call(
                L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, sr.COUNT_ONLY)))[0]
            same_fields(ctab, sr.filter_call(blocks, atts, keys, sr.COUNT_ONLY)[0], (devices, "count only"))
            same_agg(multi_call(devices, lambda L, h, chk: cc.agg_blocks_call(
                L.cryo_multi_agg_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.agg_desc(cols))),
                sr.agg_call(blocks, atts, keys, cols), devices)
            same_group(multi_call(devices, lambda L, h, chk: cc.group_blocks_call(
                L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.group_desc(by), cc.agg_desc(cols[1:]))),
                sr.group_call(blocks, atts, keys, by, cols[1:]), devices)
            rows = np.full((290 * n, rb), SENTINEL, np.uint8)
            rec = np.full(8 * 290 * n, SENTINEL, np.uint8).view(cc.PROJECT_REC)
            ptab, prec, prows, (tw, tr) = multi_call(devices, lambda L, h, chk: cc.project_blocks_call(
                L.cryo_multi_project_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.project_desc(pcols), rb, rows, rec))
            if G == 1:
                same_project((ptab, prec[:tr], prows[:tw], (tw, tr)), sr.project_call(blocks, atts, keys, pcols), devices)
            else:
                etable, regions, etotal = sr.multi_project_call(blocks, atts, keys, pcols, G)
                same_fields(ptab, etable, devices)
                assert (tw, tr) == etotal
                ww, wr = np.zeros(len(prows), bool), np.zeros(prec.size, bool)
                for first, erows, erecs in regions:
                    assert np.array_equal(prows[first:first + len(erows)], erows) and np.array_equal(prec[first:first + erecs.size], erecs)
                    ww[first:first + len(erows)] = True
                    wr[first:first + erecs.size] = True
                assert (prows[~ww] == SENTINEL).all() and (prec[~wr].view(np.uint8) == SENTINEL).all()


# ---- arguments ----
def test_descriptor_rules(dev, enc):
    """the argument rules of a set key -- and the older refusals beside them -- on host arrays and, through the device-resident
    call, on device arrays; the aggregate, the grouping and the projection refuse through the same rules"""
    B = sc.B
    blk = tc.build_block(B, [sc.T(1, b"p", 2, 3, 4)])
    comp = np.ascontiguousarray(enc(METHOD_LZ4, blk))
    L = dev.L
    src, szs = (C.c_void_p * 1)(comp.ctypes.data), (C.c_uint32 * 1)(comp.nbytes)
    dst, rec, table, tot = np.zeros(B, np.uint8), np.zeros(290, cc.FILTER_REC), np.zeros(1, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
    for name, atts, keys, key_rsv, ok in sc.descriptors():
        assert sr.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
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
    comps = [comp]
    bad = [(5, sr.INT4, sr.IN, list(range(1025)))]
    for call in (lambda: agg_batch(dev, METHOD_LZ4, comps, B, sc.ATTS, bad, [(1, sr.INT4)]),
                 lambda: group_batch(dev, METHOD_LZ4, comps, B, sc.ATTS, bad, [(1, sr.INT4)], []),
                 lambda: project_batch(dev, METHOD_LZ4, comps, B, sc.ATTS, bad, [1]),
                 lambda: agg_host(dev, METHOD_LZ4, comps, B, sc.ATTS, bad, [(1, sr.INT4)]),
                 lambda: group_host(dev, METHOD_LZ4, comps, B, sc.ATTS, bad, [(1, sr.INT4)], []),
                 lambda: project_host(dev, METHOD_LZ4, comps, B, sc.ATTS, bad, [1])):
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
