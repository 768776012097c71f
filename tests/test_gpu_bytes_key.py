"""GPU tests of the byte-string scan keys (CRYO_KEY_BYTES) in cryo_codec_filter_batch / _agg_batch / _group_batch, their
host-buffer forms and cryo_multi_*_blocks.

Every row, record, cell and byte is compared with tests/bytes_key_ref.py, the plain-Python statement of the rules in
include/cryo_codec.h, applied to the blocks the ORACLE encoded; the hand-made blocks of tests/bytes_key_cases.py also carry their
expectations written out by hand.  Outputs are filled with a sentinel before every call, and after every device-resident call the
caller's key array is read back: the library must not have written it."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import bytes_key_cases as bc
import bytes_key_ref as br
import tuple_craft as tc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc
from scan_calls import (REC_SENTINEL, SENTINEL, Device, Encoder, agg_batch, agg_host, filter_batch, filter_host, group_batch,
                        group_host, multi_call, same_agg, same_fields, same_filter, same_group)
from tuple_craft import Long, Toast

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def columns(atts):
    """(aggregate columns, group columns) every descriptor of the cases allows: column 1 is an int4, column 4 an int8"""
    return ([(1, br.INT4), (4, br.INT8)] if len(atts) >= 4 else [(1, br.INT4)]), [(1, br.INT4)]


def other_block(B):
    return tc.build_block(B, [bc.T(i, b"r" * (i % 5), [b"abc", b"m", b"de", b"k1"][i % 4], 10 + i % 2, b"xy"[i % 2:]) for i in range(1, 31)])


# ---- the hand-made vectors ----
@pytest.mark.parametrize("method", METHODS)
def test_crafted_blocks_filter(dev, enc, method):
    """every hand-made block in batches of 1, 4, 5 and 9 blocks (a lone wave, a full workgroup, one over, two over), alternating
    with a block of other tuples; device buffers, and for every third case host buffers and COUNT_ONLY"""
    for idx, (name, B, atts, blk, keys, matches, bad) in enumerate(bc.cases()):
        n = (1, 4, 5, 9)[idx % 4]
        blocks = [blk if j % 2 == 0 else other_block(B) for j in range(n)]
        comps = [enc(method, b) for b in blocks]
        want = br.filter_call(blocks, atts, keys)
        assert want[1]["pos"][want[1]["status"] == 0][:len(matches)].tolist() == matches, name       # block 0's, as written by hand
        assert want[0]["n_match"][0] == len(matches) and want[0]["n_bad"][0] == len(bad), name
        got = filter_batch(dev, method, comps, B, atts, keys)
        same_filter(got, want, name)
        first = got[1][:len(matches) + len(bad)]
        assert {int(r["pos"]): int(r["status"]) for r in first if r["status"]} == bad and (first["len"][first["status"] != 0] == 0).all(), name
        if idx % 3 == 0:
            same_filter(filter_host(dev, method, comps, B, atts, keys), want, (name, "host buffers"))
            cwant = br.filter_call(blocks, atts, keys, br.COUNT_ONLY)
            same_filter(filter_batch(dev, method, comps, B, atts, keys, br.COUNT_ONLY), cwant, (name, "count only"))
        if idx % 3 == 1:
            cwant = br.filter_call(blocks, atts, keys, br.COUNT_ONLY)
            same_filter(filter_host(dev, method, comps, B, atts, keys, br.COUNT_ONLY), cwant, (name, "count only, host buffers"))


def test_crafted_blocks_agg_and_group(dev, enc):
    """the same blocks through the aggregate (1, 4, 5, 9 blocks) and the grouped scan (1, 2, 3 blocks: two waves per workgroup)
    with the case's keys: an undecided tuple counts in n_bad and is in no cell and no group"""
    for idx, (name, B, atts, blk, keys, matches, bad) in enumerate(bc.cases()):
        method = METHODS[idx % 2]
        cols, by = columns(atts)
        for n, call in (((1, 4, 5, 9)[idx % 4], "agg"), ((1, 2, 3)[idx % 3], "group")):
            blocks = [blk if j % 2 == 0 else other_block(B) for j in range(n)]
            comps = [enc(method, b) for b in blocks]
            host = (idx // 2) % 3 == 0
            if call == "agg":
                want = br.agg_call(blocks, atts, keys, cols)
                got = agg_host(dev, method, comps, B, atts, keys, cols) if host else agg_batch(dev, method, comps, B, atts, keys, cols)
                same_agg(got, want, (name, host))
            else:
                want = br.group_call(blocks, atts, keys, by, cols[1:])
                got = (group_host if host else group_batch)(dev, method, comps, B, atts, keys, by, cols[1:])
                same_group(got, want, (name, host))
            assert want[0]["n_bad"][0] == len(bad) and want[0]["n_match"][0] == len(matches), name


def test_big_block_all_three(dev, enc):
    """one block of 290 items at B = 16 384: matches and undecided tuples in each of the five turns"""
    atts, blk = bc.big_block()
    keys = [(2, br.BYTES, br.EQ, b"k1")]
    for method in METHODS:
        comps = [enc(method, blk)]
        got = filter_batch(dev, method, comps, 16384, atts, keys)
        same_filter(got, br.filter_call([blk], atts, keys), method)
        assert (got[0]["n_match"][0], got[0]["n_bad"][0]) == (91, 17)
        recs = got[1][:108]
        und = recs[recs["status"] == br.UNDECIDED]
        assert und["pos"].tolist() == list(range(17, 291, 17)) and (und["len"] == 0).all()
        for turn in range(5):                                            # both kinds in every turn of 64 items
            st = recs["status"][(recs["pos"] > 64 * turn) & (recs["pos"] <= 64 * turn + 64)]
            assert (st == 0).any() and (st == br.UNDECIDED).any(), turn
        same_agg(agg_batch(dev, method, comps, 16384, atts, keys, [(1, br.INT4)]), br.agg_call([blk], atts, keys, [(1, br.INT4)]), method)
        same_group(group_batch(dev, method, comps, 16384, atts, keys, [(1, br.INT4)], []),
                   br.group_call([blk], atts, keys, [(1, br.INT4)], []), method)


# ---- the constants of the device-resident calls ----
def test_device_constants_at_any_address(dev, enc):
    """a constant at an odd device address; two constants adjacent in one buffer; the caller's key array unchanged (checked in
    every device-resident call of this file)"""
    pre = [bc.T(i, b"p", p, 10 * i, b"t") for i, p in enumerate((b"abb", b"abc", b"abcz", b"abd", b"ab", b"abd0", b"abc\xff"), 1)]
    blk = tc.build_block(bc.B, pre)
    keys = [bc.K3(br.GE, b"abc"), bc.K3(br.LT, b"abd")]                 # 'abc' and 'abd' back to back: one of them is odd
    want = br.filter_call([blk] * 5, bc.ATTS, keys)
    assert want[1]["pos"][:3].tolist() == [2, 3, 7]
    comps = [enc(METHOD_LZ4, blk)] * 5
    for shift in range(8):
        same_filter(filter_batch(dev, METHOD_LZ4, comps, bc.B, bc.ATTS, keys, shift=shift), want, shift)
    long_keys = [bc.K3(br.NE, bc.pattern(255)), (5, br.BYTES, br.EQ, b"t"), bc.K3(br.GT, bc.pattern(17))]
    for shift in (1, 6):
        same_agg(agg_batch(dev, METHOD_ZSTD, [enc(METHOD_ZSTD, blk)] * 2, bc.B, bc.ATTS, long_keys, [(4, br.INT8)], shift=shift),
                 br.agg_call([blk] * 2, bc.ATTS, long_keys, [(4, br.INT8)]), shift)
        same_group(group_batch(dev, METHOD_LZ4, comps[:3], bc.B, bc.ATTS, keys, [(1, br.INT4)], [(4, br.INT8)], shift=shift),
                   br.group_call([blk] * 3, bc.ATTS, keys, [(1, br.INT4)], [(4, br.INT8)]), shift)


# ---- a seeded property test ----
def random_value(rng):
    kind = rng.random()
    if kind < 0.08:
        return None
    if kind < 0.14:
        return Toast()
    payload = bytes(rng.choice(b"ab\xe9") for _ in range(rng.choice((0, 1, 1, 2, 2, 3, 7, 8, 9, 16, 17, 40, 130))))
    if kind < 0.22:
        return ("compressed", payload + b"zzzz")
    return Long(payload) if kind < 0.4 else payload


def random_tuple(rng, rowid):
    vals = [rowid, b"p" * rng.randrange(9), random_value(rng), rng.randrange(-3, 4), random_value(rng)]
    squeezed = [(Long(v[1]) if isinstance(v, tuple) else v) for v in vals]
    t = tc.form_tuple(bc.ATTS, squeezed[:rng.choice((5, 5, 5, 3, 2))])
    for v in vals[:len(squeezed)]:
        if isinstance(v, tuple) and t.count(struct.pack("<I", (len(v[1]) + 4) << 2) + v[1]) == 1:
            t = bc.compressed(t, v[1])
    return t


def random_keys(rng):
    keys = []
    for _ in range(rng.randrange(1, 5)):
        kind = rng.random()
        if kind < 0.6:
            const = bytes(rng.choice(b"ab\xe9") for _ in range(rng.choice((0, 1, 1, 2, 2, 3, 8, 9))))
            keys.append((rng.choice((3, 3, 5)), br.BYTES, rng.randrange(br.LT, br.NE + 1), const))
        elif kind < 0.8:
            keys.append((4, br.INT8, rng.randrange(br.LT, br.NE + 1), rng.randrange(-2, 3)))
        else:
            keys.append((rng.choice((3, 5)), 0, rng.choice((br.ISNULL, br.NOTNULL)), 0))
    return keys


@pytest.fixture(scope="module")
def random_blocks():
    rng = random.Random(20240917)
    blocks = []
    for k in range(64):
        tuples, room = [], bc.B - 8
        for i in range(rng.randrange(1, 30)):
            t = random_tuple(rng, 100 * k + i)
            if room < tc.maxalign(len(t)) + 8:
                break
            tuples.append(t)
            room -= tc.maxalign(len(t)) + 8
        blocks.append(tc.build_block(bc.B, tuples))
    return blocks


def test_random_tuples_all_three(dev, enc, random_blocks):
    """64 blocks of random tuples over a small alphabet (so that = hits occur), random key sets: the three calls against the
    reference, device buffers and host buffers"""
    rng = random.Random(7)
    blocks = random_blocks
    seen = {"match": 0, "undecided": 0, "tuple": 0}
    for turn in range(8):
        keys, method = random_keys(rng), METHODS[turn % 2]
        comps = [enc(method, b) for b in blocks]
        want = br.filter_call(blocks, bc.ATTS, keys)
        seen["match"] += int(want[0]["n_match"].sum())
        seen["undecided"] += int((want[1]["status"] == br.UNDECIDED).sum())
        same_filter(filter_batch(dev, method, comps, bc.B, bc.ATTS, keys), want, keys)
        same_filter(filter_host(dev, method, comps, bc.B, bc.ATTS, keys), want, (keys, "host buffers"))
        cols, by = [(4, br.INT8), (1, br.INT4)], [(4, br.INT8)]
        awant, gwant = br.agg_call(blocks, bc.ATTS, keys, cols), br.group_call(blocks, bc.ATTS, keys, by, cols[1:])
        same_agg(agg_batch(dev, method, comps, bc.B, bc.ATTS, keys, cols), awant, keys)
        same_agg(agg_host(dev, method, comps, bc.B, bc.ATTS, keys, cols), awant, (keys, "host buffers"))
        same_group(group_batch(dev, method, comps, bc.B, bc.ATTS, keys, by, cols[1:]), gwant, keys)
        same_group(group_host(dev, method, comps, bc.B, bc.ATTS, keys, by, cols[1:]), gwant, (keys, "host buffers"))
    assert seen["match"] > 500 and seen["undecided"] > 200, seen


# ---- chunks ----
def test_chunks_keep_the_constants(dev, enc, random_blocks):
    """CRYO_OPT_WORKSPACE_MAX_BYTES so low that the 64 blocks run in several chunks: the library's copy of keys and constants
    serves them all"""
    blocks = random_blocks
    keys = [bc.K3(br.GE, b"a"), bc.K3(br.LT, b"b"), (5, br.BYTES, br.NE, b"ab")]
    cols, by = [(4, br.INT8), (1, br.INT4)], [(4, br.INT8)]
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        want = br.filter_call(blocks, bc.ATTS, keys)
        assert want[0]["n_match"].sum() > 20 and want[0]["n_match"][40:].sum() > 0
        whole = filter_batch(dev, method, comps, bc.B, bc.ATTS, keys)
        same_filter(whole, want, "one chunk")
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 128 << 10)                    # at most 31 decoded blocks fit: three chunks or more
        same_filter(filter_batch(dev, method, comps, bc.B, bc.ATTS, keys), want, "small budget")
        same_filter(filter_host(dev, method, comps, bc.B, bc.ATTS, keys), want, "small budget, host buffers")
        same_agg(agg_batch(dev, method, comps, bc.B, bc.ATTS, keys, cols), br.agg_call(blocks, bc.ATTS, keys, cols), "small budget")
        same_agg(agg_host(dev, method, comps, bc.B, bc.ATTS, keys, cols), br.agg_call(blocks, bc.ATTS, keys, cols), "small budget, host")
        gwant = br.group_call(blocks, bc.ATTS, keys, by, cols[1:])
        same_group(group_batch(dev, method, comps, bc.B, bc.ATTS, keys, by, cols[1:]), gwant, "small budget")
        same_group(group_host(dev, method, comps, bc.B, bc.ATTS, keys, by, cols[1:]), gwant, "small budget, host")
        dev.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


# ---- several handles ----
def test_multi_handles(dev, enc, random_blocks):
    """one handle, two handles on one device, and two devices where the machine has them"""
    blocks = random_blocks[:11]
    B, atts = bc.B, bc.ATTS
    keys = [bc.K3(br.GE, b"a"), (5, br.BYTES, br.NE, b"ab")]
    cols, by = [(4, br.INT8)], [(1, br.INT4)]
    for devices in [(0,), (0, 0)] + ([(0, 1)] if cc.device_count() > 1 else []):
        G = len(devices)
        for method in METHODS:
            comps = [enc(method, b) for b in blocks]
            n = len(comps)
            table, recs, dst, total = multi_call(devices, lambda L, h, chk: cc.filter_blocks_call(
                L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys),
                np.full(n * B, SENTINEL, np.uint8), np.full(n * 290, REC_SENTINEL, cc.FILTER_REC)))
            if G == 1:
                same_filter((table, recs, dst, total), br.filter_call(blocks, atts, keys), devices)
            else:
                etable, regions, etotal = br.multi_filter_call(blocks, atts, keys, G, B)
                same_fields(table, etable, devices)
                assert total == etotal
                wb, wr = np.zeros(dst.size, bool), np.zeros(recs.size, bool)
                for b0, packed, r0, rs in regions:
                    assert np.array_equal(dst[b0:b0 + packed.size], packed) and np.array_equal(recs[r0:r0 + rs.size], rs)
                    wb[b0:b0 + packed.size] = True
                    wr[r0:r0 + rs.size] = True
                assert (dst[~wb] == SENTINEL).all() and (recs[~wr].view(np.uint8) == SENTINEL).all()
            ctab = multi_call(devices, lambda L, h, chk: cc.filter_blocks_call(
                L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys, br.COUNT_ONLY)))[0]
            same_fields(ctab, br.filter_call(blocks, atts, keys, br.COUNT_ONLY)[0], (devices, "count only"))
            same_agg(multi_call(devices, lambda L, h, chk: cc.agg_blocks_call(
                L.cryo_multi_agg_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.agg_desc(cols))),
                br.agg_call(blocks, atts, keys, cols), devices)
            same_group(multi_call(devices, lambda L, h, chk: cc.group_blocks_call(
                L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(atts, keys), cc.group_desc(by), cc.agg_desc(cols))),
                br.group_call(blocks, atts, keys, by, cols), devices)


# ---- arguments ----
def test_descriptor_rules(dev, enc):
    """the argument rules of a byte-string key -- and the filter's older refusals beside them -- on host arrays and, through the
    device-resident call, on device arrays"""
    B = bc.B
    blk = tc.build_block(B, [bc.T(1, b"p", b"abc", 10, b"t")])
    comp = np.ascontiguousarray(enc(METHOD_LZ4, blk))
    L = dev.L
    src, szs = (C.c_void_p * 1)(comp.ctypes.data), (C.c_uint32 * 1)(comp.nbytes)
    dst, rec, table, tot = np.zeros(B, np.uint8), np.zeros(290, cc.FILTER_REC), np.zeros(1, cc.FILTER_BLOCK), (C.c_uint64 * 2)()
    for name, atts, keys, key_rsv, ok in bc.descriptors():
        assert br.desc_ok(atts, keys, 0, 0, key_rsv) == ok, name
        f, a, k = cc.filter_desc(atts, keys)
        if key_rsv:
            k["rsv"][:len(key_rsv)] = key_rsv
        rc = L.cryo_codec_filter_blocks(dev.h, METHOD_LZ4, src, szs, 1, B, C.byref(f), dst.ctypes.data, dst.nbytes, rec.ctypes.data,
                                        rec.size, table.ctypes.data, tot)
        assert rc == (cc.OK if ok else cc.E_ARG), (name, rc)
        with Device(dev, [comp], atts, keys, shift=1) as d:
            if key_rsv:
                d.k["rsv"][:len(key_rsv)] = key_rsv
                d.keys.upload(d.k)
            d_dst, d_rec, d_tab, d_tot = d.alloc(B), d.alloc(8 * 290), d.alloc(32), d.alloc(16)
            g = cc.CryoFilter(len(atts), len(keys), 0, 0, d.atts.ptr, d.keys.ptr)
            rc = L.cryo_codec_filter_batch(dev.h, METHOD_LZ4, d.src.ptr, d.off.ptr, d.sz.ptr, B, 1, C.byref(g), d_dst.ptr, B, d_rec.ptr,
                                           290, d_tab.ptr, d_tot.ptr)
            dev.sync()
            assert rc == (cc.OK if ok else cc.E_ARG), (name, "device arrays", rc)
    # a byte-string entry is no aggregate and no group column
    comps, f = [comp], cc.filter_desc(bc.ATTS, [bc.K3(br.EQ, b"abc")])
    with pytest.raises(CryoError) as e:
        dev.agg_blocks(METHOD_LZ4, comps, B, f, cc.agg_desc([(3, br.BYTES)]))
    assert e.value.code == cc.E_ARG
    with pytest.raises(CryoError) as e:
        dev.group_blocks(METHOD_LZ4, comps, B, f, cc.group_desc([(3, br.BYTES)]))
    assert e.value.code == cc.E_ARG
    with pytest.raises(CryoError) as e:
        dev.group_blocks(METHOD_LZ4, comps, B, f, cc.group_desc([(1, br.INT4)]), cc.agg_desc([(5, br.BYTES)]))
    assert e.value.code == cc.E_ARG
    # the refusals of the aggregate and the grouping with a bad byte-string key, through the device-resident calls
    bad = [bc.K3(br.EQ, b"x" * 257)]
    for call in (lambda: agg_batch(dev, METHOD_LZ4, comps, B, bc.ATTS, bad, [(1, br.INT4)]),
                 lambda: group_batch(dev, METHOD_LZ4, comps, B, bc.ATTS, bad, [(1, br.INT4)], [])):
        with pytest.raises(CryoError) as e:
            call()
        assert e.value.code == cc.E_ARG
