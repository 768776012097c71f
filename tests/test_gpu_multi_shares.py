"""Two corners of the cryo_multi_* calls that 11 blocks over two handles with generous caps do not reach: more handles than
blocks (a handle with an empty share, the deal's tail), and a handle's region that ends exactly at the caller's cap or one unit
short of its need (a region that reaches beyond its cap is cut there, include/cryo_codec.h).  Synthetic blocks of 8 KiB, both
methods, every handle on device 0.  The references (fetch_ref, filter_ref, project_ref: multi_call) alone decide where handle 1's
region starts and what its share packs."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import agg_ref as ar
import fetch_ref as fe
import filter_ref as fr
import group_ref as gr
import project_ref as pr
import scan_calls as sc
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

pytestmark = pytest.mark.gpu

SENTINEL = sc.SENTINEL
SYNTH_ATTS = [(4, 4), (-1, 4)]
B = 8192
DISTS = (1, 2, 1, 0, 2)            # the generator's distribution per block: 1 and 2 give tuples of SYNTH_ATTS, 0 gives 290 bad items
KEYS = [(1, fr.INT4, fr.GE, 50), (1, fr.INT4, fr.LT, 1300)]              # block k's rowids are 290 k + 1 ...: a part of blocks 0 and 4
ROWID = [(1, fr.INT4)]
COLS = [1]
ROW_BYTES = pr.row_layout(SYNTH_ATTS, COLS)[1]
METHODS = [METHOD_LZ4, METHOD_ZSTD]


@pytest.fixture(scope="module")
def five(oracle):
    """five blocks, their streams per method and the positions asked of each: a few that exist, one that does not"""
    raws = [oracle.synth(17, k, B, DISTS[k]) for k in range(5)]
    comps = {METHOD_LZ4: [oracle.lz4_compress(r, 1) for r in raws], METHOD_ZSTD: [oracle.zstd_compress(r, 1) for r in raws]}
    requests = [list(range(1 + k, 100, 7)) + [291] for k in range(5)]
    return raws, comps, requests


@contextlib.contextmanager
def handles(G):
    """(library, a cryo_multi of G handles on device 0, chk that raises CryoError)"""
    L = cc.lib()
    h = C.c_void_p()
    assert L.cryo_multi_open((C.c_int * G)(*([0] * G)), G, C.byref(h)) == 0
    try:
        def chk(rc, what):
            if rc != 0:
                raise CryoError(rc, what, L.cryo_multi_last_error(h).decode())
        yield L, h, chk
    finally:
        L.cryo_multi_close(h)


# ---- the calls: every buffer larger than the cap passed and filled with SENTINEL ----
def fetch(m, method, comps, requests, cap=None):
    L, h, chk = m
    big = np.full(len(comps) * B + 64, SENTINEL, np.uint8)
    recs, _, total = cc.fetch_blocks_call(L.cryo_multi_fetch_blocks, h, chk, method, comps, B, requests,
                                          big[:len(comps) * B if cap is None else cap])
    return recs, big, total


def filter_(m, method, comps, dst_cap=None, rec_cap=None):
    L, h, chk = m
    n = len(comps)
    big, big_rec = np.full(n * B + 64, SENTINEL, np.uint8), np.full(n * 290 + 8, sc.REC_SENTINEL, cc.FILTER_REC)
    table, _, _, total = cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, method, comps, B, cc.filter_desc(SYNTH_ATTS, KEYS),
                                               big[:n * B if dst_cap is None else dst_cap],
                                               big_rec[:n * 290 if rec_cap is None else rec_cap])
    return table, big_rec, big, total


def project(m, method, comps, row_cap=None, rec_cap=None):
    L, h, chk = m
    n = len(comps)
    big = np.full((n * 290 + 8, ROW_BYTES), SENTINEL, np.uint8)
    big_rec = np.full(8 * (n * 290 + 8), SENTINEL, np.uint8).view(cc.PROJECT_REC)
    table, _, _, total = cc.project_blocks_call(L.cryo_multi_project_blocks, h, chk, method, comps, B,
                                                cc.filter_desc(SYNTH_ATTS, KEYS), cc.project_desc(COLS), ROW_BYTES,
                                                big[:n * 290 if row_cap is None else row_cap],
                                                big_rec[:n * 290 if rec_cap is None else rec_cap])
    return table, big_rec, big, total


# ---- comparing with a reference's multi_call: the table, the totals, every region, and the sentinel everywhere else ----
def only_regions(buf, regions, what):
    """regions: [(first entry, expected entries)]; they hold what is expected, do not overlap, and nothing else was written"""
    written = np.zeros(buf.shape[0], bool)
    for first, want in regions:
        assert buf[first:first + want.shape[0]].tobytes() == want.tobytes(), (what, first)
        assert not written[first:first + want.shape[0]].any(), (what, first)
        written[first:first + want.shape[0]] = True
    assert (buf[~written].view(np.uint8) == SENTINEL).all(), (what, "written outside the regions' used parts")


def same_fetch(got, want, what):
    (recs, big, total), (erecs, regions, etotal) = got, want
    sc.same_fields(recs, erecs, what)
    assert total == etotal, (what, total, etotal)
    only_regions(big, regions, what)


def same_filter(got, want, what):
    (table, recs, big, total), (etable, regions, etotal) = got, want
    sc.same_fields(table, etable, what)
    assert tuple(total) == tuple(etotal), (what, total, etotal)
    only_regions(big, [(b0, packed) for b0, packed, _, _ in regions], what)
    only_regions(recs, [(r0, rs) for _, _, r0, rs in regions], what)


def same_project(got, want, what):
    (table, recs, big, total), (etable, regions, etotal) = got, want
    sc.same_fields(table, etable, what)
    assert tuple(total) == tuple(etotal), (what, total, etotal)
    only_regions(big, [(first, rows) for first, rows, _ in regions], what)
    only_regions(recs, [(first, rs) for first, _, rs in regions], what)


def refused(call, bufs_and_caps, what):
    """the call returns CRYO_E_DSTSIZE and leaves everything at or beyond each cap as it was"""
    with pytest.raises(CryoError) as e:
        call()
    assert e.value.code == cc.E_DSTSIZE, (what, e.value.code)
    for buf, cap in bufs_and_caps:
        assert (buf[cap:].view(np.uint8) == SENTINEL).all(), (what, "written beyond the cap")


# ---- more handles than blocks ----
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("method", METHODS)
def test_more_handles_than_blocks(five, method, n):
    """three handles and 1, 2 or 4 blocks: a handle without a share is not touched, and the regions of those with one are the
    reference's for G = 3; agg and group give the single-handle result"""
    raws, comps, requests = five
    raws, comps, requests = raws[:n], comps[method][:n], requests[:n]
    with handles(3) as m:
        same_fetch(fetch(m, method, comps, requests), fe.multi_call(raws, requests, 3, B), ("fetch", n))
        same_filter(filter_(m, method, comps), fr.multi_call(raws, SYNTH_ATTS, KEYS, 3, B), ("filter", n))
        same_project(project(m, method, comps), pr.multi_call(raws, SYNTH_ATTS, KEYS, COLS, 3), ("project", n))
        L, h, chk = m
        got = cc.agg_blocks_call(L.cryo_multi_agg_blocks, h, chk, method, comps, B, cc.filter_desc(SYNTH_ATTS, KEYS),
                                 cc.agg_desc(ROWID + ROWID))
        sc.same_agg(got, ar.agg_call(raws, SYNTH_ATTS, KEYS, ROWID + ROWID), ("agg", n))
        got = cc.group_blocks_call(L.cryo_multi_group_blocks, h, chk, method, comps, B, cc.filter_desc(SYNTH_ATTS, KEYS),
                                   cc.group_desc(ROWID), cc.agg_desc(ROWID))
        sc.same_group(got, gr.group_call(raws, SYNTH_ATTS, KEYS, ROWID, ROWID), ("group", n))


# ---- a region cut by the cap: two handles, five blocks, handle 1 holds blocks 1 and 3 behind handle 0's three ----
@pytest.mark.parametrize("method", METHODS)
def test_fetch_region_ends_at_the_cap(five, method):
    raws, comps, requests = five
    want = fe.multi_call(raws, requests, 2, B)
    start, packed = want[1][1]
    assert start == 3 * B and packed.size > 0 and want[2] == start + packed.size     # handle 1's share packs something
    cap = start + packed.size
    with handles(2) as m:
        same_fetch(fetch(m, method, comps[method], requests, cap), want, "the cap at the end of handle 1's bytes")
        big = np.full(5 * B + 64, SENTINEL, np.uint8)
        L, h, chk = m
        refused(lambda: cc.fetch_blocks_call(L.cryo_multi_fetch_blocks, h, chk, method, comps[method], B, requests, big[:cap - 8]),
                [(big, cap - 8)], "8 bytes less")


@pytest.mark.parametrize("method", METHODS)
def test_filter_regions_end_at_their_caps(five, method):
    raws, comps, _ = five
    want = fr.multi_call(raws, SYNTH_ATTS, KEYS, 2, B)
    b0, packed, r0, recs = want[1][1]
    assert (b0, r0) == (3 * B, 3 * 290) and packed.size > 0 and recs.size > 0      # handle 1's share packs bytes and records
    assert want[2] == (b0 + packed.size, r0 + recs.size)
    cap_b, cap_r = b0 + packed.size, r0 + recs.size
    with handles(2) as m:
        L, h, chk = m
        desc = cc.filter_desc(SYNTH_ATTS, KEYS)

        def short(dst_cap, rec_cap, what):
            big, big_rec = np.full(5 * B + 64, SENTINEL, np.uint8), np.full(5 * 290 + 8, sc.REC_SENTINEL, cc.FILTER_REC)
            refused(lambda: cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, method, comps[method], B, desc, big[:dst_cap],
                                                  big_rec[:rec_cap]), [(big, dst_cap), (big_rec, rec_cap)], what)
        same_filter(filter_(m, method, comps[method], dst_cap=cap_b), want, "the byte cap at the end of handle 1's bytes")
        short(cap_b - 8, 5 * 290, "8 bytes less")
        same_filter(filter_(m, method, comps[method], rec_cap=cap_r), want, "the record cap at the end of handle 1's records")
        short(5 * B, cap_r - 1, "one record less")
        same_filter(filter_(m, method, comps[method], cap_b, cap_r), want, "both caps at the ends")


@pytest.mark.parametrize("method", METHODS)
def test_project_regions_end_at_their_caps(five, method):
    raws, comps, _ = five
    want = pr.multi_call(raws, SYNTH_ATTS, KEYS, COLS, 2)
    first, rows, recs = want[1][1]
    assert first == 3 * 290 and rows.shape[0] > 0 and recs.size > rows.shape[0]     # handle 1's share packs rows, and more records
    assert want[2] == (first + rows.shape[0], first + recs.size)
    cap_w, cap_r = first + rows.shape[0], first + recs.size
    with handles(2) as m:
        L, h, chk = m
        desc, pdesc = cc.filter_desc(SYNTH_ATTS, KEYS), cc.project_desc(COLS)

        def short(row_cap, rec_cap, what):
            big = np.full((5 * 290 + 8, ROW_BYTES), SENTINEL, np.uint8)
            big_rec = np.full(8 * (5 * 290 + 8), SENTINEL, np.uint8).view(cc.PROJECT_REC)
            refused(lambda: cc.project_blocks_call(L.cryo_multi_project_blocks, h, chk, method, comps[method], B, desc, pdesc,
                                                   ROW_BYTES, big[:row_cap], big_rec[:rec_cap]),
                    [(big, row_cap), (big_rec, rec_cap)], what)
        same_project(project(m, method, comps[method], row_cap=cap_w), want, "the row cap at the end of handle 1's rows")
        short(cap_w - 1, 5 * 290, "one row less")
        same_project(project(m, method, comps[method], rec_cap=cap_r), want, "the record cap at the end of handle 1's records")
        short(5 * 290, cap_r - 1, "one record less")
        same_project(project(m, method, comps[method], cap_w, cap_r), want, "both caps at the ends")
