"""GPU tests of the tuple walk that cryo_codec_filter_batch, _agg_batch, _group_batch and _project_batch share (csrc/filter_walk.h),
on the wide random tuples of tests/walk_gen.py: null bitmaps of up to 200 bytes, t_hoff up to 240, 1600 live columns, every fixed
width and alignment the argument rule admits, varlenas aligned to 8, busy header words, and one tuple cut to each of its lengths.

Every call is compared twice: with the by-construction expectation of walk_gen (computed from the rows the tuples were made from,
never from tuple bytes) and, field by field and byte by byte, with the Python reference applied to the same blocks.  The streams
are the oracle's; the outputs are filled with a sentinel before every call (tests/scan_calls.py): nothing at or beyond the totals
may be written, and the caller's key array must come back untouched.  Everything is integer-exact."""
import numpy as np
import pytest

import bytes_key_ref as br
import project_ref as pr
import walk_gen as wg
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc
from scan_calls import (REC_SENTINEL, SENTINEL, Encoder, agg_batch, agg_host, filter_batch, filter_host, group_batch, group_host,
                        multi_call, project_batch, project_host, same_agg, same_fields, same_filter, same_group, same_project)

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
KERNELS = ["filter", "agg", "group", "project"]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


def run(dev, enc, kernel, case, blks, plan, keysets, atts=None):
    """one kernel over the blocks for each key set and both methods: the reference's full output, computed once per key set, and
    the construction"""
    atts = atts or case.call_atts
    blocks = [b.data for b in blks]
    B = blocks[0].size
    for keys in keysets:
        what = (case.name, kernel, keys)
        if kernel == "filter":
            want = br.filter_call(blocks, atts, keys)
        elif kernel == "agg":
            want = br.agg_call(blocks, atts, keys, plan.agg_cols)
        elif kernel == "group":
            want = br.group_call(blocks, atts, keys, plan.by, plan.group_cols)
        else:
            want = pr.project_call(blocks, atts, keys, plan.project_cols)
        for method in METHODS:
            comps = [enc(method, b) for b in blocks]
            if kernel == "filter":
                got = filter_batch(dev, method, comps, B, atts, keys)
                same_filter(got, want, what)
                wg.check_filter(case, blks, keys, got, what)
            elif kernel == "agg":
                got = agg_batch(dev, method, comps, B, atts, keys, plan.agg_cols)
                same_agg(got, want, what)
                wg.check_agg(case, blks, keys, plan.agg_cols, got, what)
            elif kernel == "group":
                got = group_batch(dev, method, comps, B, atts, keys, plan.by, plan.group_cols)
                same_group(got, want, what)
                wg.check_group(case, blks, keys, plan.by, plan.group_cols, got, what)
            else:
                got = project_batch(dev, method, comps, B, atts, keys, plan.project_cols)
                same_project(got, want, what)
                wg.check_project(case, blks, keys, plan.project_cols, got, what)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", wg.NAMES)
def test_walk(dev, enc, name, kernel):
    """the case's blocks under key sets of 0, 4, 2, 3 and 1 integer keys and null tests: the aggregate captures four columns, the
    grouping two and four, the projection eight"""
    case = wg.case(name)
    run(dev, enc, kernel, case, case.blocks, case.plan, case.plan.keysets)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", wg.BYTES_NAMES)
def test_walk_with_byte_string_keys(dev, enc, name, kernel):
    """the byte-string instantiation: the key's text column lies beyond column 8, and in-line, compressed and external values
    stand in one block"""
    case = wg.case(name)
    assert case.plan.bytes_col > 8 and case.plan.bytes_keysets
    run(dev, enc, kernel, case, case.blocks, case.plan, case.plan.bytes_keysets)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", wg.SWEEP_NAMES)
def test_cut_sweep(dev, enc, name, kernel):
    """one tuple cut to each of its lengths (the tuple of 1600 columns: to 1 .. t_hoff + 64): TUPLE below `need`, from there on
    the uncut tuple's verdict and capture, and never a byte of the pad or of the neighbouring item"""
    case = wg.case(name)
    plan = case.sweep_plan()
    run(dev, enc, kernel, case, case.sweeps(), plan, [plan.keysets[0], plan.keysets[3]])


# ---- host buffers and several handles: the staging of a 40-column descriptor ----
def test_host_buffers_bitmap_edges(dev, enc):
    """one host-buffer call per kernel with all 40 columns of bitmap-edges in the descriptor"""
    case = wg.case("bitmap-edges")
    plan, atts, blks = case.plan, case.atts, case.blocks
    blocks, B, keys = [b.data for b in blks], case.B, case.plan.keysets[1]
    for method in METHODS:
        comps = [enc(method, b) for b in blocks]
        got = filter_host(dev, method, comps, B, atts, keys)
        same_filter(got, br.filter_call(blocks, atts, keys), method)
        wg.check_filter(case, blks, keys, got, method)
        got = agg_host(dev, method, comps, B, atts, keys, plan.agg_cols)
        same_agg(got, br.agg_call(blocks, atts, keys, plan.agg_cols), method)
        wg.check_agg(case, blks, keys, plan.agg_cols, got, method)
        got = group_host(dev, method, comps, B, atts, keys, plan.by, plan.group_cols)
        same_group(got, br.group_call(blocks, atts, keys, plan.by, plan.group_cols), method)
        wg.check_group(case, blks, keys, plan.by, plan.group_cols, got, method)
        got = project_host(dev, method, comps, B, atts, keys, plan.project_cols)
        same_project(got, pr.project_call(blocks, atts, keys, plan.project_cols), method)
        wg.check_project(case, blks, keys, plan.project_cols, got, method)


def test_two_handles_bitmap_edges(dev, enc):
    """cryo_multi_*_blocks on two handles of device 0, the same 40-column descriptor: every block's result is found through the
    table alone and equals the construction; nothing is written outside the regions' used parts"""
    case = wg.case("bitmap-edges")
    plan, atts, blks = case.plan, case.atts, case.blocks
    blocks, B, keys, n = [b.data for b in blks], case.B, case.plan.keysets[1], len(case.blocks)
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    f = cc.filter_desc(atts, keys)
    _, rb = pr.row_layout(atts, plan.project_cols)

    def calls(L, h, chk):
        return (cc.filter_blocks_call(L.cryo_multi_filter_blocks, h, chk, METHOD_ZSTD, comps, B, f, np.full(n * B, SENTINEL, np.uint8),
                                      np.full(n * 290, REC_SENTINEL, cc.FILTER_REC)),
                cc.agg_blocks_call(L.cryo_multi_agg_blocks, h, chk, METHOD_ZSTD, comps, B, f, cc.agg_desc(plan.agg_cols)),
                cc.group_blocks_call(L.cryo_multi_group_blocks, h, chk, METHOD_ZSTD, comps, B, f, cc.group_desc(plan.by),
                                     cc.agg_desc(plan.group_cols)),
                cc.project_blocks_call(L.cryo_multi_project_blocks, h, chk, METHOD_ZSTD, comps, B, f, cc.project_desc(plan.project_cols),
                                       rb, np.full((290 * n, rb), SENTINEL, np.uint8),
                                       np.full(8 * 290 * n, SENTINEL, np.uint8).view(cc.PROJECT_REC)))

    filt, agg, grp, prj = multi_call((0, 0), calls)
    table, recs, dst, total = filt
    etable, regions, etotal = br.multi_filter_call(blocks, atts, keys, 2, B)
    same_fields(table, etable, "filter")
    assert total == etotal
    wb, wr = np.zeros(dst.size, bool), np.zeros(recs.size, bool)
    for b0, packed, r0, rs in regions:
        assert np.array_equal(dst[b0:b0 + packed.size], packed) and np.array_equal(recs[r0:r0 + rs.size], rs)
        wb[b0:b0 + packed.size] = True
        wr[r0:r0 + rs.size] = True
    assert (dst[~wb] == SENTINEL).all() and (recs[~wr].view(np.uint8) == SENTINEL).all()
    wg.check_filter(case, blks, keys, filt, "two handles")
    same_agg(agg, br.agg_call(blocks, atts, keys, plan.agg_cols), "two handles")
    wg.check_agg(case, blks, keys, plan.agg_cols, agg, "two handles")
    same_group(grp, br.group_call(blocks, atts, keys, plan.by, plan.group_cols), "two handles")
    wg.check_group(case, blks, keys, plan.by, plan.group_cols, grp, "two handles")
    table, rec, rows, total = prj
    etable, regions, etotal = pr.multi_call(blocks, atts, keys, plan.project_cols, 2)
    assert total == etotal and table.tobytes() == etable.tobytes()
    used_w, used_r = np.zeros(rows.shape[0], bool), np.zeros(rec.size, bool)
    for first, erows, erecs in regions:
        assert rows[first:first + erows.shape[0]].tobytes() == erows.tobytes() and rec[first:first + erecs.size].tobytes() == erecs.tobytes()
        used_w[first:first + erows.shape[0]] = True
        used_r[first:first + erecs.size] = True
    assert (rows[~used_w] == SENTINEL).all() and (rec[~used_r].view(np.uint8) == SENTINEL).all()
    wg.check_project(case, blks, keys, plan.project_cols, prj, "two handles")
