"""GPU tests of the tuple walk in the newer block kernels and routes, on the wide random tuples of tests/walk_gen.py: the ordered
scan (ten capture slots, its own row assembly, rows of 8 .. 64 bytes), the text grouping (the capture carries an offset and a
length), the bucket grouping, and -- in all seven calls -- the float instantiation, the pattern units and set keys under a truth
table.  Null bitmaps of up to 200 bytes, 1600 columns, captures beyond bitmap byte 0, varlenas aligned to 8, a tuple cut to each
of its lengths, and blocks of more than 64 items.

Every call is compared twice, as tests/test_gpu_walk.py does: with the reference's full output, field by field and byte by byte,
and with the by-construction expectation of walk_gen, which reads no tuple.  The streams are the oracle's; the outputs are filled
with a sentinel before every call.  Integer- and byte-exact; a float cell is the reference's, bit for bit."""
import numpy as np
import pytest

import scan_calls
import topn_ref as tn
import truth_calls as tcall
import walk_gen as wg
import walk_routes as wr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, codec as cc
from scan_calls import SENTINEL, Encoder, same_agg, same_fields, same_filter, same_group, same_project
from topn_calls import same_multi, same_topn, topn_batch, topn_host, topn_multi

pytestmark = pytest.mark.gpu

METHODS = [METHOD_LZ4, METHOD_ZSTD]
ALL_NAMES = wg.NAMES + wg.NEW_NAMES
ROUTE_NAMES = ["bitmap-edges", "random-64", "bitmap-edges-dense", "max-columns"]


@pytest.fixture()
def dev(codec):
    yield codec
    codec.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


@pytest.fixture(scope="module")
def enc(oracle):
    return Encoder(oracle)


# ---- the grouped call with text columns or buckets, over any descriptor ----
def group_text_batch(codec, method, comps, B, atts, keys, by, cols, truth=None):
    """cryo_codec_group_batch under CRYO_GROUP_TEXT on device copies of everything: (rows, records, cells, total, key cells)"""
    n, nc = len(comps), len(cols)
    nt = sum(1 for _, typ in by if typ == wg.BYTES)
    cpg, cap = nc + nt, 290 * len(comps)
    with scan_calls.Device(codec, comps, atts, keys) as d:
        b, g = d.put(cc.group_desc(by)[1]), d.put(cc.agg_desc(cols)[1])
        rows, recs, cells, total = (d.alloc(32 * n + 64, SENTINEL), d.alloc(24 * cap + 64, SENTINEL),
                                    d.alloc(40 * cap * cpg + 64, SENTINEL), d.alloc(8, SENTINEL))
        codec.group_batch(method, d.src, d.off, d.sz, B, n, d.natts, d.atts, d.nkeys, d.keys if keys else None, len(by), b, nc,
                          g if nc else None, rows, recs, cap, cells if cpg else None, total, truth=truth, text=True)
        codec.sync()
        d.keys_untouched()
        r, q, c = rows.download(), recs.download(), cells.download()
        tot = int(total.download().view("<u8")[0])
        assert tot <= cap and (r[32 * n:] == SENTINEL).all() and (q[24 * tot:] == SENTINEL).all() and (c[40 * tot * cpg:] == SENTINEL).all()
        agg, key = cc.group_cells_split(c[:40 * tot * cpg].reshape(tot, cpg * 40), nc, nt)
        return r[:32 * n].view(cc.GROUP_BLOCK).copy(), q[:24 * tot].view(cc.GROUP_REC).copy(), agg, tot, key


def group_bucket_batch(codec, method, comps, B, atts, keys, by, cols, buckets, truth=None, shift=1):
    """cryo_codec_group_batch under CRYO_GROUP_BUCKETS on device copies of everything, the lists of boundaries at ptr + shift"""
    n, nc, cap = len(comps), len(cols), 290 * len(comps)
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
        r, q, c = rows.download(), recs.download(), cells.download()
        tot = int(total.download().view("<u8")[0])
        assert tot <= cap and (r[32 * n:] == SENTINEL).all() and (q[24 * tot:] == SENTINEL).all() and (c[40 * tot * nc:] == SENTINEL).all()
        return (r[:32 * n].view(cc.GROUP_BLOCK).copy(), q[:24 * tot].view(cc.GROUP_REC).copy(),
                c[:40 * tot * nc].view(cc.AGG_CELL).reshape(tot, nc).copy(), tot)


def same_text(got, want, what=""):
    assert len(got) == 5 and got[3] == want[3], (what, got[3], want[3])
    for j in (0, 1, 2, 4):
        same_fields(got[j], want[j], (what, j))


# ---- a call on the device, against its reference and the construction ----
def device_call(dev, method, comps, B, atts, call):
    kind, keys, truth, args = call
    if kind == "filter":
        return tcall.filter_batch(dev, method, comps, B, atts, keys, 0, truth)
    if kind == "agg":
        return tcall.agg_batch(dev, method, comps, B, atts, keys, args, truth)
    if kind == "group":
        return tcall.group_batch(dev, method, comps, B, atts, keys, *args, truth)
    if kind == "project":
        return tcall.project_batch(dev, method, comps, B, atts, keys, args, truth)
    if kind == "topn":
        return topn_batch(dev, method, comps, B, atts, keys, *args, truth=truth)
    if kind == "group_text":
        return group_text_batch(dev, method, comps, B, atts, keys, *args, truth)
    return group_bucket_batch(dev, method, comps, B, atts, keys, *args, truth)


def host_call(dev, method, comps, B, atts, call):
    kind, keys, truth, args = call
    if kind == "topn":
        return topn_host(dev, method, comps, B, atts, keys, *args, truth=truth)
    f = cc.filter_desc(atts, keys, 0, truth)
    if kind == "group_text":
        by, cols = args
        return dev.group_blocks(method, comps, B, f, cc.group_desc(by, text=True), cc.agg_desc(cols) if cols else None)
    by, cols, buckets = args
    return dev.group_blocks(method, comps, B, f, cc.group_desc(by), cc.agg_desc(cols) if cols else None, None, buckets=buckets)


SAME = {"filter": same_filter, "agg": same_agg, "group": same_group, "project": same_project, "topn": same_topn,
        "group_text": same_text, "group_bucket": same_group}
_wanted = {}


def wanted(case, blks, which, call, route):
    """the reference's result of a call, computed once: the cost of a test is the Python reference on wide tuples"""
    key = (case.name, which, route, repr(call))
    if key not in _wanted:
        _wanted[key] = wr.reference([b.data for b in blks], case.call_atts, call, route)
    return _wanted[key]


def run(dev, enc, case, blks, which, plan, kind, route, short=False, call_fn=device_call, methods=METHODS):
    """the calls of one kind under a route over the blocks, both methods: the reference's full output and the construction"""
    blocks, atts = [b.data for b in blks], case.call_atts
    B = blocks[0].size
    made = wr.calls(case, blks, plan, kind, route, short)
    assert made
    for call in made:
        want = wanted(case, blks, which, call, route)
        what = (case.name, route, call)
        for method in methods:
            comps = [enc(method, b) for b in blocks]
            got = call_fn(dev, method, comps, B, atts, call)
            SAME[kind](got, want, what)
            wr.check(case, blks, call, got, method)


NEW = [(name, kind) for name in ALL_NAMES for kind in wr.NEW_KINDS if wr.runs(wg.case(name).plan, kind, "plain")]


@pytest.mark.parametrize("name,kind", NEW)
def test_walk_new_kernels(dev, enc, name, kind):
    """the ordered scan under every order spec, column list (rows of 8 .. 64 bytes over the cases) and kind of limit; the text
    grouping by the text column alone, with an integer column and by a second text column; the bucket grouping under a width
    that sends the type's minimum below INT64_MIN, lists of boundaries on both sides of eight members and INFINITE: key sets of
    0, 4 and 3 integer keys and null tests.  A case without a text column has no text grouping"""
    case = wg.case(name)
    run(dev, enc, case, case.blocks, "blocks", case.plan, kind, "plain")


ROUTED = [(route, name, kind) for route in wr.ROUTES for name in ROUTE_NAMES for kind in wr.KINDS
          if wr.runs(wg.case(name).plan, kind, route)]


@pytest.mark.parametrize("route,name,kind", ROUTED)
def test_walk_routes(dev, enc, route, name, kind):
    """all seven calls under the float route (float keys, a float aggregate column, float order columns), the pattern route
    and the table route (set keys on both sides of eight members; a truth table over an integer key, a set key, a byte-string
    key and a null test).  max-columns has no text column: no pattern route, no text grouping, an integer key for the
    byte-string key"""
    case = wg.case(name)
    run(dev, enc, case, case.blocks, "blocks", case.plan, kind, route)


SWEEPS = [(name, kind, "plain") for name in wg.SWEEP_NAMES for kind in wr.NEW_KINDS if kind != "group_text" or name != "max-columns"]
SWEEPS += [("bitmap-edges", "topn", "like"), ("bitmap-edges", "topn", "float")]


@pytest.mark.parametrize("name,kind,route", SWEEPS)
def test_cut_sweep_new_kernels(dev, enc, name, kind, route):
    """one tuple cut to each of its lengths: TUPLE below `need` -- from the highest of the key, order, group and projected
    columns --, from there on the uncut tuple's verdict, keys and row"""
    case = wg.case(name)
    run(dev, enc, case, case.sweeps(), "sweeps", case.sweep_plan(), kind, route, short=True)


# ---- host buffers and two handles: the staging of the ten-slot table ----
def test_host_buffers_bitmap_edges(dev, enc):
    """one host-buffer call of each new kernel on the 34 columns of bitmap-edges"""
    case = wg.case("bitmap-edges")
    for kind in wr.NEW_KINDS:
        run(dev, enc, case, case.blocks, "blocks", case.plan, kind, "plain", short=True, call_fn=host_call)


def test_two_handles_topn_bitmap_edges(enc):
    """cryo_multi_topn_blocks on two handles of device 0: every block's rows are found through the table alone and equal the
    construction; nothing is written outside the regions' used parts"""
    case = wg.case("bitmap-edges")
    plan, atts, blks = case.plan, case.call_atts, case.blocks
    blocks, keys = [b.data for b in blks], plan.keysets[1]
    by, cols, limit = plan.topn_by[1], plan.topn_cols[-1], 5
    comps = [enc(METHOD_ZSTD, b) for b in blocks]
    got = topn_multi(2, METHOD_ZSTD, comps, case.B, atts, keys, by, limit, cols)
    same_multi(got, tn.multi_call(blocks, atts, keys, by, limit, cols, 2), limit, "two handles")
    table, rec, rows, _ = got
    wg.check_topn(case, blks, keys, by, limit, cols, (table, rec, rows, int(table["n_rows"].sum())), "two handles")
