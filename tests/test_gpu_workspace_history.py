"""No call may depend on what the handle's workspace held before it.

A handle's device and pinned buffers are grow-only, never cleared, and shared between very different calls ("Workspace
rules"): a kernel that reads a region another kernel of the same call did not write passes as long as its call is the one that
allocates the buffer -- fresh device memory is zero -- and fails in a long-lived backend.  The session-wide handle of conftest.py
gives every other GPU test whatever the tests before it left; here the history is controlled:

  test_filled_workspace   every route of tests/workspace_routes.py runs once, so that the buffers have their size, and then after
                          cryo_codec_debug_fill has filled every handle-owned buffer with 0x00, 0xFF (all-ones flags and "done"
                          bits), 0x01 (plausible small 8-, 16- and 32-bit indices and counts) and 0xA5; every output is compared
                          with the oracle or the Python references each time.  The fill must have covered the buffers the route
                          is known to use, and no buffer may have grown in a run: a regrown buffer was not the poisoned one
  test_real_histories     the whole table in three seeded orders on one handle without any fill, a cryo_codec_trim and one switch
                          of CRYO_OPT_WORKSPACE_KEEP_BYTES to 0 and back at seeded points: what the routes leave for each other
  test_after_failed_calls batches of rejected streams and refused calls, then a route of every entry point in every group
  test_route_table_covers_the_options_and_entry_points   (no GPU) a route added to the library without an entry here fails it; the
                          entry points are read from the header, the option values are a list kept by hand, which
  test_path_option_values_are_the_librarys               holds against what cryo_codec_set_option takes and refuses
  test_caps_cut_the_calls_as_the_routes_assume           the tiled and the chunked routes rest on how the planners answer a
                          workspace cap of one byte: tiles of 16 frames on one lane, one block per chunk; a planner that
                          answers otherwise fails here instead of quietly turning those routes into one-tile, one-chunk calls

The handle is this module's own, so that the shared one's history is not disturbed."""
import random

import pytest

import oracle_lib
import workspace_routes as wr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, Codec, CryoError, codec as cc

FILLS = (0x00, 0xFF, 0x01, 0xA5)
ORDERS = (20261, 20262, 20263)


@pytest.fixture(scope="module")
def table(oracle):
    stock = oracle_lib.StockLibs()
    if stock.zstd is None:
        pytest.fail("libzstd.so.1 is needed to write the checksummed and the non-default frames")
    return wr.Table(oracle, stock)


@pytest.fixture(scope="module")
def hist():
    c = Codec(0)
    yield c
    c.close()


def test_route_table_covers_the_options_and_entry_points(table):
    routes = table.all()
    assert len({(r.group, r.name) for r in routes}) == len(routes), "two routes of one name"
    for opt, values in wr.PATH_OPTIONS.items():
        seen = {r.path_options()[opt] for r in routes}
        assert set(values) <= seen, ("option %d: no route runs under" % opt, sorted(set(values) - seen))
    declared = wr.header_entry_points()
    assert len(declared) >= 21 and "cryo_codec_decompress_blocks_keyed" in declared and "cryo_codec_verify_batch" in declared, declared
    called = set().union(*(r.entry for r in routes))
    assert declared <= called, ("entry points without a route", sorted(declared - called))
    assert called <= declared, ("routes name entry points the header does not declare", sorted(called - declared))
    known = set(wr.FILL_KEYS)
    assert all(set(r.buffers) <= known for r in routes)
    used = set().union(*(r.buffers for r in routes))
    assert used == known, ("buffers no route is known to use", known - used)


@pytest.mark.gpu
def test_path_option_values_are_the_librarys(hist):
    for opt, values in wr.PATH_OPTIONS.items():
        taken = []
        for v in range(-2, 12):
            try:
                hist.set_option(opt, v)
                taken.append(v)
            except CryoError as e:
                assert e.code == cc.E_ARG, (opt, v, e)
        hist.set_option(opt, 0)
        assert tuple(taken) == tuple(values), ("option %d takes other values than the route table knows" % opt, taken, values)


@pytest.mark.gpu
def test_caps_cut_the_calls_as_the_routes_assume(table):
    """On fresh handles, so that a buffer's capacity is what the one call asked for.  Tiles: the workspace of the 304-frame
    route under the cap is exactly that of a 16-frame call (one tile of the planner's smallest size, one lane: 19 tiles for
    the route), and less than the same 304 frames take without a cap (much of a tile is of fixed size).  Chunks: under the cap a check of eight blocks holds in d_vfy what a check of one
    block holds (a chunk of one block), less than without the cap"""
    def ws(make, fill_key):
        with Codec(0) as c:
            make(c)
            return c.debug_fill(0)[fill_key]
    tiled = table.group("zstd_decode_tiles")[0]
    comps, want = table.once(("zstd", 4096, 304), None)
    sixteen = [c for c, w in zip(comps, want) if w is not None][:16]
    cap = {cc.OPT_ZSTD_DECODE_PATH: 2, cc.OPT_WORKSPACE_MAX_BYTES: 1}

    def few(c, opts):
        for o, v in opts.items():
            c.set_option(o, v)
        wr.decompress_batch(c, METHOD_ZSTD, sixteen, 4096)
    capped, one_tile = ws(lambda c: tiled.go(c), "d_ws"), ws(lambda c: few(c, cap), "d_ws")
    free = ws(lambda c: wr.decompress_batch(c, METHOD_ZSTD, comps, 4096), "d_ws")
    assert capped == one_tile and capped < free, (capped, one_tile, free)
    for method in (METHOD_LZ4, METHOD_ZSTD):
        streams, _ = table.stored(method, 32768)

        def check(c, part, capped_):
            c.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 1 if capped_ else 0)
            c.check_blocks(method, part, 32768)
        eight, one = ws(lambda c: check(c, streams, True), "d_vfy"), ws(lambda c: check(c, streams[:1], True), "d_vfy")
        whole = ws(lambda c: check(c, streams, False), "d_vfy")
        assert eight == one and eight < whole, (method, eight, one, whole)


@pytest.mark.gpu
@pytest.mark.parametrize("group", wr.GROUPS)
def test_filled_workspace(hist, table, group):
    own = []
    try:
        for r in table.group(group):
            c = hist
            if r.own_handle:
                c = Codec(0)
                own.append(c)
            r.go(c, "sizing run")
            before = None
            for value in FILLS:
                report = c.debug_fill(value)
                assert set(report) == set(wr.FILL_KEYS)
                empty = [b for b in r.buffers if report[b] == 0]
                assert not empty, (r.group, r.name, "a buffer the route uses was not there to be filled", empty)
                assert before is None or report == before, (r.group, r.name, "a buffer grew in the run: it was not the filled one",
                                                            {k: (before[k], report[k]) for k in report if report[k] != before[k]})
                before = report
                r.go(c, "after a fill with 0x%02X" % value)
            report = c.debug_fill(0)
            assert report == before, (r.group, r.name, "a buffer grew in the last run", {k: (before[k], report[k]) for k in report if report[k] != before[k]})
    finally:
        for c in own:
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ORDERS)
def test_real_histories(hist, table, seed):
    routes = list(table.all())
    rng = random.Random(seed)
    rng.shuffle(routes)
    trim_at = rng.randrange(len(routes))
    keep_at = rng.choice([i for i, r in enumerate(routes) if r.host])       # only the host-buffer calls trim when they return
    for i, r in enumerate(routes):
        if i == trim_at:
            hist.trim()
        if i == keep_at:
            hist.set_option(cc.OPT_WORKSPACE_KEEP_BYTES, 0)     # the host-buffer calls give their buffers back when they return
        try:
            r.go(hist, ("order %d, route %d" % (seed, i), [q.name for q in routes[max(0, i - 3):i]]))
        finally:
            if i == keep_at:
                hist.set_option(cc.OPT_WORKSPACE_KEEP_BYTES, -1)


@pytest.mark.gpu
def test_after_failed_calls(hist, table, oracle):
    chosen = wr.one_route_per_kind(table)
    assert set().union(*(r.entry for r in chosen)) == wr.header_entry_points() and {r.group for r in chosen} == set(wr.GROUPS)
    for r in chosen:
        wr.failing_calls(hist, oracle)
        r.go(hist, "after rejected batches and refused calls")
