"""The ordered scan's routes in the table of tests/workspace_routes.py.

That table holds one route or more per entry point include/cryo_codec.h declares, and tests/test_gpu_workspace_history.py runs all of
them over a handle whose buffers were filled with hostile bytes, in seeded orders and after failed calls; its coverage test fails
for an entry point without a route.  cryo_codec_topn_batch and cryo_codec_topn_blocks get theirs here: importing this module adds
the group "scan_topn" to the table -- GROUPS and the method Table._scan_topn, exactly where a group lives -- so that every run
that collects the suite finds the routes in place before a test starts.  Nothing of the table is changed or removed.

  test_the_routes_are_in_the_table   (no GPU) the group is registered once, in front of the pool's, and names the two entry points
  test_routes_after_a_fill           the routes of this group alone, after a fill of every handle-owned buffer with each of four
                                     values: what test_filled_workspace does for the whole table, for a run of this file alone"""
import pytest

import float_cases as fc
import float_ref as fl
import oracle_lib
import topn_calls
import topn_ref
import workspace_routes as wr
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, Codec, codec as cc

GROUP = "scan_topn"
FILLS = (0x00, 0xFF, 0x01, 0xA5)


def _scan_topn(self):
    """cryo_codec_topn_batch / _blocks on the scans' streams: integer keys and the mixed keys under their truth table, ordered by an
    int8 and an int4 column or by the float8 column, whole and with one block per chunk; the side area (rows, records, order list)
    and the kernel's table lie in the workspace a fill has written"""
    atts, B = fc.ATTS, 4096
    dec_by_method = {m: self.stored(m, B) for m in (METHOD_LZ4, METHOD_ZSTD)}
    dec = dec_by_method[METHOD_LZ4][1]
    for mixed, by, limit in ((False, [(6, fl.INT8, topn_ref.DESC), (1, fl.INT4, topn_ref.NULLS_FIRST)], 7),
                             (True, [(2, fl.FLOAT8, topn_ref.DESC | topn_ref.NULLS_FIRST)], 300)):
        keys, W = (self.MIX_KEYS, self.MIX_TRUTH) if mixed else (self.INT_KEYS, None)
        want = topn_ref.topn_call(dec, atts, keys, by, limit, self.PCOLS, W)
        assert want[3] > 0 and {0, 1, 2} <= set(want[0]["status"].tolist()), mixed
        for opts in ({}, {cc.OPT_WORKSPACE_MAX_BYTES: 1}):
            for method in (METHOD_LZ4, METHOD_ZSTD):
                comps = dec_by_method[method][0]
                for host in (False, True):
                    chunk = 1 if opts else len(comps)
                    buf = ("d_vfy",) + (wr.HOST_IN if host else (("d_keytab",) if mixed else ()))
                    buf += ("d_ws",) if method == METHOD_ZSTD else wr.lz4_ws(B, chunk)
                    tag = "%s method %d %s%s" % ("host" if host else "device", method, "mixed keys" if mixed else "integer keys",
                                                 ", chunked" if opts else "")
                    fn = topn_calls.topn_host if host else topn_calls.topn_batch

                    def run(c, fn=fn, method=method, comps=comps, keys=keys, by=by, limit=limit, W=W):
                        return fn(c, method, comps, B, atts, keys, by, limit, self.PCOLS, truth=W)

                    def check(got, state, what, w=want):
                        topn_calls.same_topn(got, w, what)
                    yield wr.Route(GROUP, tag, run, check, "cryo_codec_topn_%s" % ("blocks" if host else "batch"), buf, opts)


def install():
    """the group into the table, once: in front of the pool's group, whose routes stay the last"""
    if GROUP not in wr.GROUPS:
        wr.GROUPS.insert(wr.GROUPS.index("pool"), GROUP)
        wr.Table._scan_topn = _scan_topn


install()


@pytest.fixture(scope="module")
def table(oracle):
    stock = oracle_lib.StockLibs()
    if stock.zstd is None:
        pytest.fail("libzstd.so.1 is needed by the table's other groups")
    return wr.Table(oracle, stock)


def test_the_routes_are_in_the_table(table):
    assert wr.GROUPS.count(GROUP) == 1 and wr.GROUPS[-1] == "pool"
    routes = table.group(GROUP)
    assert len(routes) == 16 and len({r.name for r in routes}) == 16
    assert set().union(*(r.entry for r in routes)) == {"cryo_codec_topn_batch", "cryo_codec_topn_blocks"} <= wr.header_entry_points()
    assert {r.host for r in routes} == {False, True} and sum(1 for r in routes if r.options) == 8


@pytest.mark.gpu
def test_routes_after_a_fill(table):
    with Codec(0) as c:
        for r in table.group(GROUP):
            r.go(c, "sizing run")
            before = None
            for value in FILLS:
                report = c.debug_fill(value)
                empty = [b for b in r.buffers if report[b] == 0]
                assert not empty, (r.name, "a buffer the route uses was not there to be filled", empty)
                assert before is None or report == before, (r.name, "a buffer grew in the run: it was not the filled one")
                before = report
                r.go(c, "after a fill with 0x%02X" % value)
