"""GPU tests of the set scan keys on the host side: cryo_filter_scan, cryo_aggregate_scan, cryo_group_scan and cryo_project_scan
(host/filter.h, aggregate.h, group.h, project.h) through the SHIPPED host library -- the real HIP codec behind the walks, no test
double, no test hook -- over a small relation with an IN list and a NOT IN list, against tests/set_key_ref.py."""
import ctypes as C

import pytest

import fetch_walk
import set_key_ref as sr
import tuple_craft as tc
from pg_cryogen_amd import host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4), (8, 8), (2, 2)]                  # (rowid int4, text, x int8, app int2)
PER, B, N = 150, 131072, 6
APPS = [3, 17, 40, 17, -2, 33000, 1 << 40]                # 33 000 and 2^40 are no int2: they equal no value
KEYS = [(4, sr.INT2, sr.IN, APPS), (1, sr.INT4, sr.GE, 100), (3, sr.INT8, sr.NOT_IN, [-3 * r for r in range(0, 900, 40)] + [7] * 50)]
COLS = [3, 4, 1]                                          # widths 8, 2, 4: offsets 0, 8, 12; 16 bytes


def make_blocks():
    return [tc.build_block(B, [tc.form_tuple(ATTS, [r, b"w" * (r % 60), -3 * r, None if r % 19 == 0 else r % 43 - 2])
                               for r in range(PER * k, PER * (k + 1))]) for k in range(N)]


@pytest.fixture()
def HP():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_filter_ops")
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B)
    L.cryo_define_compression_gucs()
    L.cryo_cache_configure(16)
    yield L, errors
    L.cryo_cache_shutdown()
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)
    host.use(production=None)


def test_the_four_scans_with_a_set_key(HP, oracle):
    L, errors = HP
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4545, C.byref(rel))
    raws, firsts = make_blocks(), []
    for k in range(N):
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
    rows = [r for r in range(100, PER * N) if r % 19 and r % 43 - 2 in (3, 17, 40, -2) and r % 40]
    assert len(rows) > 60 and any(r % 43 - 2 == -2 for r in rows) and any(r % 40 == 0 and r % 43 - 2 in APPS for r in range(100, PER * N))
    # the filter: the matching tuples in scan order
    events, t = host.filter_scan(rel, ATTS, KEYS)
    want = sr.filter_call(raws, ATTS, KEYS)
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == rows
    assert [(e[1], e[2]) for e in events if e[0] == "tuple"] == [(firsts[r // PER], r % PER + 1) for r in rows]
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"]) == (N, N * PER, int(want[0]["n_match"].sum()), 0, 0)
    events, c = host.filter_scan(rel, ATTS, KEYS, sr.COUNT_ONLY)
    assert events == [] and c["matches"] == len(rows)
    # the aggregate: per-block counts and the cells added up
    events, t = host.aggregate_scan(rel, ATTS, KEYS, [(3, sr.INT8), (4, sr.INT2)])
    arows, _ = sr.agg_call(raws, ATTS, KEYS, [(3, sr.INT8), (4, sr.INT2)])
    assert [(e[3], e[4], e[5]) for e in events if e[0] == "block"] == [(int(r["n_items"]), int(r["n_match"]), int(r["n_bad"])) for r in arows]
    apps = [r % 43 - 2 for r in rows]
    assert t["cells"][0] == (len(rows), -3 * rows[-1], -3 * rows[0], -3 * sum(rows)) and t["cells"][1] == (len(rows), -2, 40, sum(apps))
    # the grouped scan by the set key's own column
    events, t = host.group_scan(rel, ATTS, KEYS, [(4, sr.INT2)], [(1, sr.INT4)])
    grows, grecs, _, total = sr.group_call(raws, ATTS, KEYS, [(4, sr.INT2)], [(1, sr.INT4)])
    assert (t["matches"], t["groups"], t["bad"]) == (len(rows), total, 0)
    assert [g[0] for e in events if e[0] == "block" for g in e[6]] == [(int(k[0]),) for k in grecs["key"]]
    assert {int(k[0]) for k in grecs["key"]} == {3, 17, 40, -2}
    # the projection: the set key's column among the projected ones
    events, t = host.project_scan(rel, ATTS, KEYS, COLS)
    wanted = []
    for k in range(N):
        table, recs, out, _ = sr.project_call([raws[k]], ATTS, KEYS, COLS)
        wanted += [("row", firsts[k], int(r["pos"]), 500 + k, int(r["nulls"]), bytes(out[i])) for i, r in enumerate(recs)]
    assert events == wanted and len(events) == len(rows)
    assert not errors
    L.cryo_memrel_destroy(mem)
