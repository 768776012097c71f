"""GPU tests of the truth table over scan keys on the host side: cryo_filter_scan, cryo_aggregate_scan, cryo_group_scan and
cryo_project_scan (host/filter.h, aggregate.h, group.h, project.h) through the SHIPPED host library -- the real HIP codec behind
the walks, no test double, no test hook -- over a small relation with a descriptor that ORs a set key with a range, against
tests/truth_key_ref.py."""
import ctypes as C

import pytest

import fetch_walk
import truth_key_ref as tr
import tuple_craft as tc
from pg_cryogen_amd import codec, host

pytestmark = pytest.mark.gpu

ATTS = [(4, 4), (-1, 4), (8, 8), (2, 2)]                  # (rowid int4, text, x int8, app int2)
PER, B, N = 150, 131072, 6
# WHERE rowid >= 100 AND (app IN (3, 17) OR x <= -3 * 860 OR tag = 'www'): four keys, A AND (B OR C OR D)
KEYS = [(1, tr.INT4, tr.GE, 100), (4, tr.INT2, tr.IN, [3, 17, 3]), (3, tr.INT8, tr.LE, -3 * 860), (2, tr.BYTES, tr.EQ, b"www")]
TABLE = codec.truth_dnf([0b0011, 0b0101, 0b1001], 4)
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


def test_the_four_scans_with_an_or(HP, oracle):
    L, errors = HP
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4646, C.byref(rel))
    raws, firsts = make_blocks(), []
    for k in range(N):
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD if k % 2 else host.COMP_LZ4, 500 + k, comp)[0])
    assert TABLE == tr.dnf([0b0011, 0b0101, 0b1001], 4) and tr.table_ok(TABLE, 4)
    rows = [r for r in range(100, PER * N) if (r % 19 and r % 43 - 2 in (3, 17)) or r >= 860 or r % 60 == 3]
    by_app, by_x, by_tag = ([r for r in rows if c(r)] for c in (lambda r: r % 19 and r % 43 - 2 in (3, 17), lambda r: r >= 860, lambda r: r % 60 == 3))
    assert by_app and by_x and by_tag and len(rows) < len(by_app) + len(by_x) + len(by_tag)     # every term finds rows, and they overlap
    assert any(r % 43 - 2 in (3, 17) for r in range(100)) and any(r % 60 == 3 for r in range(100))        # the AND excludes some
    # the filter: the matching tuples in scan order
    events, t = host.filter_scan(rel, ATTS, KEYS, truth=TABLE)
    want = tr.filter_call(raws, ATTS, KEYS, 0, TABLE)
    assert [int.from_bytes(e[4][24:28], "little") for e in events if e[0] == "tuple"] == rows
    assert [(e[1], e[2]) for e in events if e[0] == "tuple"] == [(firsts[r // PER], r % PER + 1) for r in rows]
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"]) == (N, N * PER, int(want[0]["n_match"].sum()), 0, 0)
    events, c = host.filter_scan(rel, ATTS, KEYS, tr.COUNT_ONLY, TABLE)
    assert events == [] and c["matches"] == len(rows)
    # without the table the same keys are ANDed
    events, t = host.filter_scan(rel, ATTS, KEYS, tr.COUNT_ONLY)
    assert t["matches"] == len([r for r in rows if r in by_app and r in by_x and r in by_tag])
    # the aggregate: per-block counts and the cells added up
    events, t = host.aggregate_scan(rel, ATTS, KEYS, [(3, tr.INT8), (1, tr.INT4)], truth=TABLE)
    arows, _ = tr.agg_call(raws, ATTS, KEYS, [(3, tr.INT8), (1, tr.INT4)], TABLE)
    assert [(e[3], e[4], e[5]) for e in events if e[0] == "block"] == [(int(r["n_items"]), int(r["n_match"]), int(r["n_bad"])) for r in arows]
    assert t["cells"][0] == (len(rows), -3 * rows[-1], -3 * rows[0], -3 * sum(rows)) and t["cells"][1] == (len(rows), rows[0], rows[-1], sum(rows))
    # the grouped scan by the set key's column
    events, t = host.group_scan(rel, ATTS, KEYS, [(4, tr.INT2)], [(1, tr.INT4)], truth=TABLE)
    grows, grecs, _, total = tr.group_call(raws, ATTS, KEYS, [(4, tr.INT2)], [(1, tr.INT4)], TABLE)
    assert (t["matches"], t["groups"], t["bad"]) == (len(rows), total, 0)
    assert [g[0] for e in events if e[0] == "block" for g in e[6]] == [(None if n & 1 else int(k[0]),) for k, n in zip(grecs["key"], grecs["nulls"])]
    # the projection
    events, t = host.project_scan(rel, ATTS, KEYS, COLS, truth=TABLE)
    wanted = []
    for k in range(N):
        table, recs, out, _ = tr.project_call([raws[k]], ATTS, KEYS, COLS, TABLE)
        wanted += [("row", firsts[k], int(r["pos"]), 500 + k, int(r["nulls"]), bytes(out[i])) for i, r in enumerate(recs)]
    assert events == wanted and len(events) == len(rows)
    # a table that is no AND/OR tree is refused through every walk
    with pytest.raises(host.FilterScanError) as e:
        host.filter_scan(rel, ATTS, KEYS, truth=TABLE ^ (1 << 15))
    assert e.value.code == -1
    assert not errors
    L.cryo_memrel_destroy(mem)
