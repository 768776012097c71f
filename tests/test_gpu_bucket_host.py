"""GPU test of cryo_group_scan (host/group.h) with bucketed group columns through the SHIPPED host library: the real HIP codec
behind the walk, no test double, no test hook.  A mini-AM relation of 12 crafted blocks of 128 KiB, half LZ4 and half zstd, whose
ts column ascends in microseconds: grouped by the day of ts (a width) and by its month (a list of boundaries) beside a raw int2
column, over a range of ts that cuts through two blocks; every block's groups are compared with tests/bucket_ref.py."""
import ctypes as C

import numpy as np
import pytest

import bucket_ref as bk
import fetch_walk
import filter_ref as fr
import tuple_craft as tc
from pg_cryogen_amd import host

pytestmark = pytest.mark.gpu

ATTS = [(8, 8), (2, 2), (8, 8)]                         # (ts int8, g int2, x int8)
BY, COLS = [(1, fr.INT8), (2, fr.INT2)], [(3, fr.INT8), (1, fr.INT8)]
PER = 200
US_PER_DAY = 86_400_000_000
STEP = US_PER_DAY // 16                                 # 16 rows per day: a block spans 12.5 days
START = -40 * US_PER_DAY                                # days before and after the origin 2000-01-01


@pytest.fixture()
def HG():
    host.use(production=True)                  # libcryo_host.so: binds libcryo_codec.so on GPU 0, exports no hook
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops") and not hasattr(L, "cryo_host_set_group_ops")
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(131072)
    L.cryo_define_compression_gucs()
    L.cryo_cache_configure(16)
    yield L, errors
    L.cryo_cache_shutdown()
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)
    host.use(production=None)


def want_events(firsts, raws, keys, buckets):
    rows, recs, cells, _ = bk.group_call(raws, ATTS, keys, BY, COLS, buckets)
    out = []
    for k, row in enumerate(rows):
        gs = []
        for g in range(int(row["first_group"]), int(row["first_group"]) + int(row["n_groups"])):
            key = tuple(None if (int(recs["nulls"][g]) >> j) & 1 else int(recs["key"][g, j]) for j in range(2))
            gs.append((key, int(recs["n_rows"][g]),
                       [(int(c["n"]), int(c["min"]), int(c["max"]), (int(c["sum_hi"]) << 64) + int(c["sum_lo"])) for c in cells[g]]))
        out.append(("block", firsts[k], 500 + k, int(row["n_items"]), int(row["n_match"]), int(row["n_bad"]), gs))
    return out


def test_bucketed_group_scan_production_library(HG, oracle):
    L, errors = HG
    B, n = 131072, 12
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 4243, C.byref(rel))
    raws, firsts = [], []
    for k in range(n):
        ids = range(PER * k, PER * (k + 1))
        raws.append(tc.build_block(B, [tc.form_tuple(ATTS, [None if r % 37 == 0 else START + r * STEP, r % 3 - 1, r]) for r in ids]))
        method = host.COMP_ZSTD if k % 2 else host.COMP_LZ4
        comp = oracle.zstd_compress(raws[k], 1) if k % 2 else oracle.lz4_compress(raws[k], 1)
        firsts.append(fetch_walk.write_chain(L, mem, rel, method, 500 + k, comp)[0])
    lo, hi = START + (3 * PER + 50) * STEP, START + (9 * PER + 120) * STEP   # blocks 3 and 9 in part
    keys = [(1, fr.INT8, fr.GE, lo), (1, fr.INT8, fr.LT, hi)]
    day = [bk.width(0, US_PER_DAY), bk.RAW]
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS, buckets=day)
    want = want_events(firsts, raws, keys, day)
    assert events == want
    assert [e[4] for e in events][2:4] == [0, 150 - 4] and t["bad"] == 0 and t["codec_calls"] == 2   # four NULLs in block 3's part
    assert all(k[0] % US_PER_DAY == 0 for e in events for k, _, _ in e[6])            # every key is a day's start
    assert t["groups"] == sum(len(e[6]) for e in events) < t["matches"] // 3
    # months of 30 days as a list that starts inside the range: what lies below the first boundary is undecided
    months = [bk.bounds([m * 30 * US_PER_DAY for m in (2, 1, 3, 1)]), bk.RAW]
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS, buckets=months)
    want = want_events(firsts, raws, keys, months)
    assert events == want and t["bad"] == sum(e[5] for e in want) > 0 and t["matches"] == sum(e[4] for e in want)
    # without buckets the call is what it was: one group per distinct ts and g
    events, t = host.group_scan(rel, ATTS, keys, BY, COLS)
    assert events == want_events(firsts, raws, keys, [bk.RAW, bk.RAW]) and t["groups"] == t["matches"]
    assert not errors
