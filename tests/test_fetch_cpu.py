"""CPU tests of the tuple fetch: the rules (tests/fetch_ref.py) on the generator's blocks and on hand-made vectors, and
cryo_fetch_tuples (host/fetch.c) walking a mini-AM relation through the test build, with a codec double whose fetch_blocks
decodes with the oracle and answers by the rules."""
import ctypes as C
import struct

import numpy as np
import pytest

import fetch_ref as fr
import fetch_walk
from mini_am import load_relation
from pg_cryogen_amd import host

B128 = 131072
E_UNSUPPORTED, E_ARG = -6, -1


# ---- the rules ----
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_reference_on_generator_blocks(oracle, B):
    """distributions 0-3 hold 290 tuples per block at both sizes, `zeros` none: every position OK / NOITEM, and the bytes are
    the block sliced by its item ids"""
    for d in range(5):
        raw = oracle.synth(21, d, B, d)
        recs, packed, total = fr.fetch_call([raw], [list(range(1, 291))])
        if d == 4:
            assert (recs["status"] == fr.NOITEM).all() and total == 0 and (recs["off"] == 0).all()
            continue
        rows = fr.slice_by_items(raw)
        assert len(rows) == 290 and (recs["status"] == fr.OK).all()
        assert recs["len"].tolist() == [len(r) for r in rows]
        assert recs["off"].tolist() == np.concatenate([[0], np.cumsum([fr.maxalign(len(r)) for r in rows])[:-1]]).tolist()
        assert total == sum(fr.maxalign(len(r)) for r in rows) == packed.size
        for r, row in zip(recs, rows):
            o = int(r["off"])
            assert np.array_equal(packed[o:o + row.size], row) and not packed[o + row.size:o + fr.maxalign(row.size)].any()


def test_reference_on_hand_made_vectors():
    B = 4096
    lens = [1, 8, 9, 23, 24, 25, 100]
    b = fr.build_block(B, lens, pad=0xEE)
    rows = fr.slice_by_items(b)
    assert [r.size for r in rows] == lens
    upper = int(b[4:8].view("<u4")[0])
    assert (b[upper + 100:upper + 104] == 0xEE).all()                                # the pads of the block are not zero
    recs, packed, total = fr.fetch_call([b, None, b, b], [[1, 3, 8], [1, 2], [], [7]])
    assert recs["status"].tolist() == [fr.OK, fr.OK, fr.NOITEM, fr.STREAM, fr.STREAM, fr.OK]
    assert recs["len"].tolist() == [1, 9, 0, 0, 0, 100]
    assert recs["off"].tolist() == [0, 8, 24, 24, 24, 24] and total == 24 + 104      # a failed request carries the next offset
    assert packed[0] == rows[0][0] and not packed[1:8].any() and not packed[8 + 9:24].any() and not packed[124:].any()
    assert np.array_equal(packed[24:124], rows[6])
    # BADREQ: zero, duplicate, descending -- the whole block, its neighbours untouched
    for req in ([0, 1], [2, 2], [3, 2], [1, 2, 2, 5]):
        recs, _, total = fr.fetch_call([b, b], [req, [2]])
        assert recs["status"].tolist() == [fr.BADREQ] * len(req) + [fr.OK] and total == 8 and (recs["off"] == 0).all()
    # HEADER
    h = b.copy()
    h[0:4] = np.frombuffer(struct.pack("<I", 12), np.uint8)
    assert [s for s, _, _ in fr.fetch_block(h, [1, 2])] == [fr.HEADER, fr.HEADER]
    # ITEM: len 0, off not aligned, off below upper, beyond the block -- the request only
    for at, val in ((12, 0), (8, upper + 4), (8, upper - 8), (12, B)):
        x = b.copy()
        x[at:at + 4] = np.frombuffer(struct.pack("<I", val), np.uint8)
        assert [s for s, _, _ in fr.fetch_block(x, [1, 2])] == [fr.ITEM, fr.OK]
    # OVERLAP: items that all claim the same large tuple; a failed request keeps its own status
    big = (B - 8 - 8 * 4) // 2 + 64 & ~7
    o = np.zeros(B, np.uint8)
    for i in range(3):
        o[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", B - big, big), np.uint8)
    o[8 + 8 * 3:16 + 8 * 3] = np.frombuffer(struct.pack("<II", B - big, 0), np.uint8)
    o[:8] = np.frombuffer(struct.pack("<II", 8 + 8 * 4, B - big), np.uint8)
    assert [s for s, _, _ in fr.fetch_block(o, [1])] == [fr.OK]
    assert [s for s, _, _ in fr.fetch_block(o, [1, 2, 4, 5])] == [fr.OVERLAP, fr.OVERLAP, fr.ITEM, fr.NOITEM]
    recs, _, total = fr.fetch_call([o, b], [[1, 2], [1]])
    assert total == 8 and recs["off"].tolist() == [0, 0, 0]
    # several handles: block i -> handle i mod G, regions of B x (blocks dealt) bytes in handle order
    recs, regions, total = fr.multi_call([b, b, b, b, b], [[1], [2], [7], [], [3]], 2, B)
    assert [s for s, _ in regions] == [0, 3 * B] and recs["off"].tolist() == [0, 3 * B, 8, 8 + 104]
    assert total == 3 * B + 8


# ---- the walk, through a codec double ----
class FetchingDouble:
    """the oracle double of tests/codec_double.py plus a fetch table that decodes with the oracle and answers from fetch_ref"""

    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self._fetch = host.FETCH_BLOCKS_FN(self.fetch_blocks)
        self.fetch_ops = host.CryoCodecFetchOps(self._fetch)

    def fetch_blocks(self, ctx, method, srcs, sizes, n, bs, req_first, pos, dst, dst_cap, result, total):
        ora = self.base.ora
        blocks, requests = [], []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(fr.decode(ora, method, comp, bs))
            requests.append([pos[r] for r in range(req_first[i], req_first[i + 1])])
        self.calls.append((method, n, req_first[n]))
        recs, packed, tot = fr.fetch_call(blocks, requests)
        if tot > dst_cap:
            return -5
        if tot:
            C.memmove(dst, packed.ctypes.data, tot)
        if recs.size:
            C.memmove(result, recs.ctypes.data, recs.nbytes)
        total[0] = tot
        return 0


@pytest.fixture()
def HF():
    L = host.lib()
    dbl = FetchingDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_fetch_ops(C.byref(dbl.fetch_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_cache_shutdown()
    L.cryo_host_set_fetch_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


def _table(L):
    rows = [struct.pack("<i", i) for i in range(1, 2501)]                # 9 blocks of int4 rows, the last one partly filled
    return load_relation(L, rows, 1, host.COMP_LZ4, xid=777)


def test_fetch_tuples_walk_through_a_double(HF, oracle):
    L, dbl, errors = HF
    mem, rel, blocks, firsts = _table(L)
    pages, events, totals = fetch_walk.build(L, oracle, mem, rel, blocks, firsts, 777)
    t = fetch_walk.check(L, rel, pages, events, totals, calls=2)
    assert [(m, n) for m, n, _ in dbl.calls] == [(host.COMP_LZ4, totals["blocks"] - 1), (host.COMP_ZSTD, 1)]   # by method
    assert t["bytes_back"] < totals["blocks"] * B128 // 8
    # the rows are what was inserted: created_xid of the table, positions in order
    ids = [struct.unpack_from("<i", e[4], 24)[0] for e in events if e[0] == "tuple" and e[1] == firsts[1]]
    assert ids == list(range(291, 581)) and all(e[3] == 777 for e in events if e[0] == "tuple" and e[1] == firsts[1])
    # a frozen block is handed over with FrozenTransactionId, as the read path does
    L.cryo_memrel_set_frozen(mem, firsts[3], True)
    got, _ = host.fetch_tuples(rel, [(firsts[3], [2])])
    assert [(e[0], e[2], e[3]) for e in got] == [("tuple", 2, 2)]
    # no pages, and a page with TIDs but no offsets
    assert host.fetch_tuples(rel, [])[1]["pages"] == 0
    bad = host.CryoFetchPage(firsts[0], 3, None)
    assert L.cryo_fetch_tuples(C.byref(rel), C.byref(bad), 1, host.FETCH_TUPLE_FN(0), host.FETCH_REPORT_FN(0), None, None) == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_fetch_tuples_batches_by_window(HF, oracle):
    """more chains than one window holds (4 096): two codec calls, the tuples still in page order"""
    L, dbl, _ = HF
    host.set_block_size(4096)
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 77, C.byref(rel))
    firsts = []
    for k in range(3):                                                   # three distinct blocks, written 4 100 times in turn
        raw = fr.build_block(4096, [24 + 4] * 50, fill=lambda i, k=k: k * 50 + i + 1)
        comp = oracle.lz4_compress(raw, 1)
        firsts.append([fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 40 + k, comp)[0] for _ in range(4100 // 3 + 1)])
    order = sorted((f, k) for k in range(3) for f in firsts[k])[:4100]
    got, t = host.fetch_tuples(rel, [(f, [2, 50]) for f, _ in order])
    assert t["codec_calls"] == 2 and [n for _, n, _ in dbl.calls] == [4096, 4] and t["blocks"] == 4100 and t["bad"] == 0
    assert [(e[1], e[2], e[3], e[4][0]) for e in got] == [(f, p, 40 + k, k * 50 + p) for f, k in order for p in (2, 50)]
    L.cryo_memrel_destroy(mem)


def test_without_a_fetch_table_the_walk_is_unsupported(HF):
    L, dbl, _ = HF
    mem, rel, blocks, firsts = _table(L)
    L.cryo_host_set_fetch_ops(None)
    with pytest.raises(host.FetchTuplesError) as e:
        host.fetch_tuples(rel, [(firsts[0], [1])])
    assert e.value.code == E_UNSUPPORTED and e.value.events == [] and e.value.totals["pages"] == 0
    L.cryo_memrel_destroy(mem)
