"""The relation-level scenario of the tuple-fetch tests (cryo_fetch_tuples, host/fetch.h), shared by the CPU test (codec
double) and the GPU test (shipped host library): a mini-AM table plus a few hand-written chains, the pages of a TID bitmap over
it, and what the walk must deliver -- taken from the access method's own read path (cryo_read_data + cryo_storage_fetch) and,
for the damaged blocks, from tests/fetch_ref.py.  Test infrastructure only."""
import ctypes as C
import struct

import numpy as np

import fetch_ref as fr
from pg_cryogen_amd import host

CHAIN, METHOD = host.CRYO_CHECK_CHAIN, host.CRYO_CHECK_METHOD


def write_chain(L, mem, rel, method, xid, comp):
    first = L.cryo_memrel_reserve(mem)
    chain, npages = (C.c_uint32 * 256)(), C.c_int()
    comp = np.ascontiguousarray(comp)
    assert L.cryo_stage_write_chain(C.byref(rel), first, method, xid, comp.ctypes.data, comp.nbytes, chain, 256,
                                    C.byref(npages)) == 0
    return first, list(chain)[:npages.value]


def read_path_tuples(L, rel, first, positions):
    """[(pos, created_xid, tuple bytes)] through the decompressed-block cache: cryo_read_data + cryo_storage_fetch"""
    e = C.c_int(-1)
    assert L.cryo_read_data(C.byref(rel), None, first, C.byref(e)) == host.CRYO_ERR_SUCCESS
    data, xid = L.cryo_cache_get_data(e.value), L.cryo_cache_get_xid(e.value)
    n = L.cryo_storage_ntuples(data)
    out = []
    ht = host.HeapTupleData()
    for pos in (range(1, n + 1) if positions is None else positions):
        L.cryo_storage_fetch(data, pos, C.byref(ht))
        out.append((pos, xid, C.string_at(ht.t_data, ht.t_len)))
    return out


def build(L, oracle, mem, rel, blocks, firsts, table_xid):
    """adds the hand-written chains and returns (pages, expected events, expected totals but for codec_calls / bytes_back).
    Needs a table of at least 6 blocks whose last block is not full."""
    B = host.get_block_size()
    raw = lambda i: np.frombuffer(blocks[i], np.uint8)          # noqa: E731
    # a zstd block among the LZ4 ones: a second codec call
    z_first, _ = write_chain(L, mem, rel, host.COMP_ZSTD, 902, oracle.zstd_compress(raw(1), 1))
    # a block with a damaged item (len 0 at position 5)
    bad = raw(2).copy()
    bad[12 + 8 * 4:16 + 8 * 4] = 0
    item_first, _ = write_chain(L, mem, rel, host.COMP_LZ4, 901, oracle.lz4_compress(bad, 1))
    # a multi-page chain of incompressible bytes: its second page is no chain start; the block itself has no valid header
    noise = np.random.default_rng(5).integers(0, 256, B, dtype=np.uint8)
    noise_first, noise_chain = write_chain(L, mem, rel, host.COMP_LZ4, 903, oracle.lz4_compress(noise, 1))
    assert len(noise_chain) > 1
    # a chain whose first page promises more bytes than the chain holds: unreadable
    short_first, _ = write_chain(L, mem, rel, host.COMP_LZ4, 904, oracle.lz4_compress(raw(0), 1))
    # a chain that names a method nobody knows
    odd_first, _ = write_chain(L, mem, rel, host.COMP_LZ4, 905, oracle.lz4_compress(raw(0), 1))
    # a stream the decoders reject
    dead_first, _ = write_chain(L, mem, rel, host.COMP_LZ4, 906, oracle.lz4_compress(raw(3), 1))
    empty = L.cryo_memrel_reserve(mem)                            # a new page, never written

    # what the access method's own read path hands out for the same TIDs -- read before any page is damaged
    last = len(firsts) - 1
    n_last = len(fr.slice_by_items(raw(last)))
    assert last >= 6 and 0 < n_last < 290
    asks = [(firsts[0], [1, 5, 290]), (firsts[1], None), (firsts[3], [2]), (firsts[4], list(range(7, 291, 7))),
            (firsts[5], [289, 290, 291]), (firsts[last], None), (z_first, [3, 4, 288])]
    want = [read_path_tuples(L, rel, first, None if positions is None else [p for p in positions if p <= 290])
            for first, positions in asks]
    assert len(want[1]) == 290 and len(want[5]) == n_last
    L.cryo_cache_invalidate_relation(rel.relid)

    def item_row(p):
        off, ln = struct.unpack_from("<II", bad, 8 + 8 * (p - 1))
        return bad[off:off + ln].tobytes()

    # the damage goes straight into the relation's pages
    page = L.cryo_memrel_page(mem, short_first)
    csize = struct.unpack_from("<I", C.string_at(page, 64), 40)[0]
    C.memmove(page + 40, struct.pack("<I", csize + 100000), 4)
    C.memmove(L.cryo_memrel_page(mem, odd_first) + 36, struct.pack("<i", 9), 4)
    C.memset(L.cryo_memrel_page(mem, dead_first) + 48, 0xFF, 64)

    def tup(first, pos, xid, data):
        return ("tuple", first, pos, xid, data + bytes(-len(data) % 8), len(data))

    def tuples(k):
        return [tup(asks[k][0], pos, xid, data) for pos, xid, data in want[k]]

    pages, events, sent = [], [], []
    pages.append((0, [1])); not_starts = 1                                # the page before the first chain
    for k in range(3):                                                    # exact; lossy over a full block; (below) one TID
        if k == 2:
            pages.append((firsts[2], []))                                 # an exact page without TIDs: counted, not read
        pages.append(asks[k]); sent.append(asks[k]); events += tuples(k)
    pages.append(asks[3]); sent.append(asks[3]); events += tuples(3)      # every 7th
    pages.append(asks[4]); sent.append(asks[4]); events += tuples(4)      # a position beyond the last item: reported
    events.append(("report", firsts[5], fr.NOITEM, 291))
    pages.append(asks[5]); sent.append(asks[5]); events += tuples(5)      # lossy over a partly filled block: its n tuples
    pages.append(asks[6]); sent.append(asks[6]); events += tuples(6)      # zstd
    pages.append((item_first, [4, 5, 6])); sent.append(pages[-1])
    events += [tup(item_first, 4, 901, item_row(4)), ("report", item_first, fr.ITEM, 5), tup(item_first, 6, 901, item_row(6))]
    assert fr.fetch_block(noise, [1])[0][0] == fr.HEADER
    pages.append((noise_first, None)); sent.append(pages[-1]); events.append(("report", noise_first, fr.HEADER, 1))
    pages.append((noise_chain[1], None)); not_starts += 1                 # a continuation page
    pages.append((short_first, [1])); events.append(("report", short_first, CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED))
    pages.append((odd_first, None)); events.append(("report", odd_first, METHOD, 9))
    pages.append((dead_first, [1, 2, 3])); sent.append(pages[-1]); events.append(("report", dead_first, fr.STREAM, 1))
    pages.append((empty, None)); not_starts += 1
    assert [p[0] for p in pages] == sorted(p[0] for p in pages)
    tuple_bytes = sum((e[5] + 7) & ~7 for e in events if e[0] == "tuple")
    totals = {"pages": len(pages), "not_block_starts": not_starts, "blocks": len(sent),
              "tuples": sum(1 for e in events if e[0] == "tuple"), "bad": sum(1 for e in events if e[0] == "report"),
              "bytes_back": tuple_bytes + 16 * sum(290 if p is None else len(p) for _, p in sent)}
    return pages, events, totals


def check(L, rel, pages, events, totals, calls):
    """runs the walk and compares; returns its totals"""
    before = (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls())
    got, t = host.fetch_tuples(rel, pages)
    assert (L.cryo_cache_hits(), L.cryo_cache_misses(), L.cryo_cache_codec_calls()) == before   # the cache is not touched
    assert len(got) == len(events), (len(got), len(events), [e for e in got if e[0] == "report"])
    for g, e in zip(got, events):
        assert g == e, (g[:4], e[:4])
    for k, v in totals.items():
        assert t[k] == v, (k, t[k], v)
    assert t["codec_calls"] == calls
    return t
