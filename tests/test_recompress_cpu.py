"""CPU tests of recompression: the packing rules (tests/recode_ref.py) on hand-made vectors, and cryo_recompress_relation
(host/recompress.c) walking mini-AM relations through the test build, with a codec double whose recode_blocks decodes with the
oracle, encodes with the oracle and packs by the rule."""
import ctypes as C
import struct

import numpy as np
import pytest

import recode_ref as rr
from pg_cryogen_amd import host

B128 = 131072
STREAM, NONE = 1, 0xFFFFFFFF
E_CORRUPT, E_UNSUPPORTED, E_VERIFY = -4, -6, -8


# ---- the packing rules ----
def test_packing_reference_on_hand_made_vectors():
    assert rr.pack_offsets([], []) == ([], [], 0)
    assert rr.pack_offsets([1], [0]) == ([1], [0], 16)                                   # one block
    assert rr.pack_offsets([17], [0], base=64) == ([17], [64], 32)
    assert rr.pack_offsets([16, 32, 48], [0, 0, 0]) == ([16, 32, 48], [0, 16, 48], 96)   # multiples of 16: no pad
    assert rr.pack_offsets([5, 0, 33, 0, 0, 16], [0, 0, 0, 0, 0, 0]) == ([5, 0, 33, 0, 0, 16], [0, 16, 16, 64, 64, 64], 80)
    # a failed block has size 0 whatever its encoder wrote, takes no room, and leaves its neighbours where they would be
    assert rr.pack_offsets([100, 999, 7], [0, -4, 0]) == ([100, 0, 7], [0, 112, 112], 128)
    assert rr.pack_offsets([9, 9, 9], [-4, -8, -4]) == ([0, 0, 0], [0, 0, 0], 0)         # all failed
    dst = np.full(64, 0xEE, np.uint8)
    sizes, offs, total = rr.pack_buffer([np.arange(1, 6, dtype=np.uint8), None, np.full(17, 9, np.uint8)], [0, -4, 0], dst)
    assert (sizes, offs, total) == ([5, 0, 17], [0, 16, 16], 48)
    assert dst[:5].tolist() == [1, 2, 3, 4, 5] and (dst[5:16] == 0).all() and (dst[16:33] == 9).all()
    assert (dst[33:48] == 0).all() and (dst[48:] == 0xEE).all()                           # zero pads, untouched tail
    # several handles: block i -> handle i mod G, each share packed from its region's start
    sizes, offs, region = rr.multi_offsets([10, 20, 30, 40, 50], [0, 0, -4, 0, 0], 2, 1000 + 8)
    assert region == 496 and sizes == [10, 20, 0, 40, 50] and offs == [0, 496, 16, 496 + 32, 16]
    sizes, offs, region = rr.multi_offsets([10, 20, 30, 40], [0] * 4, 3, 3 * 64)
    assert region == 64 and offs == [0, 64, 128, 16]


# ---- the codec double ----
class RecodingDouble:
    """the oracle double of tests/codec_double.py in the layout that carries recode_blocks"""

    def __init__(self, with_recode=True):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self.fail_verify = set()        # compressed sizes of source streams whose new stream "fails write verification"
        self._recode = host.RECODE_BLOCKS_FN(self.recode_blocks)
        self.ops = host.CryoCodecOpsRecode(self.base._bound, self.base._comp, self.base._decomp, None)
        if with_recode:
            self.ops.recode_blocks = C.cast(self._recode, C.c_void_p)

    def recode_blocks(self, ctx, src_method, srcs, sizes, n, bs, dst_method, dst_param, dst, dst_cap, out_off, out_size, status):
        ora = self.base.ora
        self.calls.append((src_method, n))
        streams, st = [], []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            r, raw = (ora.lz4_decompress if src_method == 0 else ora.zstd_decompress)(comp, bs)
            if r != bs:
                streams.append(None); st.append(E_CORRUPT)
                continue
            if sizes[i] in self.fail_verify:
                streams.append(None); st.append(E_VERIFY)
                continue
            streams.append(ora.lz4_compress(raw, dst_param) if dst_method == 0 else ora.zstd_compress(raw, dst_param))
            st.append(0)
        szs, offs, total = rr.pack_offsets([0 if s is None else len(s) for s in streams], st)
        if total > dst_cap:
            return -5
        area = np.ctypeslib.as_array(C.cast(dst, C.POINTER(C.c_uint8)), (max(total, 1),))
        rr.pack_buffer(streams, st, area)
        for i in range(n):
            out_off[i], out_size[i], status[i] = offs[i], szs[i], st[i]
        return 0


@pytest.fixture()
def HR():
    L = host.lib()
    dbl = RecodingDouble()
    L.cryo_host_set_codec_ops(C.cast(C.byref(dbl.ops), C.POINTER(host.CryoCodecOps)))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_cache_shutdown()
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


def _new_rel(L, relid):
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, relid, C.byref(rel))
    return mem, rel


def _write_at(L, rel, first, method, xid, comp):
    chain, npages = (C.c_uint32 * 64)(), C.c_int()
    assert L.cryo_stage_write_chain(C.byref(rel), first, method, xid, comp.ctypes.data, comp.nbytes, chain, 64,
                                    C.byref(npages)) == 0
    return list(chain)[:npages.value]


def _poke(L, mem, b, at, data):
    C.memmove(L.cryo_memrel_page(mem, b) + at, data, len(data))


def _scan(L, mem, rel):
    """the relation in sequential-scan order: [(first page, method, xid, compressed bytes, chain)]"""
    it = L.cryo_seqscan_iter_create()
    out = []
    while True:
        b = L.cryo_seqscan_iter_next(it)
        if b == host.InvalidBlockNumber or b >= L.cryo_memrel_nblocks(mem):
            break
        comp, csize, method, xid = C.c_void_p(), C.c_size_t(), C.c_int(), C.c_uint32()
        chain, n = (C.c_uint32 * 64)(), C.c_uint32()
        err = L.cryo_stage_read_chain(C.byref(rel), b, C.byref(comp), C.byref(csize), C.byref(method), C.byref(xid), chain, 64,
                                      C.byref(n))
        if err == host.CRYO_ERR_EMPTY_BLOCK:
            continue
        assert err == host.CRYO_ERR_SUCCESS, (b, err)
        for p in list(chain)[1:n.value]:
            L.cryo_seqscan_iter_exclude(it, p, True)
        out.append((b, method.value, xid.value, np.ctypeslib.as_array(C.cast(comp, C.POINTER(C.c_uint8)), (csize.value,)).copy(),
                    list(chain)[:n.value]))
    L.cryo_seqscan_iter_free(it)
    return out


def _build(L, oracle, mem, rel, count=12):
    """LZ4 and zstd blocks mixed, chains of one and of many pages, two pairs of interleaved chains, empty pages;
    returns [(first, method, xid, raw, compressed, chain)] in scan order"""
    enc = {host.COMP_LZ4: lambda r: oracle.lz4_compress(r, 1), host.COMP_ZSTD: lambda r: oracle.zstd_compress(r, 1)}
    blocks = []
    k = 0
    while k < count:
        pair = 2 if k in (2, 7) else 1                       # blocks 2+3 and 7+8: first pages reserved before either is written
        todo = []
        for _ in range(pair):
            method = host.COMP_LZ4 if k % 3 else host.COMP_ZSTD
            raw = oracle.synth(8, k, B128, (1, 2, 3, 0)[k % 4])   # `random` and `wide` rows: chains of many pages
            todo.append((L.cryo_memrel_reserve(mem), method, 700 + k, raw, enc[method](raw)))
            k += 1
        for first, method, xid, raw, comp in todo:
            blocks.append((first, method, xid, raw, comp, _write_at(L, rel, first, method, xid, comp)))
        if k in (4, 9):
            L.cryo_memrel_reserve(mem)                       # reserved, never written
    return blocks


def test_recompress_relation_mixed_methods(HR, oracle):
    L, dbl, errors = HR
    mem, rel = _new_rel(L, 41)
    dmem, dst = _new_rel(L, 42)
    try:
        blocks = _build(L, oracle, mem, rel)
        assert {len(b[5]) for b in blocks} >= {1} and max(len(b[5]) for b in blocks) > 4
        assert blocks[2][5][1] > blocks[3][0]                # interleaved: block 2's second page lies behind block 3's first
        assert {b[1] for b in blocks} == {host.COMP_LZ4, host.COMP_ZSTD}
        assert [b[0] for b in blocks] == sorted(b[0] for b in blocks)
        moved, reports, totals = host.recompress_relation(rel, dst, host.COMP_ZSTD, 3)
        assert reports == [] and not errors
        got = _scan(L, dmem, dst)
        # the same decoded blocks in the same order, each under the target method with its source's xid
        assert len(got) == len(blocks)
        for (first, method, xid, comp, chain), (_, _, sxid, raw, _, _) in zip(got, blocks):
            assert method == host.COMP_ZSTD and xid == sxid
            r, out = oracle.zstd_decompress(comp, B128)
            assert r == B128 and np.array_equal(out, raw)
            assert np.array_equal(comp, oracle.zstd_compress(raw, 3))
        # the map: complete, in order, page counts those of cryo_pages_needed
        assert [m[0] for m in moved] == [b[0] for b in blocks]
        assert [m[1] for m in moved] == [g[0] for g in got]
        assert [m[2] for m in moved] == [len(b[5]) for b in blocks]
        assert [m[3] for m in moved] == [L.cryo_pages_needed(len(g[3])) for g in got] == [len(g[4]) for g in got]
        assert totals == {"blocks": 12, "recoded": 12, "verbatim": 0, "skipped": 0, "empty_pages": 2,
                          "bytes_in": sum(len(b[4]) for b in blocks), "bytes_out": sum(len(g[3]) for g in got),
                          "pages_in": sum(len(b[5]) for b in blocks), "pages_out": sum(len(g[4]) for g in got), "codec_calls": 2}
        assert L.cryo_memrel_nblocks(dmem) == 1 + totals["pages_out"]
        # one window: one call per source method present, not one per block
        assert sorted(dbl.calls) == sorted([(host.COMP_LZ4, sum(b[1] == host.COMP_LZ4 for b in blocks)),
                                            (host.COMP_ZSTD, sum(b[1] == host.COMP_ZSTD for b in blocks))])
        assert L.cryo_cache_hits() == 0 and L.cryo_cache_misses() == 0 and L.cryo_cache_codec_calls() == 0
        # a level change within one method, back to LZ4
        d2mem, d2 = _new_rel(L, 43)
        try:
            moved2, reports2, totals2 = host.recompress_relation(dst, d2, host.COMP_LZ4, 1)
            got2 = _scan(L, d2mem, d2)
            assert reports2 == [] and totals2["recoded"] == 12 and totals2["codec_calls"] == 1
            for (_, method, xid, comp, _), b in zip(got2, blocks):
                assert method == host.COMP_LZ4 and xid == b[2] and np.array_equal(comp, oracle.lz4_compress(b[3], 1))
        finally:
            L.cryo_memrel_destroy(d2mem)
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def test_windows_bound_the_codec_calls(HR, oracle):
    """4 100 small LZ4 blocks: a window of 4 096 and one of 4, a call each"""
    L, dbl, errors = HR
    host.set_block_size(8192)
    mem, rel = _new_rel(L, 44)
    dmem, dst = _new_rel(L, 45)
    try:
        comps = [oracle.lz4_compress(oracle.synth(9, k, 8192, 1 + k % 2), 1) for k in range(20)]
        n = 4100
        for k in range(n):
            _write_at(L, rel, L.cryo_memrel_reserve(mem), host.COMP_LZ4, 777, comps[k % 20])
        moved, reports, totals = host.recompress_relation(rel, dst, host.COMP_LZ4, 9)
        assert reports == [] and not errors
        assert dbl.calls == [(host.COMP_LZ4, 4096), (host.COMP_LZ4, 4)] and totals["codec_calls"] == 2
        assert totals["blocks"] == n and totals["recoded"] == n and len(moved) == n
        assert [m[0] for m in moved] == list(range(1, n + 1)) and [m[1] for m in moved] == list(range(1, n + 1))
    finally:
        host.set_block_size(B128)
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def test_bad_input_is_reported_never_lost(HR, oracle):
    L, dbl, errors = HR
    mem, rel = _new_rel(L, 46)
    dmem, dst = _new_rel(L, 47)
    try:
        blocks = _build(L, oracle, mem, rel)
        # a flipped stream byte (the zstd frame's magic number): the decoders reject the stream
        flipped = next(i for i, b in enumerate(blocks) if b[1] == host.COMP_ZSTD and i > 0)
        first = blocks[flipped][0]
        _poke(L, mem, first, 48, bytes([C.string_at(L.cryo_memrel_page(mem, first) + 48, 1)[0] ^ 0xFF]))
        # a chain cut short: compressed_size beyond what the chain holds
        cut = next(i for i, b in enumerate(blocks) if len(b[5]) > 1 and i != flipped)
        first = blocks[cut][0]
        csize = struct.unpack("<I", C.string_at(L.cryo_memrel_page(mem, first) + 40, 4))[0]
        _poke(L, mem, first, 40, struct.pack("<I", csize + 20000))
        # a method field of 7
        odd = next(i for i, b in enumerate(blocks) if i not in (flipped, cut) and i > 0)
        _poke(L, mem, blocks[odd][0], 36, struct.pack("<i", 7))
        moved, reports, totals = host.recompress_relation(rel, dst, host.COMP_ZSTD, 1)
        want = sorted([(blocks[flipped][0], STREAM, NONE, len(blocks[flipped][5])),
                       (blocks[cut][0], host.CRYO_CHECK_CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED, len(blocks[cut][5])),
                       (blocks[odd][0], host.CRYO_CHECK_METHOD, 7, len(blocks[odd][5]))])
        assert reports == want and not errors
        assert totals["blocks"] == 12 and totals["recoded"] == 9 and totals["verbatim"] == 1 and totals["skipped"] == 2
        assert totals["codec_calls"] == 2 and sum(n for _, n in dbl.calls) == 10
        kept = [b for i, b in enumerate(blocks) if i not in (cut, odd)]
        got = _scan(L, dmem, dst)
        assert [m[0] for m in moved] == [b[0] for b in kept] and len(got) == len(kept)
        for (_, method, xid, comp, _), b in zip(got, kept):
            assert xid == b[2]
            if b[0] == blocks[flipped][0]:                   # verbatim: the same bytes under the same method field
                damaged = b[4].copy()
                damaged[0] ^= 0xFF
                assert method == b[1] and np.array_equal(comp, damaged)
            else:                                            # its neighbours are recoded
                assert method == host.COMP_ZSTD and np.array_equal(comp, oracle.zstd_compress(b[3], 1))
        assert totals["bytes_in"] == sum(len(b[4]) for b in kept) and totals["bytes_out"] == sum(len(g[3]) for g in got)
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def test_failed_verification_keeps_the_block_as_it_was(HR, oracle):
    """a block whose new stream fails write verification (CRYO_E_VERIFY from the codec) is copied verbatim and reported with
    CRYO_CHECK_STREAM, offset = the status as uint32; its neighbours are recoded"""
    L, dbl, errors = HR
    mem, rel = _new_rel(L, 53)
    dmem, dst = _new_rel(L, 54)
    try:
        blocks = _build(L, oracle, mem, rel, count=6)
        victim = 4
        assert sum(len(b[4]) == len(blocks[victim][4]) for b in blocks) == 1
        dbl.fail_verify.add(len(blocks[victim][4]))
        moved, reports, totals = host.recompress_relation(rel, dst, host.COMP_ZSTD, 1)
        assert reports == [(blocks[victim][0], STREAM, E_VERIFY & 0xFFFFFFFF, len(blocks[victim][5]))] and not errors
        assert totals["recoded"] == 5 and totals["verbatim"] == 1 and totals["skipped"] == 0 and len(moved) == 6
        got = _scan(L, dmem, dst)
        for i, ((_, method, xid, comp, _), b) in enumerate(zip(got, blocks)):
            assert xid == b[2]
            if i == victim:
                assert method == b[1] and np.array_equal(comp, b[4])
            else:
                assert method == host.COMP_ZSTD and np.array_equal(comp, oracle.zstd_compress(b[3], 1))
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def test_needs_recode_blocks_and_a_known_target(HR, oracle):
    L, _, errors = HR
    dbl = RecodingDouble(with_recode=False)
    L.cryo_host_set_codec_ops(C.cast(C.byref(dbl.ops), C.POINTER(host.CryoCodecOps)))
    mem, rel = _new_rel(L, 48)
    dmem, dst = _new_rel(L, 49)
    try:
        _build(L, oracle, mem, rel, count=3)
        with pytest.raises(host.RecompressRelationError) as e:
            host.recompress_relation(rel, dst, host.COMP_ZSTD, 1)
        assert e.value.code == E_UNSUPPORTED
        assert L.cryo_memrel_nblocks(dmem) == 1 and dbl.calls == []          # dst untouched
        with pytest.raises(host.RecompressRelationError) as e:
            host.recompress_relation(rel, dst, 7, 1)
        assert e.value.code == -1 and L.cryo_memrel_nblocks(dmem) == 1
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def test_empty_relation(HR):
    L, dbl, _ = HR
    mem, rel = _new_rel(L, 50)
    dmem, dst = _new_rel(L, 51)
    try:
        moved, reports, totals = host.recompress_relation(rel, dst, host.COMP_LZ4, 1)
        assert moved == [] and reports == [] and set(totals.values()) == {0} and dbl.calls == []
        assert L.cryo_memrel_nblocks(dmem) == 1
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_memrel_destroy(dmem)


def test_old_layout_double_still_passes_the_check(oracle):
    """a double of the layout that ends with check_blocks (existing tests build such ones) never has recode_blocks read"""
    from test_check_cpu import CheckingDouble
    L = host.lib()
    dbl = CheckingDouble()
    assert C.sizeof(dbl.ops) == C.sizeof(host.CryoCodecOpsRecode) - 8
    L.cryo_host_set_codec_ops(C.byref(dbl.ops))
    host.set_block_size(B128)
    mem, rel = _new_rel(L, 52)
    try:
        for k in range(4):
            comp = oracle.lz4_compress(oracle.synth(8, k, B128, 1 + k % 2), 1)
            _write_at(L, rel, L.cryo_memrel_reserve(mem), host.COMP_LZ4, 777, comp)
        reports, totals = host.check_relation(rel)
        assert reports == [] and totals == {"blocks": 4, "empty_pages": 0, "bad": 0, "codec_calls": 1}
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_host_set_codec_ops(None)
        host.set_block_size(1 << 20)
