"""CPU tests of the stored-block check: the layout rules of tests/layout_ref.py on valid and hand-corrupted blocks, and
cryo_check_relation (host/check.c) walking a mini-AM relation through the test build, with a codec double whose check_blocks
decodes with the oracle and checks with layout_ref."""
import ctypes as C
import struct

import numpy as np
import pytest

import layout_ref as ref
from pg_cryogen_amd import host
from mini_am import pack_rows

B128 = 131072


# ---- the rules ----
@pytest.mark.parametrize("B", [4096, B128, 1 << 20])
@pytest.mark.parametrize("dist", range(5))
def test_synth_blocks_pass(oracle, B, dist):
    for k in range(3):
        blk = oracle.synth(3, k, B, dist)
        if B == 4096 and dist in (0, 3):
            # wide / random rows sized so that 290 of them fill the block are 0 bytes long at 4 KiB: the generator's
            # degenerate case, no block cryo_storage_insert can write (a tuple has a 23-byte header)
            assert ref.check_block(blk) == (ref.ITEM, 8)
            continue
        assert ref.check_block(blk) == (ref.OK, ref.NONE)


def test_storage_insert_blocks_pass(oracle):
    L = host.lib()
    for bs, rows in ((B128, [struct.pack("<i", i) for i in range(1, 1001)]),
                     (B128, [bytes(range(i % 97)) * 3 for i in range(700)]),
                     (8192, [b"x" * (i % 29 + 1) for i in range(300)])):
        host.set_block_size(bs)
        try:
            blocks = pack_rows(L, rows, 1, bs)
        finally:
            host.set_block_size(1 << 20)
        assert len(blocks) >= 2
        for b in blocks:
            assert ref.check_block(np.frombuffer(b, np.uint8)) == (ref.OK, ref.NONE)


def _block(oracle, dist=1, B=8192):
    return np.array(oracle.synth(1, 0, B, dist), np.uint8)


def _put(b, at, v):
    b[at:at + 4] = np.frombuffer(struct.pack("<I", v & 0xFFFFFFFF), np.uint8)


def test_each_rule_fails_with_its_offset(oracle):
    b0 = _block(oracle)                  # narrow rows at 8 KiB: t_len 61, slots of 64, pads of 3
    B = b0.size
    lower, upper = (int(x) for x in b0[:8].view("<u4"))
    n = (lower - 8) // 8
    assert ref.check_block(b0) == (ref.OK, ref.NONE) and n > 3
    cases = []
    for v in (0, 4, 7, lower + 4, upper + 8):                   # lower out of range
        b = b0.copy(); _put(b, 0, v); cases.append((b, (ref.HEADER, 0)))
    for v in (lower - 8, B + 8, B + 1):                          # upper out of range
        b = b0.copy(); _put(b, 4, v); cases.append((b, (ref.HEADER, 0)))
    b = np.zeros(B, np.uint8); _put(b, 0, 8 + 8 * 291); _put(b, 4, B); cases.append((b, (ref.HEADER, 0)))   # n = 291
    b = np.zeros(B, np.uint8); _put(b, 0, 8); _put(b, 4, B - 8); cases.append((b, (ref.HEADER, 0)))         # n = 0, upper != B
    b = b0.copy(); _put(b, 12 + 8 * 2, 0); cases.append((b, (ref.ITEM, 8 + 8 * 2)))                          # a zero len
    for i in (0, n // 2, n - 1):                                 # a broken slot chain
        b = b0.copy(); _put(b, 8 + 8 * i, int(b[8 + 8 * i:12 + 8 * i].view("<u4")[0]) - 8)
        cases.append((b, (ref.ITEM, 8 + 8 * i)))
    b = b0.copy(); _put(b, 4, upper + 64)                        # the last item no longer starts at upper
    cases.append((b, (ref.ITEM, 8 + 8 * (n - 1))))
    b = b0.copy(); _put(b, 12, 0); _put(b, 12 + 8 * 3, 0); cases.append((b, (ref.ITEM, 8)))  # the lowest failing item
    b = b0.copy(); b[upper - 1] = 1; cases.append((b, (ref.NONZERO, upper - 1)))            # a gap byte
    b = b0.copy(); b[lower] = 1; b[upper - 1] = 1; cases.append((b, (ref.NONZERO, lower)))
    off0 = int(b0[8:12].view("<u4")[0])
    b = b0.copy(); b[off0 + 62] = 9; cases.append((b, (ref.NONZERO, off0 + 62)))            # a pad byte of item 0
    b = b0.copy(); b[off0 + 62] = 9; b[upper + 63] = 1                                      # item n-1's pad is lower
    cases.append((b, (ref.NONZERO, upper + 63)))
    b = b0.copy(); b[off0 + 62] = 9; _put(b, 12 + 8 * 5, 0); cases.append((b, (ref.ITEM, 8 + 8 * 5)))      # ITEM wins
    b = b0.copy(); b[off0 + 10] ^= 0xFF; cases.append((b, (ref.OK, ref.NONE)))              # a tuple body byte: not seen
    for b, want in cases:
        assert ref.check_block(b) == want


# ---- cryo_check_relation with a codec double ----
class CheckingDouble:
    """the oracle double of tests/codec_double.py plus check_blocks: decode with the oracle, check with layout_ref"""

    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self._check = host.CHECK_BLOCKS_FN(self.check_blocks)
        self.ops = host.CryoCodecOpsCheck(self.base._bound, self.base._comp, self.base._decomp, None)
        self.ops.check_blocks = C.cast(self._check, C.c_void_p)

    def check_blocks(self, ctx, method, srcs, sizes, n, bs, result):
        self.calls.append((method, n))
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            reason, offset = ref.check_stream(self.base.ora, method, comp, bs)
            result[2 * i], result[2 * i + 1] = reason, offset
        return 0


@pytest.fixture()
def HC():
    L = host.lib()
    dbl = CheckingDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.ops))
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


def _write(L, rel, mem, method, comp):
    first = L.cryo_memrel_reserve(mem)
    chain, npages = (C.c_uint32 * 64)(), C.c_int()
    assert L.cryo_stage_write_chain(C.byref(rel), first, method, 777, comp.ctypes.data, comp.nbytes, chain, 64,
                                    C.byref(npages)) == 0
    return first, list(chain)[:npages.value]


def _poke(L, mem, b, at, data):
    C.memmove(L.cryo_memrel_page(mem, b) + at, data, len(data))


def test_check_relation_reports(HC, oracle):
    L, dbl, errors = HC
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 31, C.byref(rel))
    enc = {host.COMP_LZ4: lambda r: oracle.lz4_compress(r, 1), host.COMP_ZSTD: lambda r: oracle.zstd_compress(r, 1)}
    blocks = {}   # first page -> (method, chain pages)
    expect = []
    try:
        for k in range(12):
            method = host.COMP_LZ4 if k % 3 else host.COMP_ZSTD
            dist = (1, 2, 3, 0)[k % 4]                   # `random` rows: chains of many pages
            raw = oracle.synth(8, k, B128, dist)
            if k == 4:
                raw = raw.copy(); raw[9000] = 0x20       # a gap byte
                expect.append(("b", k, ref.NONZERO, 9000))
            if k == 7:
                raw = raw.copy(); _put(raw, 12 + 8 * 40, 0)
                expect.append(("b", k, ref.ITEM, 8 + 8 * 40))
            first, chain = _write(L, rel, mem, method, enc[method](raw))
            blocks[k] = (first, method, chain)
            if k in (2, 5):
                L.cryo_memrel_reserve(mem)               # reserved, never written: skipped like a scan skips it
        assert len(blocks[3][2]) > 1 and len(blocks[11][2]) > 1
        # a chain cut short: compressed_size beyond what the chain holds
        first, _, chain = blocks[3]
        csize = struct.unpack("<I", C.string_at(L.cryo_memrel_page(mem, first) + 40, 4))[0]
        _poke(L, mem, first, 40, struct.pack("<I", csize + 20000))
        expect.append(("b", 3, host.CRYO_CHECK_CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED))
        # an orphan continuation page: a page that names another page as its chain's start
        orphan = L.cryo_memrel_reserve(mem)
        _poke(L, mem, orphan, 14, struct.pack("<H", 8192))
        _poke(L, mem, orphan, 24, struct.pack("<II", blocks[0][0], 0xFFFFFFFF))
        expect.append(("p", orphan, host.CRYO_CHECK_CHAIN, host.CRYO_ERR_WRONG_STARTING_BLOCK, 0))
        # a method byte of 7
        _poke(L, mem, blocks[8][0], 36, struct.pack("<i", 7))
        expect.append(("b", 8, host.CRYO_CHECK_METHOD, 7))
        # a payload byte flipped so that the stream is rejected (the zstd frame's magic number)
        first = blocks[9][0]
        assert blocks[9][1] == host.COMP_ZSTD
        _poke(L, mem, first, 48, bytes([C.string_at(L.cryo_memrel_page(mem, first) + 48, 1)[0] ^ 0xFF]))
        expect.append(("b", 9, ref.STREAM, ref.NONE))
        want = []
        for e in expect:
            if e[0] == "p":
                want.append(e[1:])
            else:
                first, _, chain = blocks[e[1]]
                want.append((first, e[2], e[3], len(chain)))
        reports, totals = host.check_relation(rel)
        assert reports == sorted(want)
        assert [r[0] for r in reports] == sorted(r[0] for r in reports)
        assert totals == {"blocks": 13, "empty_pages": 2, "bad": 6, "codec_calls": 2}
        assert sorted(m for m, _ in dbl.calls) == [host.COMP_LZ4, host.COMP_ZSTD]
        assert sum(n for _, n in dbl.calls) == 10        # 12 chains, less the cut one and the method-7 one
        assert not errors
        # the walk neither reads through the cache nor fills it
        assert L.cryo_cache_hits() == 0 and L.cryo_cache_misses() == 0 and L.cryo_cache_codec_calls() == 0
    finally:
        L.cryo_memrel_destroy(mem)


def test_check_relation_needs_check_blocks(oracle):
    import codec_double
    L = host.lib()
    dbl = codec_double.OracleCodecOps()
    ops = host.CryoCodecOpsCheck(dbl._bound, dbl._comp, dbl._decomp, None)   # check_blocks NULL
    L.cryo_host_set_codec_ops(C.byref(ops))
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 32, C.byref(rel))
    try:
        with pytest.raises(host.CheckRelationError) as e:
            host.check_relation(rel)
        assert e.value.code == -6                        # CRYO_E_UNSUPPORTED
    finally:
        L.cryo_memrel_destroy(mem)
        L.cryo_host_set_codec_ops(None)


def test_empty_relation(HC):
    L, dbl, _ = HC
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, 33, C.byref(rel))
    try:
        assert host.check_relation(rel) == ([], {"blocks": 0, "empty_pages": 0, "bad": 0, "codec_calls": 0})
        assert dbl.calls == []
    finally:
        L.cryo_memrel_destroy(mem)
