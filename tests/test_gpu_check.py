"""GPU tests of the stored-block check (cryo_codec_check_batch, cryo_codec_check_blocks, cryo_multi_check_blocks, and
cryo_check_relation through the shipped host library).

Every verdict is compared with tests/layout_ref.py, the numpy statement of the layout rules in include/cryo_codec.h."""
import ctypes as C
import struct

import numpy as np
import pytest

import layout_ref as ref
import oracle_lib
from mini_am import load_relation
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc, host

pytestmark = pytest.mark.gpu

DISTS = range(5)


@pytest.fixture(scope="module")
def stock():
    return oracle_lib.StockLibs()


@pytest.fixture()
def chk(codec):
    yield codec
    for opt, v in ((cc.OPT_ZSTD_CHECKSUM, 0), (cc.OPT_ENCODE_SEGMENT_BYTES, 0), (cc.OPT_WORKSPACE_MAX_BYTES, 0),
                   (cc.OPT_PIPE_MIN_BYTES, 64 << 20), (cc.OPT_POOL_BYTES, 0), (cc.OPT_LZ4_DECODE_PATH, 0),
                   (cc.OPT_ZSTD_DECODE_PATH, 0)):
        codec.set_option(opt, v)


def check_batch(codec, method, comps, B):
    """cryo_codec_check_batch on device copies of the streams (16-byte aligned, cryo_dev_alloc slack): (n, 2) uint32"""
    n = len(comps)
    sizes = np.array([len(c) for c in comps], np.uint32)
    offs = np.zeros(n, np.uint64)
    pos = 0
    for i, c in enumerate(comps):
        offs[i] = pos
        pos += (len(c) + 15) & ~15
    packed = np.zeros(max(pos, 16), np.uint8)
    for i, c in enumerate(comps):
        packed[int(offs[i]):int(offs[i]) + len(c)] = np.asarray(c, np.uint8)
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(8 * n)]
    d_src, d_off, d_sz, d_res = bufs
    try:
        d_src.upload(packed)
        d_off.upload(offs)
        d_sz.upload(sizes)
        d_res.memset(0xEE)
        codec.check_batch(method, d_src, d_off, d_sz, B, n, d_res)
        codec.sync()
        return d_res.download(dtype=np.uint32).reshape(n, 2).copy()
    finally:
        for b in bufs:
            b.free()


def oracle_encode(oracle, method, raw):
    return oracle.lz4_compress(raw, 1) if method == METHOD_LZ4 else oracle.zstd_compress(raw, 1)


def expect_ok(res):
    assert (res[:, 0] == ref.OK).all() and (res[:, 1] == ref.NONE).all(), res[res[:, 0] != ref.OK][:5]


# ---- valid streams pass ----
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_valid_streams_pass(chk, oracle, stock, B):
    raws = [oracle.synth(11, 3 * d + k, B, d) for d in DISTS for k in range(2 if B > 131072 else 4)]
    for raw in raws:
        assert ref.check_block(raw) == (ref.OK, ref.NONE)
    for method in (METHOD_LZ4, METHOD_ZSTD):
        sources = {"oracle": [oracle_encode(oracle, method, r) for r in raws],
                   "gpu": chk.compress_blocks(method, 1, raws)}
        if method == METHOD_ZSTD:
            chk.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
            sources["gpu checksummed"] = chk.compress_blocks(method, 1, raws)
            chk.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
        chk.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 16384)
        sources["gpu segment"] = chk.compress_blocks(method, 1, raws)
        chk.set_option(cc.OPT_ENCODE_SEGMENT_BYTES, 0)
        if method == METHOD_LZ4 and stock.lz4 is not None:
            sources["liblz4"] = [stock.lz4_compress(r, 1) for r in raws]
        if method == METHOD_ZSTD and stock.zstd is not None:
            sources["libzstd"] = [stock.zstd_compress(r, 1) for r in raws]
            sources["libzstd checksummed"] = [stock.zstd_compress2(r, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: 1,
                                                                       oracle_lib.ZSTD_C_CHECKSUM_FLAG: 1}) for r in raws]
        for name, comps in sources.items():
            res = check_batch(chk, method, comps, B)
            assert (res[:, 0] == ref.OK).all(), (method, name, res[res[:, 0] != ref.OK][:4])
            expect_ok(res)


def test_zero_blocks_and_small_sizes(chk, oracle):
    """narrow, int4 and empty blocks at 4 KiB and 16 bytes; an empty 16-byte block is header-only"""
    raws = [oracle.synth(5, d, 4096, d) for d in (1, 2, 4)]
    for method in (METHOD_LZ4, METHOD_ZSTD):
        expect_ok(check_batch(chk, method, [oracle_encode(oracle, method, r) for r in raws], 4096))
        tiny = np.zeros(16, np.uint8)
        tiny[:8] = np.frombuffer(struct.pack("<II", 8, 16), np.uint8)
        expect_ok(check_batch(chk, method, [oracle_encode(oracle, method, tiny)], 16))


# ---- layout corruptions against the reference ----
def corrupted_set(oracle, method, B, count, seed):
    rng = np.random.default_rng(seed)
    raws = []
    for k in range(count):
        d = int(rng.integers(0, 5))
        raws.append(ref.corrupt(oracle.synth(seed, k, B, d), rng))
    comps = [oracle_encode(oracle, method, r) for r in raws]
    return raws, comps


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_layout_corruptions_match_reference(chk, oracle, method, B):
    raws, comps = corrupted_set(oracle, method, B, 60 if B > 131072 else 100, 1000 + method * 7 + (B >> 17))
    res = check_batch(chk, method, comps, B)
    exp = np.array([ref.check_block(r) for r in raws], np.uint32)
    bad = np.flatnonzero((res != exp).any(axis=1))
    assert bad.size == 0, [(int(i), tuple(res[i]), tuple(exp[i])) for i in bad[:6]]
    assert {ref.OK, ref.HEADER, ref.ITEM, ref.NONZERO} <= set(exp[:, 0].tolist())


# ---- several faults in one block: the lowest one is reported ----
def make_block(B, lens, fill=0xAB):
    """a valid block of tuples of the given lengths, every tuple byte nonzero (a load past the gap's edge would see them)"""
    b = np.zeros(B, np.uint8)
    off = B
    for i, ln in enumerate(lens):
        off -= ref.maxalign(ln)
        b[off:off + ln] = fill
        b[8 + 8 * i:16 + 8 * i] = np.frombuffer(struct.pack("<II", off, ln), np.uint8)
    b[:8] = np.frombuffer(struct.pack("<II", 8 + 8 * len(lens), off), np.uint8)
    return b


def item(b, i):
    return struct.unpack_from("<II", b.tobytes(), 8 + 8 * i)


def several_faults(oracle, B):
    """(block, expected) pairs: bad pads in several turns and lanes, pads against gap bytes, gap bytes in several pieces and
    at the gap's edges where a 16-byte piece is half gap, half item array or tuple, and several failing items"""
    nar = np.array(oracle.synth(4, 0, B, 1), np.uint8)          # narrow: 290 items, t_len 61, pads of 3
    lower, upper = (int(x) for x in nar[:8].view("<u4"))
    pad = lambda b, i: item(b, i)[0] + 62                      # noqa: E731  a byte of item i's pad
    cases = []

    def case(base, pads=(), gaps=(), zero_len=(), want=None):
        b = base.copy()
        for i in pads:
            b[pad(b, i)] = 0x31
        for g in gaps:
            b[g] = 0x07
        for i in zero_len:
            b[12 + 8 * i:16 + 8 * i] = 0
        cases.append((b, want))

    case(nar, pads=(3, 100, 250), want=(ref.NONZERO, pad(nar, 250)))         # turns 0, 1, 3: the highest item is lowest
    case(nar, pads=(10, 65, 70), want=(ref.NONZERO, pad(nar, 70)))           # one turn, lanes 1 and 6
    case(nar, pads=(63, 64), want=(ref.NONZERO, pad(nar, 64)))               # either side of a turn boundary
    case(nar, pads=(256, 289, 5), want=(ref.NONZERO, pad(nar, 289)))         # the last turn
    case(nar, pads=(289,), gaps=(upper - 1,), want=(ref.NONZERO, upper - 1))   # the gap lies below every pad
    case(nar, pads=(5,), gaps=(lower,), want=(ref.NONZERO, lower))
    case(nar, gaps=(60000, 20000, B - 30000 if B > 131072 else 100000), want=(ref.NONZERO, 20000))   # several pieces
    case(nar, gaps=(20003, 20001, 20013), want=(ref.NONZERO, 20001))          # one 16-byte load
    case(nar, gaps=(20000 + 1024 + 5, 20000 + 4096 + 2), want=(ref.NONZERO, 20000 + 1024 + 5))   # two waves, two loads
    case(nar, zero_len=(200, 70), pads=(3,), want=(ref.ITEM, 8 + 8 * 70))    # items before pads
    case(nar, zero_len=(64, 63), want=(ref.ITEM, 8 + 8 * 63))
    # gap edges that split a 16-byte piece: tuples of 33 bytes in slots of 40
    odd = make_block(B, [33] * 145)      # upper at 8 mod 16
    even = make_block(B, [33] * 144)     # lower at 8 mod 16
    for b in (odd, even):
        lo, up = (int(x) for x in b[:8].view("<u4"))
        assert ref.check_block(b) == (ref.OK, ref.NONE)
        case(b, want=(ref.OK, ref.NONE))
        case(b, gaps=(up - 1,), want=(ref.NONZERO, up - 1))
        case(b, gaps=(lo,), want=(ref.NONZERO, lo))
        case(b, gaps=(up - 8, up - 1), want=(ref.NONZERO, up - 8))
    assert int(odd[4:8].view("<u4")[0]) % 16 == 8 and int(even[:4].view("<u4")[0]) % 16 == 8
    return cases


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_several_faults_report_the_lowest(chk, oracle, method, B):
    cases = several_faults(oracle, B)
    for b, want in cases:
        assert ref.check_block(b) == want
    res = check_batch(chk, method, [oracle_encode(oracle, method, b) for b, _ in cases], B)
    got = [tuple(int(x) for x in r) for r in res]
    assert got == [w for _, w in cases]


# ---- stream corruptions ----
def test_stream_corruptions(chk, oracle, stock):
    B = 131072
    raws = [oracle.synth(21, k, B, d) for k, d in enumerate((0, 1, 2, 3))]
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, r) for r in raws]
        truncated = [c[:len(c) - 7] for c in comps] + [c[:len(c) // 2] for c in comps]
        res = check_batch(chk, method, truncated, B)
        assert (res[:, 0] == ref.STREAM).all() and (res[:, 1] == ref.NONE).all(), res
    # a zstd frame whose checksum trailer no longer matches its content
    chk.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    frames = chk.compress_blocks(METHOD_ZSTD, 1, raws)
    chk.set_option(cc.OPT_ZSTD_CHECKSUM, 0)
    expect_ok(check_batch(chk, METHOD_ZSTD, frames, B))
    bent = [f.copy() for f in frames]
    for f in bent:
        f[-2] ^= 0x10
    res = check_batch(chk, METHOD_ZSTD, bent, B)
    assert (res[:, 0] == ref.STREAM).all() and (res[:, 1] == ref.NONE).all(), res
    # the documented limit: an LZ4 stream whose damage lands in a tuple body still decodes to B bytes and passes.  The last
    # bytes of a `random` block are the first tuple's body, and an LZ4 block ends with literals.
    comp = oracle.lz4_compress(raws[3], 1).copy()
    comp[-1] ^= 0x5A
    r, out = oracle.lz4_decompress(comp, B)
    assert r == B and not np.array_equal(out, raws[3]) and ref.check_block(out) == (ref.OK, ref.NONE)
    body = raws[3].copy()
    lower = int(body[:4].view("<u4")[0])
    off = int(body[8:12].view("<u4")[0])
    body[off + 40] ^= 0xFF
    assert lower < off
    expect_ok(check_batch(chk, METHOD_LZ4, [comp, oracle.lz4_compress(body, 1)], B))


# ---- decode routes, chunking ----
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_small_calls_and_chunks_give_the_same_results(chk, oracle, method):
    B = 1 << 20
    raws, comps = corrupted_set(oracle, method, B, 24, 77 + method)
    whole = check_batch(chk, method, comps, B)
    exp = np.array([ref.check_block(r) for r in raws], np.uint32)
    assert np.array_equal(whole, exp)
    # one block and eight blocks per call: the few-blocks / few-frames routes
    ones = np.concatenate([check_batch(chk, method, [c], B) for c in comps[:4]])
    assert np.array_equal(ones, exp[:4])
    eights = np.concatenate([check_batch(chk, method, comps[i:i + 8], B) for i in range(0, 24, 8)])
    assert np.array_equal(eights, exp)
    # the handle's decode-path options do not change the routes the check takes
    chk.set_option(cc.OPT_LZ4_DECODE_PATH if method == METHOD_LZ4 else cc.OPT_ZSTD_DECODE_PATH, 1)
    assert np.array_equal(check_batch(chk, method, comps, B), exp)
    chk.set_option(cc.OPT_LZ4_DECODE_PATH if method == METHOD_LZ4 else cc.OPT_ZSTD_DECODE_PATH, 0)
    # a small workspace budget: several chunks
    chk.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 8 << 20)
    assert np.array_equal(check_batch(chk, method, comps, B), exp)
    chk.set_option(cc.OPT_WORKSPACE_MAX_BYTES, 0)


def test_arguments(chk, oracle):
    comp = oracle.lz4_compress(oracle.synth(1, 0, 4096, 1), 1)
    d = [chk.alloc(64) for _ in range(4)]
    try:
        for method, B in ((7, 4096), (METHOD_LZ4, 4092), (METHOD_LZ4, 8), (METHOD_LZ4, 0)):
            with pytest.raises(CryoError) as e:
                chk.check_batch(method, d[0], d[1], d[2], B, 1, d[3])
            assert e.value.code == cc.E_ARG
        assert chk.L.cryo_codec_check_batch(chk.h, METHOD_LZ4, None, None, None, 4096, 0, None) == cc.OK
        assert chk.L.cryo_codec_check_batch(chk.h, METHOD_LZ4, d[0].ptr, d[1].ptr, d[2].ptr, 4096, 1, None) == cc.E_ARG
    finally:
        for b in d:
            b.free()
    with pytest.raises(CryoError) as e:
        chk.check_blocks(METHOD_ZSTD, [comp], 4100)
    assert e.value.code == cc.E_ARG
    assert chk.check_blocks(METHOD_LZ4, [], 4096).shape == (0, 2)


# ---- host-buffer calls ----
def multi_check(method, comps, B, devices=(0, 0)):
    L = cc.lib()
    h = C.c_void_p()
    devs = (C.c_int * len(devices))(*devices)
    assert L.cryo_multi_open(devs, len(devices), C.byref(h)) == 0
    try:
        n = len(comps)
        arrs = [np.ascontiguousarray(np.asarray(c, np.uint8)) for c in comps]
        src = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        szs = (C.c_uint32 * n)(*[a.nbytes for a in arrs])
        out = np.zeros((n, 2), np.uint32)
        assert L.cryo_multi_check_blocks(h, method, src, szs, n, B, out.ctypes.data) == 0
        tc = cc.TransferCounters()
        assert L.cryo_multi_get_transfer_counters(h, C.byref(tc)) == 0
        return out, tc.d2h_bytes
    finally:
        L.cryo_multi_close(h)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_host_buffer_calls(chk, oracle, method):
    B = 131072
    raws, comps = corrupted_set(oracle, method, B, 40, 300 + method)
    exp = np.array([ref.check_block(r) for r in raws], np.uint32)
    dev = check_batch(chk, method, comps, B)
    assert np.array_equal(dev, exp)
    chk.set_option(cc.OPT_POOL_BYTES, 8 * B)
    before_t, before_c = chk.transfer_counters(), chk.counters()
    res = chk.check_blocks(method, comps, B)
    after_t, after_c = chk.transfer_counters(), chk.counters()
    chk.set_option(cc.OPT_POOL_BYTES, 0)
    assert np.array_equal(res, exp)
    assert after_t["d2h_bytes"] - before_t["d2h_bytes"] == 8 * len(comps)
    assert after_t["h2d_bytes"] - before_t["h2d_bytes"] >= sum(len(c) for c in comps)
    for k in ("pool_hits", "pool_misses", "pool_blocks"):
        assert after_t[k] == before_t[k], k
    assert after_c == before_c
    got, d2h = multi_check(method, comps, B)
    assert np.array_equal(got, exp) and d2h == 8 * len(comps)


def test_host_buffer_pipelined_calls(chk, oracle):
    """the pipelined staging of cryo_codec_decompress_blocks (CRYO_OPT_PIPE_MIN_BYTES = 0): a check per chunk (LZ4, chunks of
    at least 512 blocks) and one check behind the uploads (zstd)"""
    B = 16384
    n = 2048
    raws = [oracle.synth(9, k, B, k % 3 + 1) for k in range(n)]
    rng = np.random.default_rng(5)
    for k in range(0, n, 97):
        raws[k] = ref.corrupt(raws[k], rng)
    exp = np.array([ref.check_block(r) for r in raws], np.uint32)
    chk.set_option(cc.OPT_PIPE_MIN_BYTES, 0)
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [oracle_encode(oracle, method, r) for r in raws]
        before = chk.transfer_counters()["d2h_bytes"]
        res = chk.check_blocks(method, comps, B)
        assert chk.transfer_counters()["d2h_bytes"] - before == 8 * n
        assert np.array_equal(res, exp)
    chk.set_option(cc.OPT_PIPE_MIN_BYTES, 64 << 20)


# ---- the shipped host library ----
@pytest.fixture()
def HG():
    host.use(production=True)
    L = host.lib()
    assert not hasattr(L, "cryo_host_set_codec_ops")
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


def test_check_relation_production_library(HG, oracle):
    L, errors = HG
    rows = [struct.pack("<i", i) for i in range(1, 10001)]
    mem, rel, blocks, firsts = load_relation(L, rows, 1, host.COMP_LZ4, batch=16)
    try:
        assert len(blocks) == 35 and not errors
        reports, totals = host.check_relation(rel)
        assert reports == [] and totals["blocks"] == 35 and totals["bad"] == 0 and totals["codec_calls"] == 1

        def poke(b, at, data):
            C.memmove(L.cryo_memrel_page(mem, b) + at, data, len(data))

        def rewrite(first_block, raw):
            comp = oracle.lz4_compress(np.frombuffer(raw, np.uint8), 1)
            chain, np_ = (C.c_uint32 * 64)(), C.c_int()
            assert L.cryo_stage_write_chain(C.byref(rel), first_block, host.COMP_LZ4, 777, comp.ctypes.data, comp.nbytes,
                                            chain, 64, C.byref(np_)) == 0 and np_.value == 1

        expect = []
        b = bytearray(blocks[3])
        b[5000] = 0x11                                           # a gap byte
        rewrite(firsts[3], bytes(b))
        expect.append((firsts[3], ref.NONZERO, 5000, 1))
        b = bytearray(blocks[9])
        struct.pack_into("<I", b, 12 + 8 * 17, 0)                # item 17's len
        rewrite(firsts[9], bytes(b))
        expect.append((firsts[9], ref.ITEM, 8 + 8 * 17, 1))
        b = bytearray(blocks[20])
        struct.pack_into("<I", b, 4, 131072 + 8)                 # upper beyond the block
        rewrite(firsts[20], bytes(b))
        expect.append((firsts[20], ref.HEADER, 0, 1))
        csize = struct.unpack_from("<I", C.string_at(L.cryo_memrel_page(mem, firsts[25]) + 40, 4))[0]
        poke(firsts[25], 40, struct.pack("<I", csize - 9))       # a truncated stream
        expect.append((firsts[25], ref.STREAM, ref.NONE, 1))
        poke(firsts[30], 36, struct.pack("<i", 7))               # method 7
        expect.append((firsts[30], host.CRYO_CHECK_METHOD, 7, 1))
        orphan = L.cryo_memrel_reserve(mem)                      # a page that names another chain's start
        poke(orphan, 14, struct.pack("<H", 8192))
        poke(orphan, 24, struct.pack("<I", firsts[0]))
        expect.append((orphan, host.CRYO_CHECK_CHAIN, host.CRYO_ERR_WRONG_STARTING_BLOCK, 0))
        L.cryo_memrel_reserve(mem)                               # a reserved, never written page: skipped
        reports, totals = host.check_relation(rel)
        assert reports == sorted(expect)
        assert totals == {"blocks": 36, "empty_pages": 1, "bad": 6, "codec_calls": 1}
        assert not errors
    finally:
        L.cryo_memrel_destroy(mem)
