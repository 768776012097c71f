"""GPU: every encode and decode route on blocks above 1 MiB (tests/large_blocks.py; the references are pinned by
tests/test_large_blocks_cpu.py).

Encode: bytes == liblz4 1.9.3 / libzstd 1.4.8 (and the oracle where it takes the input: LZ4, zstd levels -5 .. 10) for every
size class and builder, in a batch, alone in a call and through the host call; with content checksums; with write
verification; with strides that put poison and identical neighbours next to the blocks.
Decode: every LZ4 route and every zstd path on stock streams, crafted LZ4 streams, frames without a content size, frames
with offsets of 32 MiB and more, and damaged copies: status 0 exactly when the oracle returns B, the oracle's bytes, nothing
outside the block (_batch_check of tests/test_gpu_decode_conformance.py).
Above: stored-block check, recompression and tuple fetch at 4 MiB + 24; the block-size limit of every entry point.

The file uses a handle of its own; every option it sets is restored after each test."""
import ctypes as C
import time

import numpy as np
import pytest

import fetch_ref
import large_blocks as lb
import layout_ref
import lz4_craft
import oracle_lib
import zstd_craft
from large_blocks import MIB
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, Codec, codec as cc
from test_gpu_decode_conformance import GAP, POISON, _batch_check, _options, _truth

pytestmark = pytest.mark.gpu

OPTIONS = [cc.OPT_LZ4_DECODE_PATH, cc.OPT_LZ4_INDEX_WALKERS, cc.OPT_LZ4_DECODE_WAVES, cc.OPT_ZSTD_DECODE_PATH,
           cc.OPT_ENCODE_VERIFY, cc.OPT_ZSTD_CHECKSUM, cc.OPT_POOL_BYTES, cc.OPT_ENCODE_SEGMENT_BYTES]
MAX_BLOCK = 0x7E000000


@pytest.fixture(scope="module")
def c():
    h = Codec(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def stock():
    return lb.require_stock()


_device_error = []


@pytest.fixture(autouse=True)
def _restore(c):
    """options back to what they were after every test; once a test has left the device in error (a failed sync), the tests
    after it fail at once instead of launching more work on it"""
    if _device_error:
        pytest.fail("not run: %s left the device in error" % _device_error[0])
    saved = {k: c.get_option(k) for k in OPTIONS}
    yield
    try:
        c.sync()
    except cc.CryoError:
        _device_error.append("an earlier test")
        raise
    for k, v in saved.items():
        c.set_option(k, v)


def _reference(oracle, stock, method, param, raw):
    """the stock library's stream; the oracle's has to be the same wherever the oracle takes the input"""
    if method == METHOD_LZ4:
        exp = stock.lz4_compress(raw, param)
        if raw.nbytes <= 16 * MIB + 1:
            assert np.array_equal(oracle.lz4_compress(raw, param), exp), ("oracle != liblz4", raw.nbytes, param)
    else:
        exp = stock.zstd_compress(raw, param)
        if param <= 10 and raw.nbytes <= 16 * MIB + 1:
            assert np.array_equal(oracle.zstd_compress(raw, param), exp), ("oracle != libzstd", raw.nbytes, param)
    assert len(exp) > 0
    return exp


def _first_diff(a, b):
    k = min(len(a), len(b))
    d = np.flatnonzero(a[:k] != b[:k])
    return int(d[0]) if d.size else k


def _encode_check(c, oracle, stock, method, param, named, alone=None):
    """one batch of equally sized blocks [(name, raw)]: bytes == the reference; `alone`: that builder once more, alone in a
    call and through the host call cryo_codec_compress_block"""
    names, raws = [n for n, _ in named], [r for _, r in named]
    B = raws[0].nbytes
    t0 = time.time()
    got = c.compress_blocks(method, param, raws)
    t1 = time.time()
    print("encode method %d param %d B %d: %d blocks in %.2f s" % (method, param, B, len(raws), t1 - t0))
    exps = []
    for name, raw, g in zip(names, raws, got):
        exp = _reference(oracle, stock, method, param, raw)
        exps.append(exp)
        assert np.array_equal(g, exp), ("byte mismatch", "lz4" if method == METHOD_LZ4 else "zstd", B, param, name, "batch",
                                        len(g), len(exp), _first_diff(g, exp))
    if alone is not None:
        i = names.index(alone)
        g = c.compress_blocks(method, param, [raws[i]])[0]
        assert np.array_equal(g, exps[i]), ("byte mismatch", method, B, param, alone, "alone", len(g), len(exps[i]))
        g = c.compress_block(method, param, raws[i])
        assert np.array_equal(g, exps[i]), ("byte mismatch", method, B, param, alone, "compress_block", len(g), len(exps[i]))


# ---------------- encode: LZ4 ----------------
LZ4_ACCELS = [1, 3, 50, 65537]


@pytest.mark.parametrize("B", lb.LZ4_ENC[:-1])
def test_lz4_encode_is_byte_identical(c, oracle, stock, B):
    """1 MiB + 1 .. 16 MiB: k_lz4_enc2<2048, 8, true, false> (8 high position bits, no tag bits); 16 MiB + 1: the serial
    kernel"""
    named = lb.blocks(oracle, B)
    for accel in LZ4_ACCELS:
        _encode_check(c, oracle, stock, METHOD_LZ4, accel, named, alone="far_repeats" if accel == 1 else None)


def test_lz4_encode_is_byte_identical_at_72mib(c, oracle, stock):
    named = lb.blocks(oracle, lb.FAR, ["wide", "far_repeats", "long_runs"])
    for accel in (1, 50):
        _encode_check(c, oracle, stock, METHOD_LZ4, accel, named, alone="long_runs" if accel == 1 else None)


# ---------------- encode: zstd ----------------
ZSTD_LEVELS = lb.ZSTD_LEVELS   # every strategy at every size class (tests/test_large_blocks_cpu.py checks the table)
# levels that repeat a strategy another level runs at every size class: lazy2 (8 everywhere) and btultra2 (19 everywhere)
# (level 10 is the one lazy2 level with window log 22: lazy2 with a 4 MiB window below an 8 MiB + 1 block is not run; levels 13
# and 16, window log 22 as well, run there)
REPEATED = {10: [MIB + 1, 2 * MIB, 2 * MIB + 1], 12: [MIB + 1, 2 * MIB, 2 * MIB + 1, 4 * MIB + 24], 22: [MIB + 1, 4 * MIB + 24]}
ZSTD_CELLS = [(B, level) for B in lb.ZSTD_ENC[:-1] for level in ZSTD_LEVELS if B in REPEATED.get(level, lb.ZSTD_ENC)]
HALF = ["wide", "far_repeats", "long_runs", "periodic_noise", "text_noise"]
FEW = ["wide", "far_repeats", "long_runs"]
# the synth block next to far_repeats at the binary-tree levels (13 .. 22: one wave per block, seconds per MiB)
TREE_SYNTH = {MIB + 1: "wide", 2 * MIB: "narrow", 2 * MIB + 1: "int4", 4 * MIB + 24: "int4", 8 * MIB + 1: "zeros"}


def _zstd_builders(B, level):
    if level >= 13:
        return ["far_repeats", TREE_SYNTH[B]]
    return lb.BUILDERS if B <= 2 * MIB + 1 else (HALF if B <= 4 * MIB + 24 else FEW)


@pytest.mark.parametrize("B,level", ZSTD_CELLS)
def test_zstd_encode_is_byte_identical(c, oracle, stock, B, level):
    """table entries of index | tag << ib with 11 .. 8 tag bits; windows smaller than the block from 1 MiB + 1 (level 2),
    2 MiB + 1 (3 .. 9), 4 MiB + 1 (10 .. 16) and 8 MiB + 1 (17 .. 19) on; frames of 9 .. 65 zstd blocks"""
    named = lb.blocks(oracle, B, _zstd_builders(B, level))
    _encode_check(c, oracle, stock, METHOD_ZSTD, level, named, alone="far_repeats" if level == 3 else None)


@pytest.mark.parametrize("level", [1, 3])
def test_zstd_encode_is_byte_identical_at_72mib(c, oracle, stock, level):
    """577 zstd blocks per frame, 5 tag bits"""
    named = lb.blocks(oracle, lb.FAR, ["wide", "far_repeats", "far_window"])
    _encode_check(c, oracle, stock, METHOD_ZSTD, level, named, alone="far_repeats" if level == 1 else None)


@pytest.mark.parametrize("B", [2 * MIB + 1, lb.FAR])
def test_zstd_encode_with_content_checksum(c, oracle, stock, B):
    c.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    named = lb.blocks(oracle, B, HALF if B < lb.FAR else ["far_repeats", "long_runs"])
    for level in (1, 9):
        got = c.compress_blocks(METHOD_ZSTD, level, [r for _, r in named])
        for (name, raw), g in zip(named, got):
            exp = stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: level, oracle_lib.ZSTD_C_CHECKSUM_FLAG: 1})
            assert np.array_equal(g, exp), ("byte mismatch", "zstd+checksum", B, level, name, len(g), len(exp), _first_diff(g, exp))


@pytest.mark.parametrize("method,param,B", [(METHOD_LZ4, 1, 4 * MIB), (METHOD_ZSTD, 3, 4 * MIB + 24)])
def test_encode_with_write_verification(c, oracle, stock, method, param, B):
    """CRYO_OPT_ENCODE_VERIFY = 1: the same bytes, every status OK (compress_blocks raises on any other)"""
    c.set_option(cc.OPT_ENCODE_VERIFY, 1)
    _encode_check(c, oracle, stock, method, param, lb.blocks(oracle, B), alone="far_repeats")
    assert c.last_verify_failure() is None


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_ZSTD, 3), (METHOD_ZSTD, 13)])
def test_encode_placement_with_odd_strides(c, oracle, stock, method, param):
    """compress_batch with src_stride = B + 3 (poison between the blocks; identical periodic blocks next to each other, so that
    a match that read past a block's end would find its continuation) and dst_stride = bound + 7 over a poisoned
    destination: the reference's bytes, nothing written at or beyond bound of a slot"""
    B = 2 * MIB + 5
    per = lb.periodic_noise(B)
    named = [("periodic_noise", per), ("periodic_noise", per), ("periodic_noise", per)] + lb.blocks(oracle, B, ["far_repeats", "wide", "long_runs"]) \
        + [("periodic_noise", per)]
    n, S = len(named), B + 3
    bound = cc.bound(method, B)
    D = bound + 7
    src = np.full(n * S, 0x61, np.uint8)          # 'a': the byte the periodic block would go on with
    for i, (_, raw) in enumerate(named):
        src[i * S:i * S + B] = raw
    bufs = [c.alloc(src.nbytes), c.alloc(n * D), c.alloc(4 * n), c.alloc(4 * n)]
    d_src, d_dst, d_sz, d_st = bufs
    try:
        d_src.upload(src)
        d_dst.memset(POISON)
        c.compress_batch(method, param, d_src, S, B, n, d_dst, D, d_sz, d_st)
        c.sync()
        st, sz = d_st.download(dtype=np.int32), d_sz.download(dtype=np.uint32)
        out = d_dst.download().reshape(n, D)
    finally:
        for b in bufs:
            b.free()
    assert (st == 0).all(), st
    assert (out[:, bound:] == POISON).all(), "wrote at or beyond bound of a slot"
    for i, (name, raw) in enumerate(named):
        exp = _reference(oracle, stock, method, param, raw)
        assert sz[i] == len(exp) and np.array_equal(out[i, :sz[i]], exp), ("byte mismatch", method, B, param, name, i, int(sz[i]), len(exp))


# ---------------- decode ----------------
def _dedupe(expect, raws):
    """the expected block as the builder's own array where they are equal (one copy in memory, not one per stream)"""
    for r in raws:
        if expect is not None and np.array_equal(expect, r):
            return r
    return expect


def _cases(oracle, method, named, B, raws):
    streams = [m for _, m in named]
    return [(name, m, _dedupe(e, raws)) for (name, m), e in zip(named, _truth(oracle, method, streams, B))]


def _lz4_builders(B):
    if B <= 4 * MIB + 24:
        return [(n, (1, 50) if n in ("wide", "far_repeats", "long_runs") else (1,)) for n in lb.BUILDERS]
    if B <= 16 * MIB + 8:
        return [("wide", (1, 50)), ("far_repeats", (1,)), ("long_runs", (1,)), ("incompressible", (1,))]
    return [("wide", (1,)), ("long_runs", (50,))]


def _lz4_cases(oracle, stock, B):
    named, raws = [], []
    for name, accels in _lz4_builders(B):
        raw = lb.build(oracle, name, B)
        raws.append(raw)
        for a in accels:
            s = stock.lz4_compress(raw, a)
            named.append(("%s/a%d" % (name, a), s))
            if a == 1 and name in ("wide", "far_repeats", "long_runs"):
                named += lb.mutants("%s/a%d" % (name, a), s, 1)
    crafted = lz4_craft.corpus(B, lb.DEC_CRAFTED_LZ4[B], lb.CRAFTED_LZ4_SEED)
    named += [("crafted/" + n, m) for n, m in crafted]
    cases = _cases(oracle, METHOD_LZ4, named, B, raws)
    stock_ok = [x for x in cases if not x[0].startswith(("crafted/", "mutated")) and x[2] is not None]
    assert len(stock_ok) == sum(len(a) for _, a in _lz4_builders(B)), "a stock stream the oracle rejects"
    assert any(x[0].startswith("crafted/") and x[2] is not None for x in cases), "no accepted crafted stream"
    assert any(x[2] is None for x in cases), "no rejected stream"
    return cases


LZ4_ROUTES = [("ring", {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_RING, cc.OPT_LZ4_INDEX_WALKERS: 0})] + \
    [("indexed/w%d/v%d" % (w, v), {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_INDEXED, cc.OPT_LZ4_INDEX_WALKERS: w, cc.OPT_LZ4_DECODE_WAVES: v})
     for w in (1, 2, 8, 64) for v in (1, 2)] + \
    [("few", {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_FEW_BLOCKS, cc.OPT_LZ4_INDEX_WALKERS: 0}),
     ("auto", {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_AUTO, cc.OPT_LZ4_INDEX_WALKERS: 0, cc.OPT_LZ4_DECODE_WAVES: 0})]
ZSTD_ROUTES = [("path%d" % p, {cc.OPT_ZSTD_DECODE_PATH: p}) for p in (0, 1, 2, 3)]


def _tile(cases, n):
    return (cases * ((n + len(cases) - 1) // len(cases)))[:n]


def _shapes(cases, B):
    """one block per call (an accepted stock stream, a crafted or content-size-less one, a rejected one), every case in calls
    of 5, and at 1 MiB + 8 one call of 70"""
    ok = [x for x in cases if x[2] is not None]
    special = [x for x in ok if x[0].startswith(("crafted/", "no_content_size/", "far_window"))]
    bad = [x for x in cases if x[2] is None]
    out = [("one", [x]) for x in (ok[0], special[0], bad[0])]
    out += [("five@%d" % k, cases[k:k + 5]) for k in range(0, len(cases), 5)]
    if B == MIB + 8:
        out.append(("seventy", _tile(cases, 70)))
    return out


def _run_routes(c, method, routes, cases, B, edge=False):
    t0 = time.time()
    for rname, opts in routes:
        with _options(c, opts):
            for shape, part in _shapes(cases, B):
                _batch_check(c, method, part, B, (rname, B, shape))
            if edge:   # 64 MiB per call exactly and one block more: either side of the few-blocks byte limit
                for n in (32, 33):
                    _batch_check(c, method, _tile(cases, n), B, (rname, B, "x%d" % n))
    print("decode method %d B %d: %d cases, %d routes in %.1f s" % (method, B, len(cases), len(routes), time.time() - t0))


@pytest.mark.parametrize("B", [b for b in lb.DEC if b not in lb.ZSTD_ONLY_DEC])
def test_lz4_decode_routes(c, oracle, stock, B):
    """ring parser; sequence index with 1, 2, 8, 64 walkers and one or two decoder waves; few-blocks (up to 2 MiB per block
    and 64 MiB per call, the automatic choice beyond); automatic"""
    _run_routes(c, METHOD_LZ4, LZ4_ROUTES, _lz4_cases(oracle, stock, B), B, edge=B == 2 * MIB)


def _zstd_dec_builders(B):
    """[(builder, levels)]; level 19 costs the CPU seconds per MiB except on runs"""
    if B <= 4 * MIB + 24:
        return [(n, (1, 3, 9, 19) if n in ("wide", "far_repeats", "long_runs") else ((1, 3, 9) if n in ("narrow", "text_noise") else (1, 3)))
                for n in lb.BUILDERS]
    if B <= 16 * MIB + 8:
        return [("wide", (1, 3, 9)), ("far_repeats", (1, 3)), ("long_runs", (3, 19)), ("periodic_noise", (1,))]
    return [("wide", (1,)), ("far_repeats", (3,)), ("long_runs", (19,))]


def _zstd_cases(oracle, stock, B):
    named, raws = [], []
    n_stock = 0
    big = B > 16 * MIB + 8          # there: one content-size-less frame, damaged copies of two frames
    for k, (name, levels) in enumerate(_zstd_dec_builders(B)):
        raw = lb.build(oracle, name, B)
        raws.append(raw)
        for lvl in levels:
            f = stock.zstd_compress(raw, lvl)
            named.append(("%s/l%d" % (name, lvl), f))
            n_stock += 1
            if lvl == levels[0] and (k == 0 or not big):
                named.append(("no_content_size/%s/l%d" % (name, lvl), lb.drop_content_size(f, B)))
                if name in ("wide", "far_repeats", "long_runs"):
                    named += lb.mutants("%s/l%d" % (name, lvl), f, 2 if big else 1)
    if B >= lb.FAR:
        for name, raw, f in lb.far_frames(stock, B):
            raws.append(raw)
            named.append((name, f))
            if name.endswith("split/wlog27/l3"):
                named += lb.mutants(name, f, 2)
    cases = _cases(oracle, METHOD_ZSTD, named, B, raws)
    plain = [x for x in cases if not x[0].startswith(("no_content_size/", "mutated", "far_window")) and x[2] is not None]
    assert len(plain) == n_stock, "a stock frame the oracle rejects"
    assert any(x[0].startswith("no_content_size/") and x[2] is not None for x in cases), "no accepted content-size-less frame"
    assert any(x[2] is None for x in cases), "no rejected stream"
    if B >= lb.FAR:
        assert sum(x[0].startswith("far_window") and x[2] is not None for x in cases) == 5
    return cases


@pytest.mark.parametrize("B", lb.DEC)
def test_zstd_decode_paths(c, oracle, stock, B):
    """automatic / fused kernel / pipeline / pipeline without the few-frames execution.  253 x 128 KiB and 8 bytes more:
    frames of 253 and 254 blocks, either side of the planner's cap; 72 MiB + 24: offset codes 25 and 26"""
    cases = _zstd_cases(oracle, stock, B)
    if B in lb.ZSTD_ONLY_DEC:
        nb = len(zstd_craft.walk(next(m for name, m, _ in cases if name == "wide/l1"))["blocks"])
        assert nb == (253 if B == lb.ZSTD_ONLY_DEC[0] else 254), (B, nb)
    _run_routes(c, METHOD_ZSTD, ZSTD_ROUTES, cases, B, edge=B == 2 * MIB)


@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_host_decode_calls(c, oracle, stock, method):
    """cryo_codec_decompress_blocks_keyed with the pool on (a miss, then a hit) and cryo_codec_decompress_blocks_to, 4 MiB + 24"""
    B = 4 * MIB + 24
    cases = (_lz4_cases if method == METHOD_LZ4 else _zstd_cases)(oracle, stock, B)[:12]
    items, expect = [x[1] for x in cases], [x[2] for x in cases]
    assert any(e is None for e in expect) and any(e is not None for e in expect)
    n = len(items)
    c.set_option(cc.OPT_POOL_BYTES, 64 * MIB)
    for round_ in range(2):
        outs, st = c.decompress_blocks_keyed(method, [(7 << 32) | i for i in range(n)], items, B)
        for i in range(n):
            assert (st[i] == 0) == (expect[i] is not None), ("keyed", round_, cases[i][0], int(st[i]))
            if st[i] == 0:
                assert np.array_equal(outs[i], expect[i]), ("keyed", round_, cases[i][0])
    assert c.transfer_counters()["pool_hits"] > 0
    c.pool_invalidate(everything=True)
    srcs = [np.ascontiguousarray(m) for m in items]
    dsts = [np.full(B + GAP, POISON, np.uint8) for _ in range(n)]
    h_src = (C.c_void_p * n)(*[a.ctypes.data for a in srcs])
    h_sz = (C.c_uint32 * n)(*[a.nbytes for a in srcs])
    h_dst = (C.c_void_p * n)(*[d.ctypes.data for d in dsts])
    st = (C.c_int32 * n)()
    c._chk(cc.lib().cryo_codec_decompress_blocks_to(c.h, method, h_src, h_sz, n, h_dst, B, st), "decompress_blocks_to")
    for i in range(n):
        assert (dsts[i][B:] == POISON).all(), ("wrote past the block", cases[i][0])
        assert (st[i] == 0) == (expect[i] is not None), ("blocks_to", cases[i][0], st[i])
        if st[i] == 0:
            assert np.array_equal(dsts[i][:B], expect[i]), ("blocks_to", cases[i][0])
        else:
            assert st[i] == cc.E_CORRUPT and (dsts[i] == POISON).all(), ("rejected block's destination written", cases[i][0])


# ---------------- the layers above, 4 MiB + 24 ----------------
def _stored_block(B):
    """a well-formed block of 290 tuples (the most the layout takes) that fill it, bodies of text with noise"""
    lens = [(B - 8 - 8 * 290) // 290 - 8 - (i % 7) for i in range(290)]
    text = lb.text_noise(B)
    at = [0]

    def fill(i):
        at[0] += lens[i]
        return text[at[0] - lens[i]:at[0]]
    return fetch_ref.build_block(B, lens, pad=0, fill=fill)


@pytest.mark.parametrize("method,param", [(METHOD_LZ4, 1), (METHOD_ZSTD, 3)])
def test_check_recode_and_fetch(c, oracle, stock, method, param):
    B = 4 * MIB + 24
    good = _stored_block(B)
    assert layout_ref.check_block(good) == (layout_ref.OK, layout_ref.NONE)
    header, item, nonzero = good.copy(), good.copy(), good.copy()
    layout_ref._set_u32(header, 0, 4)
    layout_ref._set_u32(item, 12 + 8 * 145, 0)
    lower, upper = layout_ref._u32(good, 0), layout_ref._u32(good, 4)
    assert upper > lower
    nonzero[upper - 1] = 9
    blocks = [good, header, item, nonzero]
    assert [layout_ref.check_block(b)[0] for b in blocks] == [layout_ref.OK, layout_ref.HEADER, layout_ref.ITEM, layout_ref.NONZERO]
    comps = c.compress_blocks(method, param, blocks)
    for raw, comp in zip(blocks, comps):
        assert np.array_equal(comp, _reference(oracle, stock, method, param, raw))
    damaged = comps[0][:len(comps[0]) - 3]
    streams = comps + [damaged]
    want = [layout_ref.check_stream(oracle, method, m, B) for m in streams]
    assert want[4] == (layout_ref.STREAM, layout_ref.NONE)
    got = c.check_blocks(method, streams, B)
    assert [tuple(int(v) for v in row) for row in got] == want
    # fetch: first, middle and last tuple of the good block, and of the damaged stream
    reqs = [[1, 145, 290], [1, 145, 290]]
    pair = [comps[0], damaged]
    rec, dst, total = c.fetch_blocks(method, pair, B, reqs)
    erec, epacked, etotal = fetch_ref.fetch_call([layout_ref.decode(oracle, method, m, B) for m in pair], reqs)
    assert total == etotal and np.array_equal(rec, erec) and np.array_equal(dst[:total], epacked)
    assert [int(s) for s in rec["status"]] == [fetch_ref.OK] * 3 + [fetch_ref.STREAM] * 3
    # recode to zstd-3 with content checksums == the compress call's bytes == libzstd's
    c.set_option(cc.OPT_ZSTD_CHECKSUM, 1)
    outs, st, _, _, _ = c.recode_blocks(method, streams, B, METHOD_ZSTD, 3)
    direct = c.compress_blocks(METHOD_ZSTD, 3, blocks)
    assert [int(s) for s in st] == [0, 0, 0, 0, cc.E_CORRUPT]
    for i, raw in enumerate(blocks):
        exp = stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: 3, oracle_lib.ZSTD_C_CHECKSUM_FLAG: 1})
        assert np.array_equal(direct[i], exp), ("compress", i)
        assert np.array_equal(outs[i], exp), ("recode", i)


# ---------------- the upper limit ----------------
def test_block_size_limit_of_every_entry_point(c):
    """block_size = 0x7E000000 is taken and 0x7E000001 (check, fetch and the four scans: 0x7E000000 + 8, they want multiples
    of 8) gets CRYO_E_ARG from every entry point that takes a block size -- with no blocks, so that nothing is launched"""
    L, h = cc.lib(), c.h
    one = np.zeros(64, np.uint8)
    p = one.ctypes.data
    ptrs = (C.c_void_p * 1)(p)
    szs = (C.c_uint32 * 1)(8)
    st = (C.c_int32 * 1)()
    first = np.zeros(2, np.uint64)
    total = C.c_uint64()
    d = c.alloc(256)
    # the scan calls: valid one-column descriptors (an int4 column, no key; that column aggregated, grouped by and projected).
    # The batch forms read their descriptors from device memory even for an empty call: real device arrays at 0, 64 and 128 of
    # `desc`, their outputs and totals in `d`
    desc = c.alloc(256)
    f_h, g_h, a_h, p_h = cc.filter_desc([(4, 4)]), cc.group_desc([(1, 2)]), cc.agg_desc([(1, 2)]), cc.project_desc([1])
    scan_total = (C.c_uint64 * 2)()
    try:
        dp = d.ptr
        desc.upload(f_h[1], 0)
        desc.upload(a_h[1], 64)
        desc.upload(p_h[1], 128)
        f_d = cc.CryoFilter(1, 0, 0, 0, desc.ptr, None)
        a_d, g_d, p_d = cc.CryoAgg(1, 0, desc.ptr + 64), cc.CryoGroup(1, 0, desc.ptr + 64), cc.CryoProject(1, 0, desc.ptr + 128)
        F, A, G, P = C.byref(f_d), C.byref(a_d), C.byref(g_d), C.byref(p_d)
        FH, AH, GH, PH = C.byref(f_h[0]), C.byref(a_h[0]), C.byref(g_h[0]), C.byref(p_h[0])
        scans = ("filter", "agg", "group", "project", "multi_filter", "multi_agg", "multi_group", "multi_project")
        calls = {
            "filter_batch": lambda B: L.cryo_codec_filter_batch(h, 0, dp, dp, dp, B, 0, F, dp, 0, dp, 0, dp, dp),
            "agg_batch": lambda B: L.cryo_codec_agg_batch(h, 0, dp, dp, dp, B, 0, F, A, dp, dp),
            "group_batch": lambda B: L.cryo_codec_group_batch(h, 0, dp, dp, dp, B, 0, F, G, A, dp, dp, 0, dp, dp),
            "project_batch": lambda B: L.cryo_codec_project_batch(h, 0, dp, dp, dp, B, 0, F, P, dp, 0, dp, 0, dp, dp),
            "filter_blocks": lambda B: L.cryo_codec_filter_blocks(h, 0, ptrs, szs, 0, B, FH, p, 0, p, 0, p, scan_total),
            "agg_blocks": lambda B: L.cryo_codec_agg_blocks(h, 0, ptrs, szs, 0, B, FH, AH, p, p),
            "group_blocks": lambda B: L.cryo_codec_group_blocks(h, 0, ptrs, szs, 0, B, FH, GH, AH, p, p, 0, p, C.byref(total)),
            "project_blocks": lambda B: L.cryo_codec_project_blocks(h, 0, ptrs, szs, 0, B, FH, PH, p, 0, p, 0, p, scan_total),
            "compress_batch": lambda B: L.cryo_codec_compress_batch(h, 0, 1, dp, B, B, 0, dp, B + B // 255 + 16, dp, dp),
            "decompress_batch": lambda B: L.cryo_codec_decompress_batch(h, 0, dp, dp, dp, dp, B, B, 0, dp),
            "verify_batch": lambda B: L.cryo_codec_verify_batch(h, 0, dp, B, B, 0, dp, dp, dp, dp, None),
            "check_batch": lambda B: L.cryo_codec_check_batch(h, 0, dp, dp, dp, B, 0, dp),
            "recode_batch": lambda B: L.cryo_codec_recode_batch(h, 0, dp, dp, dp, B, 0, 1, 3, dp, B + (B >> 8), dp, dp),
            "synth_batch": lambda B: L.cryo_codec_synth_batch(h, 1, 0, 1, 0, B, 0, dp, B),
            "compare_batch": lambda B: L.cryo_codec_compare_batch(h, dp, B, dp, B, B, 0, dp),
            "fetch_batch": lambda B: L.cryo_codec_fetch_batch(h, 0, dp, dp, dp, B, 0, dp, None, 0, None, 0, None, dp),
            "compress_blocks": lambda B: L.cryo_codec_compress_blocks(h, 0, 1, p, B, 0, p, B + B // 255 + 16, p),
            "decompress_blocks": lambda B: L.cryo_codec_decompress_blocks(h, 0, ptrs, szs, 0, p, B, st),
            "decompress_blocks_to": lambda B: L.cryo_codec_decompress_blocks_to(h, 0, ptrs, szs, 0, ptrs, B, st),
            "decompress_blocks_keyed": lambda B: L.cryo_codec_decompress_blocks_keyed(h, 0, first.ctypes.data, ptrs, szs, 0, ptrs, B, st),
            "check_blocks": lambda B: L.cryo_codec_check_blocks(h, 0, ptrs, szs, 0, B, p),
            "recode_blocks": lambda B: L.cryo_codec_recode_blocks(h, 0, ptrs, szs, 0, B, 1, 3, p, 64, p, p, p),
            "fetch_blocks": lambda B: L.cryo_codec_fetch_blocks(h, 0, ptrs, szs, 0, B, first.ctypes.data, None, None, 0, None,
                                                                C.byref(total)),
        }
        for name, call in calls.items():
            over = MAX_BLOCK + (8 if name.startswith(("check", "fetch") + scans) else 1)
            assert call(MAX_BLOCK) == cc.OK, (name, "0x7E000000 refused", call(MAX_BLOCK))
            assert call(over) == cc.E_ARG, (name, hex(over), call(over))
        # the single-block host calls have no empty form: only the refusal (the arguments are checked before anything else)
        n = C.c_size_t()
        assert L.cryo_codec_compress_block(h, 0, 1, p, MAX_BLOCK + 1, p, 64, C.byref(n)) == cc.E_ARG
        assert L.cryo_codec_decompress_block(h, 0, p, 8, p, MAX_BLOCK + 1) == cc.E_ARG
        assert cc.bound(METHOD_LZ4, MAX_BLOCK) == MAX_BLOCK + MAX_BLOCK // 255 + 16 and cc.bound(METHOD_LZ4, MAX_BLOCK + 1) == 0
        m = C.c_void_p()
        assert L.cryo_multi_open((C.c_int * 1)(0), 1, C.byref(m)) == cc.OK
        try:
            mh = m.value
            multi = {
                "multi_compress_blocks": lambda B: L.cryo_multi_compress_blocks(mh, 0, 1, p, B, 0, p, B + B // 255 + 16, p),
                "multi_decompress_blocks": lambda B: L.cryo_multi_decompress_blocks(mh, 0, ptrs, szs, 0, p, B, st),
                "multi_decompress_blocks_to": lambda B: L.cryo_multi_decompress_blocks_to(mh, 0, ptrs, szs, 0, ptrs, B, st),
                "multi_decompress_blocks_keyed": lambda B: L.cryo_multi_decompress_blocks_keyed(mh, 0, first.ctypes.data, ptrs, szs, 0,
                                                                                                ptrs, B, st),
                "multi_check_blocks": lambda B: L.cryo_multi_check_blocks(mh, 0, ptrs, szs, 0, B, p),
                "multi_recode_blocks": lambda B: L.cryo_multi_recode_blocks(mh, 0, ptrs, szs, 0, B, 1, 3, p, 64, p, p, p),
                "multi_fetch_blocks": lambda B: L.cryo_multi_fetch_blocks(mh, 0, ptrs, szs, 0, B, first.ctypes.data, None, None, 0,
                                                                          None, C.byref(total)),
                "multi_filter_blocks": lambda B: L.cryo_multi_filter_blocks(mh, 0, ptrs, szs, 0, B, FH, p, 0, p, 0, p, scan_total),
                "multi_agg_blocks": lambda B: L.cryo_multi_agg_blocks(mh, 0, ptrs, szs, 0, B, FH, AH, p, p),
                "multi_group_blocks": lambda B: L.cryo_multi_group_blocks(mh, 0, ptrs, szs, 0, B, FH, GH, AH, p, p, 0, p, C.byref(total)),
                "multi_project_blocks": lambda B: L.cryo_multi_project_blocks(mh, 0, ptrs, szs, 0, B, FH, PH, p, 0, p, 0, p, scan_total),
            }
            for name, call in multi.items():
                over = MAX_BLOCK + (8 if "check" in name or "fetch" in name or name.startswith(scans) else 1)
                assert call(MAX_BLOCK) == cc.OK, (name, "0x7E000000 refused", call(MAX_BLOCK))
                assert call(over) == cc.E_ARG, (name, hex(over), call(over))
        finally:
            L.cryo_multi_close(mh)
    finally:
        d.free()
        desc.free()
