"""GPU: every LZ4 and zstd decode route against the oracle on crafted LZ4 streams (tests/lz4_craft.py), non-default zstd
frames (tests/zstd_craft.py) and hand-assembled zstd frames (tests/zstd_asm.py) -- the corpora
tests/test_decode_conformance_cpu.py pins the oracle to the stock libraries on.

For every route: status 0 exactly when the oracle returns B, then the oracle's bytes; and nothing written outside a block's
B bytes, accepted or rejected (the device batch call with dst_stride = B + 256 over a poisoned destination, compressed items
at odd offsets).  The host call cryo_codec_decompress_blocks_to leaves a rejected block's destination untouched."""
import ctypes as C

import numpy as np
import pytest

import lz4_craft
import oracle_lib
import zstd_asm
import zstd_craft
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD
from pg_cryogen_amd import codec as cc

pytestmark = pytest.mark.gpu

POISON = 0xE7
GAP = 256
LZ4_SIZES = [(4096, 300), (32768, 300), (131072, 300), (300001, 150), (1 << 20, 12)]
LZ4_SEED, ZSTD_SEED, CRAFT_SEED = 1, 5, 11


def _truth(oracle, method, items, B):
    dec = oracle.lz4_decompress if method == METHOD_LZ4 else oracle.zstd_decompress
    out = []
    for m in items:
        r, o = dec(m, B, fill=POISON)
        out.append(o.copy() if r == B else None)
    return out


@pytest.fixture(scope="module")
def lz4_corpus(oracle):
    """{B: [(name, stream, the oracle's block or None)]}"""
    out = {}
    for B, n in LZ4_SIZES:
        cs = lz4_craft.corpus(B, n, LZ4_SEED)
        out[B] = list(zip([name for name, _ in cs], [m for _, m in cs], _truth(oracle, METHOD_LZ4, [m for _, m in cs], B)))
    return out


@pytest.fixture(scope="module")
def zstd_corpus(oracle):
    stock = oracle_lib.StockLibs()
    if stock.zstd is None:
        pytest.fail("libzstd.so.1 is needed to write the non-default frames")
    by_b = {}
    for name, B, f in zstd_craft.zstd_corpus(stock, oracle, ZSTD_SEED):
        by_b.setdefault(B, ([], []))
        by_b[B][0].append(name)
        by_b[B][1].append(f)
    return {B: list(zip(names, items, _truth(oracle, METHOD_ZSTD, items, B))) for B, (names, items) in by_b.items()}


@pytest.fixture(scope="module")
def crafted_corpus(oracle):
    """{B: [(name, hand-assembled frame, the oracle's block or None)]}"""
    by_b = {}
    for name, B, f, _ in zstd_asm.crafted_corpus(CRAFT_SEED):
        by_b.setdefault(B, ([], []))
        by_b[B][0].append(name)
        by_b[B][1].append(f)
    return {B: list(zip(names, items, _truth(oracle, METHOD_ZSTD, items, B))) for B, (names, items) in by_b.items()}


def _options(codec, opts):
    """set codec options ({option: value}) for a with-block and restore what was there before, whatever happens"""
    class _Ctx:
        def __enter__(self_):
            self_.saved = {k: codec.get_option(k) for k in opts}
            for k, v in opts.items():
                codec.set_option(k, v)

        def __exit__(self_, *a):
            for k, v in self_.saved.items():
                codec.set_option(k, v)
    return _Ctx()


def _batch_check(codec, method, cases, B, tag):
    """one device batch of (name, stream, expected block or None): streams at odd offsets, dst_stride = B + GAP over a
    poisoned destination"""
    names, items, expect = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    n = len(items)
    S = B + GAP
    offs = np.zeros(n, np.uint64)
    szs = np.array([len(m) for m in items], np.uint32)
    pos = 1
    for i, m in enumerate(items):
        offs[i] = pos
        pos += len(m) + 1
        pos += 1 - (pos & 1)          # the next item starts at an odd offset too
    packed = np.full(pos + 64, 0x33, np.uint8)
    for i, m in enumerate(items):
        packed[int(offs[i]):int(offs[i]) + len(m)] = m
    bufs = [codec.alloc(packed.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(n * S), codec.alloc(4 * n)]
    d_src, d_off, d_sz, d_dst, d_st = bufs
    try:
        d_src.upload(packed)
        d_off.upload(offs)
        d_sz.upload(szs)
        d_dst.memset(POISON)
        d_st.memset(0x7F)
        codec.decompress_batch(method, d_src, d_off, d_sz, d_dst, S, B, n, d_st)
        codec.sync()
        st = d_st.download(dtype=np.int32)
        raw = d_dst.download().reshape(n, S)
    finally:
        for b in bufs:
            b.free()
    gaps = np.nonzero((raw[:, B:] != POISON).any(axis=1))[0]
    assert len(gaps) == 0, (tag, "wrote past its block", [(names[i], int(st[i])) for i in gaps[:8]])
    for i in range(n):
        assert st[i] in (cc.OK, cc.E_CORRUPT), (tag, i, names[i], int(st[i]))
        assert (st[i] == 0) == (expect[i] is not None), (tag, i, names[i], int(st[i]), len(items[i]))
        if st[i] == 0:
            assert np.array_equal(raw[i, :B], expect[i]), (tag, i, names[i], len(items[i]))


def _shapes(cases, singles, big):
    """the batch shapes a route sees: single blocks (the first `singles` cases), chunks of at most 64, and the whole corpus
    tiled to `big` items"""
    out = [("one", cases[i:i + 1]) for i in range(min(singles, len(cases)))]
    out += [("le64", cases[k:k + 64]) for k in range(0, len(cases), 64)]
    if big:
        out.append(("big", (cases * ((big + len(cases) - 1) // len(cases)))[:big]))
    return out


# ---------------- LZ4 ----------------
@pytest.mark.parametrize("B", [B for B, _ in LZ4_SIZES])
def test_lz4_ring_parser_on_crafted_streams(codec, lz4_corpus, B):
    cases = lz4_corpus[B]
    with _options(codec, {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_RING, cc.OPT_LZ4_INDEX_WALKERS: 0}):
        _batch_check(codec, METHOD_LZ4, cases, B, ("ring", B))


@pytest.mark.parametrize("B", [B for B, _ in LZ4_SIZES])
def test_lz4_indexed_decoder_on_crafted_streams(codec, lz4_corpus, B):
    """the index pass with 1 .. 64 walkers per block, then one wave per block (k_lz4_dec_seq) or two (k_lz4_dec_dual and
    the side stream of its last round); literal-heavy blocks go back to the ring parser inside the same call"""
    cases = lz4_corpus[B]
    for walkers in (1, 2, 8, 64):
        for waves in (1, 2):
            with _options(codec, {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_INDEXED, cc.OPT_LZ4_INDEX_WALKERS: walkers,
                                  cc.OPT_LZ4_DECODE_WAVES: waves}):
                _batch_check(codec, METHOD_LZ4, cases, B, ("indexed", B, walkers, waves))


@pytest.mark.parametrize("B", [32768, 131072, 300001, 1 << 20])
def test_lz4_few_blocks_path_on_crafted_streams(codec, lz4_corpus, B):
    cases = lz4_corpus[B]
    with _options(codec, {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_FEW_BLOCKS, cc.OPT_LZ4_INDEX_WALKERS: 0}):
        for shape, part in _shapes(cases, singles=8, big=0):
            _batch_check(codec, METHOD_LZ4, part, B, ("few", B, shape))


@pytest.mark.parametrize("B", [B for B, _ in LZ4_SIZES])
def test_lz4_automatic_path_on_crafted_streams(codec, lz4_corpus, B):
    """what the automatic choice makes of one block per call, of at most 64, and of a few hundred"""
    cases = lz4_corpus[B]
    with _options(codec, {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_AUTO, cc.OPT_LZ4_INDEX_WALKERS: 0,
                          cc.OPT_LZ4_DECODE_WAVES: 0}):
        for shape, part in _shapes(cases, singles=12, big=400 if B <= 300001 else 0):
            _batch_check(codec, METHOD_LZ4, part, B, ("auto", B, shape))


# ---------------- zstd ----------------
ZSTD_PATHS = [0, 1, 2, 3]   # automatic / fused kernel / pipeline (k_zexec, k_zlat_* for few frames) / pipeline without k_zlat


@pytest.mark.parametrize("path", ZSTD_PATHS)
def test_zstd_decode_paths_on_nondefault_frames(codec, zstd_corpus, path):
    with _options(codec, {cc.OPT_ZSTD_DECODE_PATH: path}):
        for B in sorted(zstd_corpus):
            cases = zstd_corpus[B]
            for shape, part in _shapes(cases, singles=6, big=300 if B <= 131072 else 0):
                _batch_check(codec, METHOD_ZSTD, part, B, ("zstd", path, B, shape))


CRAFT_SIZES = [255, 256, 4096, 8192, 32768, 65791, 131072, 262144]


@pytest.mark.parametrize("B", CRAFT_SIZES)
@pytest.mark.parametrize("path", ZSTD_PATHS)
def test_zstd_decode_paths_on_crafted_frames(codec, crafted_corpus, path, B):
    """hand-assembled frames: every frame alone, chunks of at most 64 (at B = 32768 what reaches the k_zlat_* kernels), and the
    corpus tiled to 300 frames"""
    cases = crafted_corpus[B]
    assert any(c[2] is not None for c in cases)
    with _options(codec, {cc.OPT_ZSTD_DECODE_PATH: path}):
        for shape, part in _shapes(cases, singles=len(cases), big=300 if B <= 131072 else 0):
            _batch_check(codec, METHOD_ZSTD, part, B, ("crafted", path, B, shape))
        if B == 32768 and path == 2:
            # the frames at k_zlat_count's edges (total * 64 against B, total against lat_nmax) in one call the few-frames
            # execution takes and in one of 65 frames, which it does not: the same verdicts and bytes
            edges = [c for c in cases if c[0].startswith("B/lat_total/")]
            assert len(edges) == 4 and all(c[2] is not None for c in edges)
            _batch_check(codec, METHOD_ZSTD, (edges * 16)[:64], B, ("crafted", path, B, "edges64"))
            _batch_check(codec, METHOD_ZSTD, (edges * 17)[:65], B, ("crafted", path, B, "edges65"))
        if B == 4096 and path in (0, 2):
            # B / 3 sequences per frame, 70 frames: twice the sequence pool's B / 6 per frame, so part of the batch leaves
            # the pipeline for the fused kernel
            third = [c for c in cases if c[0].startswith("B/third_of_B/")]
            assert len(third) == 3 and all(c[2] is not None for c in third)
            _batch_check(codec, METHOD_ZSTD, (third * 24)[:70], B, ("crafted", path, B, "third70"))


# ---------------- host contract ----------------
@pytest.mark.parametrize("method", [METHOD_LZ4, METHOD_ZSTD])
def test_decompress_blocks_to_leaves_rejected_destinations_untouched(codec, lz4_corpus, zstd_corpus, crafted_corpus, method):
    """cryo_codec_decompress_blocks_to (include/cryo_codec.h): block i -> h_dst[i]; a block whose status is not CRYO_OK
    leaves its destination untouched -- one mixed batch of accepted and rejected streams into separate poisoned buffers"""
    B = 131072
    cases = lz4_corpus[B] if method == METHOD_LZ4 else zstd_corpus[B] + crafted_corpus[B]
    items, expect = [c[1] for c in cases], [c[2] for c in cases]
    assert any(e is None for e in expect) and any(e is not None for e in expect)
    n = len(items)
    srcs = [np.ascontiguousarray(m) for m in items]
    dsts = [np.full(B + GAP, POISON, np.uint8) for _ in range(n)]
    L = cc.lib()
    h_src = (C.c_void_p * n)(*[a.ctypes.data for a in srcs])
    h_sz = (C.c_uint32 * n)(*[a.nbytes for a in srcs])
    h_dst = (C.c_void_p * n)(*[d.ctypes.data for d in dsts])
    st = (C.c_int32 * n)()
    codec._chk(L.cryo_codec_decompress_blocks_to(codec.h, method, h_src, h_sz, n, h_dst, B, st), "decompress_blocks_to")
    for i in range(n):
        assert (dsts[i][B:] == POISON).all(), ("wrote past the block", i)
        assert (st[i] == 0) == (expect[i] is not None), (i, st[i])
        if st[i] == 0:
            assert np.array_equal(dsts[i][:B], expect[i]), i
        else:
            assert st[i] == cc.E_CORRUPT and (dsts[i] == POISON).all(), ("rejected block's destination written", i)
