"""What the host-buffer codec calls must keep whatever code they share (pg_cryogen_amd/csrc/host_stage.h and the staging in
cryo_codec.cpp): compress, decompress, decompress_blocks_to, check, keyed decompress and a multi-GPU share's compress, one-shot
(100 blocks) and pipelined (CRYO_OPT_PIPE_MIN_BYTES = 0 and 1200 blocks of 16 KiB: three chunks of 576 / 576 / 48, LZ4 decoded
per chunk, zstd in one launch), straight through the C ABI.  Expected bytes come from the CPU oracle, expected check results from
layout_ref, expected transfer counters from the staged layout: [offsets u64 x n][sizes u32 x n] rounded up to 64, then every
stream rounded up to 16."""
import ctypes as C

import numpy as np
import pytest

import layout_ref as ref
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, bound, codec as cc

pytestmark = pytest.mark.gpu

B = 16384
N_PIPED, N_ONE_SHOT = 1200, 100       # CRYO_OPT_PIPE_MIN_BYTES = 0: a call of 128 blocks or more takes the pipeline
DISTINCT = 48                         # block i of a call is distinct block i % DISTINCT
METHODS = [METHOD_LZ4, METHOD_ZSTD]
FILL = 0xA5


@pytest.fixture(scope="module")
def blocks(oracle):
    """DISTINCT raw blocks, their streams per method as the oracle writes them, and what the check says of each"""
    raws = [oracle.synth(29, k, B, k % 4) for k in range(DISTINCT)]
    comps = {METHOD_LZ4: [oracle.lz4_compress(r, 1) for r in raws], METHOD_ZSTD: [oracle.zstd_compress(r, 1) for r in raws]}
    checks = [ref.check_block(r) for r in raws]
    return raws, comps, checks


@pytest.fixture()
def staged(codec):
    old = {opt: codec.get_option(opt) for opt in (cc.OPT_PIPE_MIN_BYTES, cc.OPT_POOL_BYTES)}
    codec.set_option(cc.OPT_PIPE_MIN_BYTES, 0)
    codec.set_option(cc.OPT_POOL_BYTES, 0)
    yield codec
    for opt, value in old.items():
        codec.set_option(opt, value)


def align(x, a):
    return (x + a - 1) // a * a


def staged_bytes(streams):
    return align(12 * len(streams), 64) + sum(align(len(s), 16) for s in streams)


def pointers(streams):
    arrs = [np.ascontiguousarray(s) for s in streams]
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    return arrs, ptrs, np.array([a.nbytes for a in arrs], np.uint32)


def moved(c, call):
    """(h2d, d2h) bytes the call adds to the handle's transfer counters"""
    t0 = c.transfer_counters()
    call()
    t1 = c.transfer_counters()
    return t1["h2d_bytes"] - t0["h2d_bytes"], t1["d2h_bytes"] - t0["d2h_bytes"]


def same_compressed(out, stride, sizes, want, untouched_tail, what):
    for i, w in enumerate(want):
        slot = out[i * stride:(i + 1) * stride]
        assert int(sizes[i]) == len(w) and np.array_equal(slot[:len(w)], w), (what, i)
        if untouched_tail:
            assert (slot[len(w):] == FILL).all(), (what, i, "written behind the stream")


# ---- 1. compress: contiguous blocks, bulk and per-block return, one-shot and pipelined ----
@pytest.mark.parametrize("method", METHODS)
def test_compress_blocks_strides(staged, blocks, method):
    raws, comps, _ = blocks
    cap = bound(method, B)
    for n in (N_PIPED, N_ONE_SHOT):
        raw = np.concatenate([raws[i % DISTINCT] for i in range(n)])
        want = [comps[method][i % DISTINCT] for i in range(n)]
        # neither a multiple of 16; up to bound + 4096 the one-shot call brings whole slots back, above it only the streams.  The
        # pipelined call always brings only the streams
        for stride, bulk in ((cap + 5, True), (cap + 4101, False)):
            out = np.full(n * stride, FILL, np.uint8)
            sizes = np.zeros(n, np.uint32)
            rc = staged.L.cryo_codec_compress_blocks(staged.h, method, 1, raw.ctypes.data, B, n, out.ctypes.data, stride, sizes.ctypes.data)
            assert rc == 0, (method, n, stride, rc)
            same_compressed(out, stride, sizes, want, n == N_PIPED or not bulk, (method, n, stride))


# ---- 2. decompress, decompress_blocks_to, check: a truncated and an empty stream among the blocks ----
def call_streams(blocks, method, n):
    """the n streams of a call, block `bad[0]` truncated and block `bad[1]` empty (both in the middle chunk of the pipelined call);
    what each decodes to (None: it does not) and what the check says of it"""
    raws, comps, checks = blocks
    streams = [comps[method][i % DISTINCT] for i in range(n)]
    want = [raws[i % DISTINCT] for i in range(n)]
    res = [checks[i % DISTINCT] for i in range(n)]
    bad = (n // 2 + 7, n // 2 + 100) if n == N_PIPED else (n // 2, n // 2 + 10)
    streams[bad[0]] = streams[bad[0]][:len(streams[bad[0]]) // 2].copy()
    streams[bad[1]] = np.zeros(0, np.uint8)
    for i in bad:
        want[i], res[i] = None, (ref.STREAM, ref.NONE)      # no bytes, or half a stream, do not decode to a block
    return streams, want, np.array(res, np.uint32)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [N_PIPED, N_ONE_SHOT])
def test_decompress_and_check_statuses_destinations_counters(staged, oracle, blocks, method, n):
    c, L = staged, staged.L
    streams, want, want_res = call_streams(blocks, method, n)
    for i in np.flatnonzero(want_res[:, 0] == ref.STREAM):
        if len(streams[i]):
            assert ref.check_stream(oracle, method, streams[i], B) == (ref.STREAM, ref.NONE)
    arrs, ptrs, szs = pointers(streams)
    up = staged_bytes(streams)
    failed = [w is None for w in want]

    out = np.full(n * B, FILL, np.uint8)
    st = np.full(n, 77, np.int32)
    got = moved(c, lambda: L.cryo_codec_decompress_blocks(c.h, method, ptrs, szs.ctypes.data, n, out.ctypes.data, B, st.ctypes.data))
    assert got == (up, n * B + 4 * n), (got, up)
    assert [s != 0 for s in st] == failed
    for i, w in enumerate(want):
        assert w is None or np.array_equal(out[i * B:(i + 1) * B], w), i

    # one destination per block, shuffled over an area with a slot to spare
    perm = np.random.default_rng(n + method).permutation(n + 1)[:n]
    area = np.full((n + 1) * B, FILL, np.uint8)
    dsts = (C.c_void_p * n)(*[area.ctypes.data + int(p) * B for p in perm])
    st = np.full(n, 77, np.int32)
    got = moved(c, lambda: L.cryo_codec_decompress_blocks_to(c.h, method, ptrs, szs.ctypes.data, n, dsts, B, st.ctypes.data))
    assert got == (up, n * B + 4 * n), (got, up)
    assert [s != 0 for s in st] == failed
    slots = area.reshape(n + 1, B)
    for i, w in enumerate(want):
        if w is None:
            assert (slots[perm[i]] == FILL).all(), (i, "a failed block's destination was written")
        else:
            assert np.array_equal(slots[perm[i]], w), i
    spare = (set(range(n + 1)) - set(perm.tolist())).pop()
    assert (slots[spare] == FILL).all()

    res = np.full((n, 2), 0xEEEEEEEE, np.uint32)
    got = moved(c, lambda: L.cryo_codec_check_blocks(c.h, method, ptrs, szs.ctypes.data, n, B, res.ctypes.data))
    assert got == (up, 8 * n), (got, up)
    assert np.array_equal(res, want_res), np.flatnonzero((res != want_res).any(axis=1))[:8]


# ---- 3. keyed decompress: a pool smaller than the call ----
@pytest.mark.parametrize("method", METHODS)
def test_keyed_decompress_in_two_rounds(staged, blocks, method):
    """40 blocks through a pool of 24 slots, first in first out: the first call misses all of them, in rounds of 24 and 16, the
    second round taking slots 0 .. 15 over.  Blocks 36 .. 39 repeat the keys and streams of 32 .. 35, block 20 is truncated (not
    kept), block 21 has no key (not kept).  What the pool then holds: 16 .. 23 but 20 and 21, and 24 .. 39; an identical second
    call finds those 22 and stages only the other 18, in one round"""
    c = staged
    raws, comps, _ = blocks
    n, S = 40, 24
    src = list(range(36)) + [32, 33, 34, 35]
    streams = [comps[method][k] for k in src]
    want = [raws[k] for k in src]
    keys = [(11 << 32) | (500 + k) for k in src]
    streams[20] = streams[20][:len(streams[20]) // 2].copy()
    want[20] = None
    keys[21] = 0
    c.set_option(cc.OPT_POOL_BYTES, S * B)
    c.pool_invalidate(everything=True)

    def call():
        t0 = c.transfer_counters()
        outs, st = c.decompress_blocks_keyed(method, keys, streams, B)
        t1 = c.transfer_counters()
        assert [s != 0 for s in st] == [w is None for w in want]
        for o, w in zip(outs, want):
            assert (o is None) if w is None else np.array_equal(o, w)     # codec.py returns None for a failed block ...
        return {k: t1[k] - t0[k] for k in ("h2d_bytes", "pool_hits", "pool_misses")}, t1
    first, t = call()
    assert first["pool_hits"] + first["pool_misses"] == n and first["pool_misses"] == n
    assert first["h2d_bytes"] == staged_bytes(streams[:S]) + staged_bytes(streams[S:])
    assert t["pool_capacity"] == S
    again, _ = call()
    missed = list(range(16)) + [20, 21]
    assert again["pool_hits"] == n - len(missed) and again["pool_misses"] == len(missed)
    assert again["h2d_bytes"] == staged_bytes([streams[i] for i in missed]), "a block still pooled was sent again"
    # ... and leaves its destination as it was
    arrs, ptrs, szs = pointers(streams)
    area = np.full(n * B, FILL, np.uint8)
    dsts = (C.c_void_p * n)(*[area.ctypes.data + i * B for i in range(n)])
    st = np.zeros(n, np.int32)
    ks = (C.c_uint64 * n)(*keys)
    assert c.L.cryo_codec_decompress_blocks_keyed(c.h, method, ks, ptrs, szs.ctypes.data, n, dsts, B, st.ctypes.data) == 0
    assert st[20] != 0 and (area[20 * B:21 * B] == FILL).all()
    assert all(np.array_equal(area[i * B:(i + 1) * B], want[i]) for i in range(n) if i != 20)


# ---- 4. a multi-GPU share's compress: blocks given by pointer, pipelined per share and one-shot ----
@pytest.mark.parametrize("method", METHODS)
def test_two_handle_compress_blocks(blocks, method):
    raws, comps, _ = blocks
    L = cc.lib()
    h = C.c_void_p()
    assert L.cryo_multi_open((C.c_int * 2)(0, 0), 2, C.byref(h)) == 0
    try:
        assert L.cryo_multi_set_option(h, cc.OPT_PIPE_MIN_BYTES, 0) == 0
        cap = bound(method, B)
        stride = cap + 5
        for n in (N_PIPED, N_ONE_SHOT):            # shares of 600 (pipelined: 128 or more) and of 50 blocks
            raw = np.concatenate([raws[i % DISTINCT] for i in range(n)])
            out = np.full(n * stride, FILL, np.uint8)
            sizes = np.zeros(n, np.uint32)
            rc = L.cryo_multi_compress_blocks(h, method, 1, raw.ctypes.data, B, n, out.ctypes.data, stride, sizes.ctypes.data)
            assert rc == 0, (method, n, L.cryo_multi_last_error(h))
            # by pointer only the streams come back, both ways
            same_compressed(out, stride, sizes, [comps[method][i % DISTINCT] for i in range(n)], True, (method, n))
    finally:
        L.cryo_multi_close(h)
