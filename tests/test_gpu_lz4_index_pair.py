"""GPU: the paired form of the one-walker LZ4 sequence index (k_lz4_idx_pair: a walker wave and a feeder wave on the same
LDS rings) against the single-wave form (k_lz4_index) and against a token walk done here.

A wrong row only costs decode speed, so the rows themselves are read back (cryo_codec_lz4_index_rows): the two forms must
write the same count and the same entries [0, count) for every block; for valid streams both must equal the low 16 bits
of every token's offset.  Then the public decode path with the paired form forced: bytes and verdicts against the oracle,
on valid, crafted, mutated and truncated streams -- which are also the termination cases of the walker / feeder pair."""
import numpy as np
import pytest

import lz4_craft
from pg_cryogen_amd import METHOD_LZ4, bound
from pg_cryogen_amd import codec as cc

pytestmark = pytest.mark.gpu

DISTS = ["wide", "narrow", "zeros", "random", "int4"]
BATCHES = [1, 63, 64, 65, 257]      # partial last pairs, lanes past the end of the batch, more than one workgroup
NMAX = max(BATCHES)


def token_walk(s, full=False):
    """low 16 bits (full: all bits) of the offset of every token of a VALID stream, the last, literals-only sequence included"""
    out, p, n = [], 0, len(s)
    while p < n:
        out.append(p if full else p & 0xffff)
        t = int(s[p]); q = p + 1
        ll = t >> 4
        if ll == 15:
            while True:
                b = int(s[q]); q += 1; ll += b
                if b != 255:
                    break
        q += ll
        if q + 2 > n:               # literals only: the last sequence
            break
        q += 2
        if (t & 15) == 15:
            while int(s[q]) == 255:
                q += 1
            q += 1
        p = q
    return out


def _pack(items, packed):
    """packed: streams at byte offsets that are no multiples of 128; else at a fixed stride of whole 128-byte lines"""
    n = len(items)
    offs = np.zeros(n, np.uint64)
    if packed:
        pos = 5
        for i, m in enumerate(items):
            offs[i] = pos
            pos += len(m) + 1 + (i % 3)
            if pos % 128 == 0:
                pos += 1
    else:
        stride = (max([len(m) for m in items] + [1]) + 127) & ~127
        offs[:] = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        pos = n * stride
    buf = np.full(pos + 256, 0x33, np.uint8)
    for i, m in enumerate(items):
        buf[int(offs[i]):int(offs[i]) + len(m)] = m
    return buf, offs, np.array([len(m) for m in items], np.uint32)


def _rows(codec, items, B, packed):
    """{form: (counts, entries n x cap)} of one batch"""
    n = len(items)
    cap = codec.lz4_index_cap(B)
    buf, offs, szs = _pack(items, packed)
    bufs = [codec.alloc(buf.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(2 * n * cap), codec.alloc(4 * n)]
    d_src, d_off, d_sz, d_ent, d_cnt = bufs
    out = {}
    try:
        d_src.upload(buf); d_off.upload(offs); d_sz.upload(szs)
        for form in (cc.LZ4_INDEX_SINGLE, cc.LZ4_INDEX_PAIR):
            d_ent.memset(0xEE); d_cnt.memset(0xEE)
            codec.lz4_index_rows(d_src, d_off, d_sz, B, n, form, d_ent, d_cnt)
            codec.sync()
            out[form] = (d_cnt.download(dtype=np.uint32).copy(), d_ent.download(dtype=np.uint16).reshape(n, cap).copy())
    finally:
        for b in bufs:
            b.free()
    return out, cap


def _same_rows(codec, items, B, packed, walk, tag):
    """both forms: equal counts, equal entries below the count; blocks listed in `walk` also against the host's token walk"""
    out, cap = _rows(codec, items, B, packed)
    c1, e1 = out[cc.LZ4_INDEX_SINGLE]
    c2, e2 = out[cc.LZ4_INDEX_PAIR]
    assert (c1 <= cap).all() and (c2 <= cap).all(), tag
    assert np.array_equal(c1, c2), (tag, np.nonzero(c1 != c2)[0][:8], c1[c1 != c2][:8], c2[c1 != c2][:8])
    live = np.arange(cap)[None, :] < c1[:, None]
    diff = (e1 != e2) & live
    assert not diff.any(), (tag, np.argwhere(diff)[:8])
    for i in walk:
        w = token_walk(items[i])
        k = min(len(w), cap)
        assert c2[i] == k, (tag, i, int(c2[i]), len(w), cap)
        assert np.array_equal(e2[i, :k], np.array(w[:k], np.uint16)), (tag, i)


_streams_cache = {}


def _streams(codec, dist, B, n):
    """n valid streams of synthetic blocks (the generator and the encoder on the device), made once per (dist, B)"""
    key = (dist, B)
    if key not in _streams_cache or len(_streams_cache[key]) < n:
        stride = (bound(METHOD_LZ4, B) + 127) & ~127
        bufs = [codec.alloc(n * B), codec.alloc(n * stride), codec.alloc(4 * n), codec.alloc(4 * n)]
        d_raw, d_comp, d_sz, d_st = bufs
        try:
            codec.synth_batch(11, 0, n, B, cc.DIST_NAMES.index(dist), d_raw)
            codec.compress_batch(METHOD_LZ4, 1, d_raw, B, B, n, d_comp, stride, d_sz, d_st)
            codec.sync()
            assert (d_st.download(dtype=np.int32) == 0).all()
            szs = d_sz.download(dtype=np.uint32)
            comp = d_comp.download().reshape(n, stride)
            _streams_cache[key] = [comp[i, :int(szs[i])].copy() for i in range(n)]
        finally:
            for b in bufs:
                b.free()
    return _streams_cache[key][:n]


# ---- test 1: the rows of the two forms ----
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("B", [4096, 131072])
@pytest.mark.parametrize("dist", DISTS)
def test_rows_equal_between_forms(codec, dist, B, n):
    items = _streams(codec, dist, B, NMAX)[:n]
    walk = sorted({0, n // 2, n - 1} | ({62, 63, 64} & set(range(n))))   # around the pair's last lane
    for packed in (False, True):
        _same_rows(codec, items, B, packed, walk, (dist, B, n, packed))


def test_rows_equal_1mib_blocks(codec):
    items = _streams(codec, "wide", 1 << 20, 4)
    for packed in (False, True):
        _same_rows(codec, items, 1 << 20, packed, [0, 3], ("wide", 1 << 20, 4, packed))


def test_rows_equal_on_crafted_streams(codec):
    B = 4096
    enc = lambda seqs, last: np.frombuffer(bytes(lz4_craft.encode(seqs, last, lit_seed=3)), np.uint8).copy()
    valid = [
        enc([(15 + 255 * 3 + 7, 1, 20), (5, 4, 8), (15 + 255 * 2, 9, 300)], 12),   # literal lengths through several 255s (state 1)
        enc([(3, 1, 8)], 50),                                                    # the last sequence is literals only ...
        enc([], 200),                                                            # ... and the only one
        enc([], 5),                                                              # fewer than 16 bytes
        enc([(1, 1, 4)] + [(0, 1, 4)] * 1500, 5),                                 # more tokens than a 4 KiB block's row holds
        enc([(2, 1, 600), (0, 3, 2000), (1, 2, 4)], 7),                           # match lengths through several 255s
        enc([(1, 1, 4)] + [(0, 1, 4), (2, 2, 5), (1, 1, 19)] * 200, 6),           # double tokens next to nibble-15 matches
    ]
    empty = np.zeros(0, np.uint8)                                                # csize == 0
    items = valid + [empty] + [m for _, m in lz4_craft.corpus(B, 56, 7)]
    assert len(token_walk(valid[4])) > codec.lz4_index_cap(B)
    for packed in (False, True):
        out, cap = _rows(codec, items, B, packed)
        assert out[cc.LZ4_INDEX_SINGLE][0][4] == cap and out[cc.LZ4_INDEX_PAIR][0][4] == cap   # both stop at the row's end
        assert out[cc.LZ4_INDEX_PAIR][0][len(valid)] == 0
        _same_rows(codec, items, B, packed, range(len(valid)), ("crafted", packed))


# ---- test 2: the public decode path on a paired index ----
class _Forced:
    def __init__(self, codec, waves=0):
        self.codec = codec
        self.opts = {cc.OPT_LZ4_DECODE_PATH: cc.LZ4_PATH_INDEXED, cc.OPT_LZ4_INDEX_WALKERS: 1,
                     cc.OPT_LZ4_INDEX_FORM: cc.LZ4_INDEX_PAIR, cc.OPT_LZ4_DECODE_WAVES: waves}

    def __enter__(self):
        self.saved = {k: self.codec.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.codec.set_option(k, v)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            self.codec.set_option(k, v)


def _decode_against_oracle(codec, oracle, items, B, tag):
    n = len(items)
    buf, offs, szs = _pack(items, True)
    bufs = [codec.alloc(buf.nbytes), codec.alloc(8 * n), codec.alloc(4 * n), codec.alloc(n * B), codec.alloc(4 * n)]
    d_src, d_off, d_sz, d_dst, d_st = bufs
    try:
        d_src.upload(buf); d_off.upload(offs); d_sz.upload(szs)
        d_dst.memset(0xA5); d_st.memset(0x7F)
        with _Forced(codec):
            codec.decompress_batch(METHOD_LZ4, d_src, d_off, d_sz, d_dst, B, B, n, d_st)
            codec.sync()
        st = d_st.download(dtype=np.int32)
        raw = d_dst.download().reshape(n, B)
    finally:
        for b in bufs:
            b.free()
    rejected = 0
    for i, m in enumerate(items):
        r, exp = oracle.lz4_decompress(m, B, fill=0xA5)
        assert st[i] in (cc.OK, cc.E_CORRUPT), (tag, i, int(st[i]))
        assert (st[i] == 0) == (r == B), (tag, i, int(st[i]), r, len(m))
        if r == B:
            assert np.array_equal(raw[i], exp), (tag, i)
        else:
            rejected += 1
    return rejected


def _mutants(items, rng, count):
    """flip or cut a valid stream at a token, inside a length run, in an offset, at the end"""
    toks_of = [token_walk(s, full=True) for s in items]
    runs_of = [np.nonzero((s[1:-1] == 255) & (s[2:] == 255))[0] + 1 for s in items]
    out = []
    for j in range(count):
        s = items[j % len(items)].copy()
        toks, runs = toks_of[j % len(items)], runs_of[j % len(items)]
        t = toks[int(rng.integers(0, len(toks)))]
        kind = j % 8
        if kind in (3, 4) and len(runs) == 0:
            kind = 2 + 4 * (kind - 3)            # a stream without a length run: cut it instead
        if kind == 0:
            s[t] ^= 0xF0                         # a token's literal nibble
        elif kind == 1:
            s[t] ^= 0x0F                         # a token's match nibble
        elif kind == 2:
            s = s[:t + 1]                        # cut behind a token
        elif kind == 3:
            s[int(runs[int(rng.integers(0, len(runs)))])] = 7      # inside a length run
        elif kind == 4:
            s = s[:int(runs[int(rng.integers(0, len(runs)))]) + 1]  # cut inside a length run
        elif kind == 5:
            q = min(t + 1 + (int(s[t]) >> 4), len(s) - 2)
            s[q] = 0; s[q + 1] = 0               # an offset (of a short literal run's sequence), made 0
        elif kind == 6:
            s = s[:len(s) - int(rng.integers(1, 6))]          # cut at the end
        else:
            s[len(s) - 1 - int(rng.integers(0, 4))] ^= 0x55   # flipped at the end
        out.append(s)
    return out


@pytest.mark.parametrize("B", [4096, 131072])
def test_decode_with_paired_index_matches_oracle(codec, oracle, B):
    valid = []
    for dist in DISTS:
        valid += _streams(codec, dist, B, NMAX)[:13]
    crafted = [m for _, m in lz4_craft.corpus(B, 64, 9)]
    rejected = _decode_against_oracle(codec, oracle, valid + crafted, B, ("valid+crafted", B))
    assert rejected > 0
    rng = np.random.default_rng([21, B])
    src = [_streams(codec, d, B, NMAX)[k] for d in DISTS for k in (0, 1, 2)]
    muts = _mutants(src, rng, 64)
    assert len(muts) == 64
    rejected = _decode_against_oracle(codec, oracle, muts, B, ("mutated", B))
    assert rejected >= 16      # the cut streams at least


# ---- test 3: both decoder forms on a paired index ----
def test_both_decoder_forms_on_a_paired_index(codec):
    B, n = 131072, 3000
    stride = (bound(METHOD_LZ4, B) + 127) & ~127
    bufs = [codec.alloc(n * B), codec.alloc(n * stride), codec.alloc(4 * n), codec.alloc(4 * n), codec.alloc(8 * n),
            codec.alloc(n * B), codec.alloc(8)]
    d_raw, d_comp, d_sz, d_st, d_off, d_out, d_mis = bufs
    try:
        codec.synth_batch(5, 0, n, B, cc.DIST_WIDE, d_raw)
        codec.compress_batch(METHOD_LZ4, 1, d_raw, B, B, n, d_comp, stride, d_sz, d_st)
        d_off.upload(np.arange(n, dtype=np.uint64) * np.uint64(stride))
        codec.sync()
        assert (d_st.download(dtype=np.int32) == 0).all()
        for waves in (1, 2):
            d_out.memset(0xA5); d_st.memset(0x7F); d_mis.memset(0)
            with _Forced(codec, waves):
                codec.decompress_batch(METHOD_LZ4, d_comp, d_off, d_sz, d_out, B, B, n, d_st)
            codec.compare_batch(d_raw, B, d_out, B, B, n, d_mis)
            codec.sync()
            assert (d_st.download(dtype=np.int32) == 0).all(), waves
            assert int(d_mis.download(dtype=np.uint64)[0]) == 0, waves
    finally:
        for b in bufs:
            b.free()


def test_index_form_option(codec):
    assert codec.get_option(cc.OPT_LZ4_INDEX_FORM) == 0
    for v in (1, 2, 0):
        codec.set_option(cc.OPT_LZ4_INDEX_FORM, v)
        assert codec.get_option(cc.OPT_LZ4_INDEX_FORM) == v
    with pytest.raises(cc.CryoError):
        codec.set_option(cc.OPT_LZ4_INDEX_FORM, 3)
    assert codec.get_option(cc.OPT_LZ4_INDEX_FORM) == 0
