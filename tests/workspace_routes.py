"""The route table of tests/test_gpu_workspace_history.py: one entry per way a call can go through a handle's device and
pinned memory.  An entry makes its call on inputs built once and gives back every output the call has (bytes, sizes, statuses,
rows, records, cells, totals); its check compares them with what the CPU oracle or the Python references say, never with an
earlier run of the code under test (segment mode, which promises the same bytes whatever the call, is also compared with its
own first run).  Inputs and expectations come from the existing builders and references: oracle_lib, lz4_craft, zstd_craft,
large_blocks, float_cases, scan_calls / truth_calls, fetch_ref, filter_ref, agg_ref, group_ref, project_ref, float_ref (which
stands on bytes_key_ref, set_key_ref and truth_key_ref), layout_ref and recode_ref.  Batches of three blocks and more hold a
truncated stream and one with trailing garbage, next to streams of very different sizes (zeros, random bytes).

A route names the entry points it calls, the values of the path options it runs under, and the handle's buffers it is known to
go through (keys of Codec.debug_fill's report): the test asserts that those were filled before the call and did not grow in it.
Test infrastructure only."""
import ctypes as C
import os
import re

import numpy as np

import agg_ref
import fetch_ref
import filter_ref
import float_cases as fc
import float_ref as fl
import group_ref
import large_blocks
import layout_ref
import lz4_craft
import project_ref
import recode_ref
import scan_calls
import truth_calls as tcall
import zstd_craft
from pg_cryogen_amd import METHOD_LZ4, METHOD_ZSTD, CryoError, codec as cc

SENTINEL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the options a route may set, and what they are when it leaves
DEFAULTS = {cc.OPT_LZ4_DECODE_PATH: 0, cc.OPT_LZ4_INDEX_WALKERS: 0, cc.OPT_LZ4_DECODE_WAVES: 0, cc.OPT_LZ4_INDEX_FORM: 0,
            cc.OPT_ZSTD_DECODE_PATH: 0, cc.OPT_WORKSPACE_MAX_BYTES: 0, cc.OPT_ENCODE_SEGMENT_BYTES: 0,
            cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY: 1, cc.OPT_ENCODE_VERIFY: 0, cc.OPT_ZSTD_CHECKSUM: 0,
            cc.OPT_PIPE_MIN_BYTES: 64 << 20}
# the values the library takes for the four path options: a copy by hand of include/cryo_codec.h, which the GPU test
# test_path_option_values_are_the_librarys holds against cryo_codec_set_option itself
PATH_OPTIONS = {cc.OPT_LZ4_DECODE_PATH: (0, 1, 2, 3), cc.OPT_ZSTD_DECODE_PATH: (0, 1, 2, 3), cc.OPT_LZ4_INDEX_FORM: (0, 1, 2),
                cc.OPT_LZ4_DECODE_WAVES: (0, 1, 2)}
AIDS = {"cryo_codec_synth_batch", "cryo_codec_checksum_batch", "cryo_codec_compare_batch"}   # test aids: no route of their own
HOST_IN = ("hb_src", "hb_meta", "pin")                      # what staging host streams goes through
HOST_IO = ("hb_src", "hb_dst", "hb_meta", "pin")
PIPE_PINS = ("pipe_pin0", "pipe_pin1", "pipe_pin2", "pipe_pin3")
# what Codec.debug_fill reports on: every handle-owned buffer but the keyed pool
FILL_KEYS = ("d_ws", "d_vfy", "d_rec", "hb_src", "hb_dst", "hb_meta", "d_in", "d_out", "d_scalars", "d_keytab", "pin") + PIPE_PINS
POOL_SLOTS = 256
GROUPS = ["lz4_decode_ring", "lz4_decode_indexed", "lz4_decode_few", "zstd_decode_fused", "zstd_decode_pipeline",
          "zstd_decode_tiles", "lz4_encode", "zstd_encode", "zstd_encode_lazy", "zstd_encode_btlazy2", "zstd_encode_optimal", "segment",
          "write_extras", "stored_codec", "stored_codec_chunked", "scan_int", "scan_keys", "scan_chunked", "pool"]


def lz4_ws(B, n=1, path=0, walkers=0):
    """whether an LZ4 decode of n blocks of B bytes goes through d_ws (lz4_decompress_workspace, lz4_dec.hip): the few-blocks
    path (up to 64 blocks and 64 MiB of 32 KiB .. 2 MiB each, asked for or automatic) and the sequence index do, the in-wave
    parser -- path 1, and the automatic choice below 16 KiB for batches below 24 576 blocks -- does not.  The passes that decode
    into handle workspace (verification, check, fetch, the scans, recode) and the host calls take the automatic choice"""
    if 1 <= n <= 64 and 32768 <= B <= (2 << 20) and n * B <= (64 << 20) and (path == 3 or (path == 0 and walkers == 0)):
        return ("d_ws",)
    if path == 1 or (path == 0 and B < 16384 and n < 24576):
        return ()
    return ("d_ws",)


def header_entry_points():
    """every cryo_codec_*_batch / cryo_codec_*_blocks* entry point include/cryo_codec.h declares, the test aids excepted"""
    text = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    return set(re.findall(r"\b(cryo_codec_\w+?_(?:batch|blocks(?:_to|_keyed)?))\(", text)) - AIDS


class Route:
    def __init__(self, group, name, run, check, entry, buffers=(), options=None, own_handle=False):
        self.group, self.name, self._run, self._check = group, name, run, check
        self.entry = {entry} if isinstance(entry, str) else set(entry)
        self.buffers, self.own_handle = tuple(buffers), own_handle
        self.options = dict(options or {})
        self.host = any(re.search(r"_blocks(_to|_keyed)?$", e) for e in self.entry)     # a host-buffer call
        self.state = {}                                     # what a check keeps from run to run (segment mode's first bytes)

    def path_options(self):
        """the values of the four path options this route runs under (what it does not set is 0)"""
        return {o: self.options.get(o, 0) for o in PATH_OPTIONS}

    def run(self, codec):
        for o, v in self.options.items():
            codec.set_option(o, v)
        try:
            return self._run(codec)
        finally:
            for o in self.options:
                codec.set_option(o, DEFAULTS[o])

    def check(self, got, what=""):
        self._check(got, self.state, (self.group, self.name, what))

    def go(self, codec, what=""):
        self.check(self.run(codec), what)


# ---- inputs ----
def encode(oracle, method, raw, param=1):
    return oracle.lz4_compress(raw, param) if method == METHOD_LZ4 else oracle.zstd_compress(raw, param)


def decode(oracle, method, comp, B):
    """the oracle's verdict and bytes: the block, or None where it does not decode to exactly B bytes"""
    return layout_ref.decode(oracle, method, comp, B)


def hurt(comps):
    """a batch of three streams and more gets a truncated one and one with trailing garbage"""
    out = [np.asarray(c, np.uint8) for c in comps]
    if len(out) >= 3:
        out[1] = out[1][:max(1, len(out[1]) - 3)].copy()
        out[len(out) // 2 + 1] = np.concatenate([out[len(out) // 2 + 1], np.array([0x5A, 0x00, 0xC3], np.uint8)])
    return out


def synth_mix(oracle, B, n, seed):
    """blocks of every size class: wide, narrow, int4, random (stored as literals), zeros (a few bytes)"""
    return [oracle.synth(seed, i, B, i % 5) for i in range(n)]


def payload_blocks(oracle, B):
    """the three blocks of an encode call: compressible text, 2-bit noise, random bytes"""
    rng = np.random.default_rng([7, B])
    return [large_blocks.text_noise(B), rng.integers(0, 4, B, dtype=np.uint8), large_blocks.incompressible(B)]


# ---- device-resident calls ----
class Dev:
    """device buffers of one call, freed on exit"""

    def __init__(self, codec):
        self.codec, self.bufs = codec, []

    def alloc(self, nbytes, fill=None):
        b = self.codec.alloc(max(int(nbytes), 16))
        self.bufs.append(b)
        if fill is not None:
            b.memset(fill)
        return b

    def put(self, arr):
        b = self.alloc(arr.nbytes)
        b.upload(arr)
        return b

    def streams(self, comps, odd=False):
        """(src, off, size) of a stream table: 16-byte aligned items, or -- odd -- every item at an odd offset"""
        n = len(comps)
        offs, szs = np.zeros(n, np.uint64), np.array([len(c) for c in comps], np.uint32)
        pos = 1 if odd else 0
        for i, c in enumerate(comps):
            offs[i] = pos
            pos += len(c)
            pos = (pos + 1) | 1 if odd else (pos + 15) & ~15
        packed = np.full(pos + 64, 0x33, np.uint8)
        for i, c in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + len(c)] = c
        return self.put(packed), self.put(offs), self.put(szs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def decompress_batch(codec, method, comps, B):
    """cryo_codec_decompress_batch on streams at odd offsets, dst_stride = B + 256 over a sentinel: (statuses, rows of B + 256)"""
    n, S = len(comps), B + 256
    with Dev(codec) as d:
        src, off, sz = d.streams(comps, odd=True)
        dst, st = d.alloc(n * S, SENTINEL), d.alloc(4 * n, 0x7F)
        codec.decompress_batch(method, src, off, sz, dst, S, B, n, st)
        codec.sync()
        return st.download(4 * n, dtype=np.int32).copy(), dst.download(n * S).reshape(n, S).copy()


def same_decode(got, want, what):
    st, rows = got
    B = rows.shape[1] - 256
    assert (rows[:, B:] == SENTINEL).all(), (what, "a byte beyond a block was written", np.flatnonzero((rows[:, B:] != SENTINEL).any(axis=1))[:5])
    for i, w in enumerate(want):
        assert st[i] == (cc.OK if w is not None else cc.E_CORRUPT), (what, i, int(st[i]), w is None)
        if w is not None:
            diff = np.flatnonzero(rows[i, :B] != w)
            assert diff.size == 0, (what, i, "first differing byte", int(diff[0]))


def compress_batch(codec, method, param, blocks):
    """cryo_codec_compress_batch: (statuses, sizes, slots); the slots are filled with a sentinel first"""
    n, B = len(blocks), len(blocks[0])
    cap = cc.bound(method, B)
    with Dev(codec) as d:
        src = d.put(np.concatenate(blocks))
        dst, sz, st = d.alloc(n * cap, SENTINEL), d.alloc(4 * n, 0x7F), d.alloc(4 * n, 0x7F)
        codec.compress_batch(method, param, src, B, B, n, dst, cap, sz, st)
        codec.sync()
        return st.download(4 * n, dtype=np.int32).copy(), sz.download(4 * n, dtype=np.uint32).copy(), dst.download(n * cap).reshape(n, cap).copy()


def compress_host(codec, method, param, blocks):
    """cryo_codec_compress_blocks: (statuses -- all 0 when the call returns --, sizes, slots)"""
    n, B = len(blocks), len(blocks[0])
    cap = cc.bound(method, B)
    src = np.concatenate(blocks)
    dst, sz = np.full(n * cap, SENTINEL, np.uint8), np.full(n, 0x7F7F7F7F, np.uint32)
    codec._chk(codec.L.cryo_codec_compress_blocks(codec.h, method, param, src.ctypes.data, B, n, dst.ctypes.data, cap, sz.ctypes.data),
               "compress_blocks")
    return np.zeros(n, np.int32), sz, dst.reshape(n, cap)


def same_streams(got, want, what):
    """statuses, sizes and the streams' bytes.  What lies behind a stream inside its slot is not looked at: a slot is
    cryo_codec_bound bytes, and include/cryo_codec.h lets an encoder write all of it ("the whole slot (up to bound bytes) may be
    written, only the first h_out_size[i] bytes are meaningful")"""
    st, sz, slots = got
    assert (st == 0).all(), (what, st)
    for i, w in enumerate(want):
        assert int(sz[i]) == len(w) and np.array_equal(slots[i, :len(w)], w), (what, i, int(sz[i]), len(w))


def decompress_host(codec, method, comps, B, each=False):
    """cryo_codec_decompress_blocks, or -- each -- _blocks_to with one destination per block: (statuses, rows of B)"""
    n = len(comps)
    src = (C.c_void_p * n)(*[c.ctypes.data for c in comps])
    szs = (C.c_uint32 * n)(*[c.nbytes for c in comps])
    rows, st = np.full((n, B), SENTINEL, np.uint8), np.full(n, 0x7F7F7F7F, np.int32)
    if each:
        dst = (C.c_void_p * n)(*[rows[i].ctypes.data for i in range(n)])
        codec._chk(codec.L.cryo_codec_decompress_blocks_to(codec.h, method, src, szs, n, dst, B, st.ctypes.data), "decompress_blocks_to")
    else:
        codec._chk(codec.L.cryo_codec_decompress_blocks(codec.h, method, src, szs, n, rows.ctypes.data, B, st.ctypes.data), "decompress_blocks")
    return st, rows


def same_decode_host(got, want, what, untouched):
    st, rows = got
    for i, w in enumerate(want):
        assert st[i] == (cc.OK if w is not None else cc.E_CORRUPT), (what, i, int(st[i]))
        if w is not None:
            assert np.array_equal(rows[i], w), (what, i)
        elif untouched:
            assert (rows[i] == SENTINEL).all(), (what, i, "a rejected block's destination was written")


def check_batch(codec, method, comps, B):
    n = len(comps)
    with Dev(codec) as d:
        src, off, sz = d.streams(comps)
        res = d.alloc(8 * n, 0xEE)
        codec.check_batch(method, src, off, sz, B, n, res)
        codec.sync()
        return res.download(8 * n, dtype=np.uint32).reshape(n, 2).copy()


def fetch_batch(codec, method, comps, B, requests):
    n = len(comps)
    first, pos = cc.request_table(requests)
    n_req = int(first[-1])
    with Dev(codec) as d:
        src, off, sz = d.streams(comps)
        d_first, d_pos = d.put(first), d.put(pos if n_req else np.zeros(8, np.uint16))
        dst, res, tot = d.alloc(n * B + 64, SENTINEL), d.alloc(16 * max(n_req, 1), 0xEE), d.alloc(8, 0xEE)
        codec.fetch_batch(method, src, off, sz, B, n, d_first, d_pos, n_req, dst, n * B, res, tot)
        codec.sync()
        return (res.download(dtype=np.uint8)[:16 * n_req].view(cc.FETCH_RESULT).copy(), dst.download(),
                int(tot.download(8, dtype=np.uint64)[0]))


def same_fetch(got, want, what):
    recs, dst, total = got
    erecs, packed, etotal = want
    assert recs.size == erecs.size and total == etotal, (what, recs.size, erecs.size, total, etotal)
    for f in ("status", "len", "off"):
        bad = np.flatnonzero(recs[f] != erecs[f])
        assert bad.size == 0, (what, f, [(int(i), tuple(recs[i]), tuple(erecs[i])) for i in bad[:5]])
    diff = np.flatnonzero(dst[:etotal] != packed)
    assert diff.size == 0, (what, "first differing byte", int(diff[0]))
    assert (dst[etotal:] == SENTINEL).all(), (what, "a byte at or beyond the total was written")


def recode_batch(codec, src_method, comps, B, dst_method, param):
    n, cap = len(comps), (cc.bound(dst_method, B) + 15) & ~15
    with Dev(codec) as d:
        src, off, sz = d.streams(comps)
        dst, osz, st = d.alloc(n * cap, SENTINEL), d.alloc(4 * n, 0x7F), d.alloc(4 * n, 0x7F)
        codec.recode_batch(src_method, src, off, sz, B, n, dst_method, param, dst, cap, osz, st)
        codec.sync()
        return st.download(4 * n, dtype=np.int32).copy(), osz.download(4 * n, dtype=np.uint32).copy(), dst.download(n * cap).reshape(n, cap).copy()


def same_recode_batch(got, want, what, bound):
    """statuses, sizes (0 unless the status is OK) and the streams' bytes; a slot's bytes behind the bound are the sentinel's
    (within the bound the tail is the encoder's to write, as for same_streams)"""
    st, sz, slots = got
    assert (slots[:, bound:] == SENTINEL).all(), (what, "a byte behind a slot's bound was written")
    for i, w in enumerate(want):
        assert st[i] == (cc.OK if w is not None else cc.E_CORRUPT), (what, i, int(st[i]))
        if w is None:
            assert int(sz[i]) == 0, (what, i, "a rejected block has a size", int(sz[i]))
        else:
            assert int(sz[i]) == len(w) and np.array_equal(slots[i, :len(w)], w), (what, i, int(sz[i]), len(w))


def same_recode_host(got, want, what):
    outs, st, off, sz, dst = got
    esz, eoff, total = recode_ref.pack_offsets([0 if w is None else len(w) for w in want], [0 if w is not None else cc.E_CORRUPT for w in want])
    for i, w in enumerate(want):
        assert st[i] == (cc.OK if w is not None else cc.E_CORRUPT), (what, i, int(st[i]))
        assert int(sz[i]) == esz[i] and (w is None or int(off[i]) == eoff[i]), (what, i, int(sz[i]), esz[i], int(off[i]), eoff[i])
        if w is not None:
            assert np.array_equal(outs[i], w), (what, i)
    assert (dst[total:] == SENTINEL).all(), (what, "a byte beyond the packed streams was written")


def verify_batch(codec, method, raws, comps):
    n, B = len(raws), len(raws[0])
    with Dev(codec) as d:
        raw = d.put(np.concatenate(raws))
        src, off, sz = d.streams(comps)
        st, first = d.alloc(4 * n, 0x7F), d.alloc(4 * n, 0x7F)
        codec.verify_batch(method, raw, B, B, n, src, off, sz, st, first)
        codec.sync()
        return st.download(4 * n, dtype=np.int32).copy(), first.download(4 * n, dtype=np.uint32).copy()


# ---- the table ----
class Table:
    """routes by group, built when first asked for (the references run in Python) and kept"""

    def __init__(self, oracle, stock):
        self.oracle, self.stock, self.built = oracle, stock, {}
        self.enc = scan_calls.Encoder(oracle)
        self._corpus, self._streams = None, {}

    def once(self, key, make):
        """inputs and the oracle's reading of them are made once and shared by the routes that take them, unchanged"""
        if key not in self._streams and make is None:
            self.all()
        if key not in self._streams:
            self._streams[key] = make()
        return self._streams[key]

    def group(self, name):
        if name not in self.built:
            self.built[name] = list(getattr(self, "_" + name)())
            assert self.built[name] and all(r.group == name for r in self.built[name]), name
        return self.built[name]

    def all(self):
        return [r for g in GROUPS for r in self.group(g)]

    # -- LZ4 decode --
    def lz4_streams(self, B, n):
        """n streams of a block size with what the oracle makes of each: oracle streams of every size class, crafted streams
        (tests/lz4_craft.py: boundary lengths, ends on the decoder's rules, truncations) and the two hurt ones"""
        crafted = [m for _, m in lz4_craft.corpus(B, 3, 11 + n)] if n >= 5 else []
        raws = synth_mix(self.oracle, B, n - len(crafted), 21 + n)
        comps = hurt([encode(self.oracle, METHOD_LZ4, r, 1 + 6 * (i % 2)) for i, r in enumerate(raws)] + crafted)
        return comps, [decode(self.oracle, METHOD_LZ4, c, B) for c in comps]

    def lz4_route(self, group, B, n, opts):
        buffers = lz4_ws(B, n, opts.get(cc.OPT_LZ4_DECODE_PATH, 0), opts.get(cc.OPT_LZ4_INDEX_WALKERS, 0))
        comps, want = self.once(("lz4", B, n), lambda: self.lz4_streams(B, n))
        assert n < 3 or (any(w is None for w in want) and any(w is not None for w in want)), (B, n)
        name = "B%d n%d %s" % (B, n, " ".join("%d=%d" % kv for kv in sorted(opts.items())))
        return Route(group, name, lambda c: decompress_batch(c, METHOD_LZ4, comps, B), lambda got, s, what: same_decode(got, want, what),
                     "cryo_codec_decompress_batch", buffers, opts)

    def _lz4_decode_ring(self):
        for B in (4096, 32768, 140000):
            for n in (1, 5, 70):
                yield self.lz4_route("lz4_decode_ring", B, n, {cc.OPT_LZ4_DECODE_PATH: 1})
        for B, n in ((4096, 70), (32768, 5), (140000, 1)):
            yield self.lz4_route("lz4_decode_ring", B, n, {cc.OPT_LZ4_DECODE_PATH: 0})    # automatic: the parser, the few-blocks path twice

    def _lz4_decode_indexed(self):
        """walkers 1, 4, 64; with one walker both index forms; one wave and two per block: the eight combinations at every block
        size, the batch sizes 1, 5, 70 going round"""
        combos = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (4, 0, 1), (4, 0, 2), (64, 0, 1), (64, 0, 2)]
        for bi, B in enumerate((4096, 32768, 140000)):
            for ci, (walkers, form, waves) in enumerate(combos):
                opts = {cc.OPT_LZ4_DECODE_PATH: 2, cc.OPT_LZ4_INDEX_WALKERS: walkers, cc.OPT_LZ4_INDEX_FORM: form,
                        cc.OPT_LZ4_DECODE_WAVES: waves}
                yield self.lz4_route("lz4_decode_indexed", B, (1, 5, 70)[(ci + bi) % 3], opts)

    def _lz4_decode_few(self):
        for B in (32768, 140000):
            for n in (1, 5):
                yield self.lz4_route("lz4_decode_few", B, n, {cc.OPT_LZ4_DECODE_PATH: 3})
            yield self.lz4_route("lz4_decode_few", B, 70, {cc.OPT_LZ4_DECODE_PATH: 3})            # more than 64: the index instead
        yield self.lz4_route("lz4_decode_few", 4096, 5, {cc.OPT_LZ4_DECODE_PATH: 3})              # below 32 KiB: the index instead

    # -- zstd decode --
    def corpus(self):
        """tests/zstd_craft.py's non-default frames by block size: {B: [frame]} of the unmutated ones"""
        if self._corpus is None:
            self._corpus = {}
            for name, B, f in zstd_craft.zstd_corpus(self.stock, self.oracle, 5):
                if not name.startswith("mutated"):
                    self._corpus.setdefault(B, {}).setdefault(name.split("/")[0], f)
        return self._corpus

    def zstd_streams(self, B, n):
        """n frames of a block size: levels 1, 5 and 19 going round over every size class, with and without a content checksum,
        one irregular frame (what the planner hands to the fused kernel: many small blocks, no content size, a skippable frame
        in front), one whose checksum is of other data, and the two hurt ones"""
        import oracle_lib as ol
        raws = synth_mix(self.oracle, B, n, 31 + n)
        comps = []
        for i, r in enumerate(raws):
            lvl = (1, 5, 19)[i % 3]
            if i % 4 == 3:
                comps.append(self.stock.zstd_compress2(r, {ol.ZSTD_C_COMPRESSION_LEVEL: lvl, ol.ZSTD_C_CHECKSUM_FLAG: 1}))
            else:
                comps.append(self.oracle.zstd_compress(r, lvl))
        if n >= 5:
            by_name = self.corpus().get(B, {})
            odd = [by_name[k] for k in ("target64", "no_content_size", "few_sequences", "checksum_of_other_data") if k in by_name]
            skippable = np.frombuffer((0x184D2A50).to_bytes(4, "little") + (5).to_bytes(4, "little") + b"cryo!", np.uint8)
            odd.append(np.concatenate([skippable, comps[0]]))
            odd.append(large_blocks.drop_content_size(comps[0], B))
            for k, f in enumerate(odd[:n - 3]):
                comps[len(comps) - 1 - k] = np.asarray(f, np.uint8)
        comps = hurt(comps)
        return comps, [decode(self.oracle, METHOD_ZSTD, c, B) for c in comps]

    def zstd_route(self, group, B, n, opts, own_handle=False):
        comps, want = self.once(("zstd", B, n), lambda: self.zstd_streams(B, n))
        assert n < 3 or (any(w is None for w in want) and any(w is not None for w in want)), (B, n)
        name = "B%d n%d %s" % (B, n, " ".join("%d=%d" % kv for kv in sorted(opts.items())))
        return Route(group, name, lambda c: decompress_batch(c, METHOD_ZSTD, comps, B), lambda got, s, what: same_decode(got, want, what),
                     "cryo_codec_decompress_batch", ("d_ws",), opts, own_handle)

    def _zstd_decode_fused(self):
        for B in (4096, 32768, 140000):
            for n in (1, 5, 70):
                yield self.zstd_route("zstd_decode_fused", B, n, {cc.OPT_ZSTD_DECODE_PATH: 1})

    def _zstd_decode_pipeline(self):
        """automatic, the pipeline (byte-parallel execution for up to 64 frames of 32 KiB and more), the pipeline without it"""
        for B in (4096, 32768, 140000):
            for n in (1, 5, 70):
                for path in (0, 2, 3):
                    yield self.zstd_route("zstd_decode_pipeline", B, n, {cc.OPT_ZSTD_DECODE_PATH: path})

    def _zstd_decode_tiles(self):
        """304 frames of 4 KiB under a workspace cap below one tile of the planner's smallest size: make_layout (zstd_pipe.hip)
        never plans fewer than 16 frames a tile, zstd_decompress_workspace then asks for one lane, so the call runs 19 tiles one
        after the other in the workspace of the first.  On a handle of its own: the launcher sizes its tiles by the workspace it
        is handed, and a workspace another route has grown would hold the whole call in one tile"""
        yield self.zstd_route("zstd_decode_tiles", 4096, 304, {cc.OPT_ZSTD_DECODE_PATH: 2, cc.OPT_WORKSPACE_MAX_BYTES: 1}, own_handle=True)

    # -- encode --
    def encode_route(self, group, method, param, B, host=False, opts=None, want=None, tag=""):
        blocks = payload_blocks(self.oracle, B)
        want = want or [encode(self.oracle, method, b, param) for b in blocks]
        call = compress_host if host else compress_batch
        verified = bool((opts or {}).get(cc.OPT_ENCODE_VERIFY))
        buffers = (HOST_IO if host else ()) + (("d_vfy",) if verified else ())
        buffers += ("d_ws",) if method == METHOD_ZSTD else (lz4_ws(B, len(blocks)) if verified else ())
        name = "%s %d B%d%s%s" % ("lz4" if method == METHOD_LZ4 else "zstd", param, B, " host" if host else "", tag)
        return Route(group, name, lambda c: call(c, method, param, blocks), lambda got, s, what: same_streams(got, want, what),
                     "cryo_codec_compress_blocks" if host else "cryo_codec_compress_batch", buffers, opts)

    def _lz4_encode(self):
        for B in (4096, 65546, 65547, 140000):
            yield self.encode_route("lz4_encode", METHOD_LZ4, 1, B)
        yield self.encode_route("lz4_encode", METHOD_LZ4, 1, 65547, host=True)

    def _zstd_encode(self):
        """one level per finder, at a block of one zstd block and at one of two: fast (-5, 1), dfast (3), greedy (5) here; lazy (7),
        lazy2 (9) and btlazy2 (13) in groups of their own, which take longer; the optimal parsers below"""
        for level in (-5, 1, 3, 5):
            for B in (20000, 140000):
                yield self.encode_route("zstd_encode", METHOD_ZSTD, level, B)
        yield self.encode_route("zstd_encode", METHOD_ZSTD, 3, 20000, host=True)

    def _zstd_encode_lazy(self):
        for level in (7, 9):
            for B in (20000, 140000):
                yield self.encode_route("zstd_encode_lazy", METHOD_ZSTD, level, B)

    def _zstd_encode_btlazy2(self):
        for B in (20000, 140000):
            yield self.encode_route("zstd_encode_btlazy2", METHOD_ZSTD, 13, B)

    def _zstd_encode_optimal(self):
        """btopt (16), btultra (19), btultra2 (22) at 20 000 bytes.  At 140 000 the three levels take 7 s a run on the MI355X
        (34 s for the five runs of the filled-workspace test): left out"""
        for level in (16, 19, 22):
            yield self.encode_route("zstd_encode_optimal", METHOD_ZSTD, level, 20000)

    def _segment(self):
        """B = 70 000 in segments of 4 KiB and 16 KiB (a partial last one): LZ4, and zstd with the strategy cap at 1, 2, 4 and 6
        at the level whose strategy at this size is the cap (1 fast, 3 dfast, 6 lazy, 11 btlazy2: zstd_enc.hip's table).  The
        oracle's decoders (pinned to liblz4 / libzstd) give back the input, the size is within the bound, and the bytes are
        those of the route's first run"""
        B = 70000
        blocks = payload_blocks(self.oracle, B)

        def route(method, param, S, cap):
            opts = {cc.OPT_ENCODE_SEGMENT_BYTES: S, cc.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY: cap}

            def check(got, state, what):
                st, sz, slots = got
                assert (st == 0).all(), (what, st)
                for i, b in enumerate(blocks):
                    assert 0 < int(sz[i]) <= cc.bound(method, B), (what, i, int(sz[i]))
                    out = decode(self.oracle, method, slots[i, :int(sz[i])], B)
                    assert out is not None and np.array_equal(out, b), (what, i, "the stock decoder does not give back the input")
                    assert (slots[i, cc.bound(method, B):] == SENTINEL).all(), (what, i)
                streams = [slots[i, :int(sz[i])].copy() for i in range(len(blocks))]
                first = state.setdefault("streams", streams)
                assert all(np.array_equal(a, b) for a, b in zip(streams, first)), (what, "not the bytes of the first run")
            name = "%s %d S%d cap%d" % ("lz4" if method == METHOD_LZ4 else "zstd", param, S, cap)
            return Route("segment", name, lambda c: compress_batch(c, method, param, blocks), check, "cryo_codec_compress_batch", ("d_ws",), opts)
        for S in (4096, 16384):
            yield route(METHOD_LZ4, 1, S, 1)
            for cap, level in ((1, 1), (2, 3), (4, 6), (6, 11)):
                yield route(METHOD_ZSTD, level, S, cap)

    def _write_extras(self):
        """write verification and content checksums on top of a device and a host encode; cryo_codec_verify_batch on streams of
        which one is another block's, one decodes to the block with one byte changed, and one is truncated"""
        import oracle_lib as ol
        on = {cc.OPT_ENCODE_VERIFY: 1, cc.OPT_ZSTD_CHECKSUM: 1}
        for B, host in ((20000, False), (140000, True)):
            want = [self.stock.zstd_compress2(b, {ol.ZSTD_C_COMPRESSION_LEVEL: 3, ol.ZSTD_C_CHECKSUM_FLAG: 1}) for b in payload_blocks(self.oracle, B)]
            yield self.encode_route("write_extras", METHOD_ZSTD, 3, B, host, on, want, " verified, checksummed")
        yield self.encode_route("write_extras", METHOD_LZ4, 1, 140000, False, on, None, " verified")
        for method in (METHOD_LZ4, METHOD_ZSTD):
            B = 32768
            raws = synth_mix(self.oracle, B, 6, 41)
            comps = [encode(self.oracle, method, r) for r in raws]
            bent = raws[2].copy()
            bent[12345] ^= 0x40
            comps[2] = encode(self.oracle, method, bent)                    # decodes, to other bytes: first mismatch at 12345
            comps[4] = comps[4][:len(comps[4]) - 5].copy()                   # does not decode
            comps[5] = comps[0]                                              # another block's stream
            assert decode(self.oracle, method, comps[4], B) is None
            est = np.array([0, 0, cc.E_VERIFY, 0, cc.E_VERIFY, cc.E_VERIFY], np.int32)
            efirst = np.array([cc.VERIFY_NONE, cc.VERIFY_NONE, 12345, cc.VERIFY_NONE, cc.VERIFY_NONE,
                               int(np.flatnonzero(raws[5] != raws[0])[0])], np.uint32)

            def check(got, state, what, est=est, efirst=efirst):
                assert np.array_equal(got[0], est) and np.array_equal(got[1], efirst), (what, got[0], got[1])
            yield Route("write_extras", "verify_batch method %d" % method, lambda c, m=method, r=raws, s=comps: verify_batch(c, m, r, s), check,
                        "cryo_codec_verify_batch", ("d_vfy",) + (("d_ws",) if method == METHOD_ZSTD else lz4_ws(B, len(comps))))

    # -- stored blocks: check, recode, fetch --
    def stored(self, method, B):
        return self.once(("stored", method, B), lambda: self.stored_streams(method, B))

    def stored_streams(self, method, B):
        """(streams, what the oracle decodes them to): tuple blocks of tests/float_cases.py, oracle blocks of two size classes, a
        block of zeros (no header), and the two hurt streams"""
        blocks = (fc.random_blocks(4, 3 + B) if B == fc.B else [fc.sized_block(n, n) for n in (1, 64, 65, 290)])
        blocks = blocks + [self.oracle.synth(51, 1, B, 1), self.oracle.synth(51, 3, B, 3), np.zeros(B, np.uint8), blocks[0]]
        comps = hurt([self.enc(method, b) for b in blocks])
        return comps, [decode(self.oracle, method, c, B) for c in comps]

    def _stored_routes(self, group, opts):
        for method in (METHOD_LZ4, METHOD_ZSTD):
            for B in (4096, 32768):
                comps, dec = self.stored(method, B)
                chunk = 1 if opts.get(cc.OPT_WORKSPACE_MAX_BYTES) else len(comps)      # blocks a decode of the pass takes at once
                zs = ("d_ws",) if method == METHOD_ZSTD else lz4_ws(B, chunk)
                tag = "method %d B%d" % (method, B)
                verdicts = np.array([layout_ref.check_block(b) if b is not None else (layout_ref.STREAM, layout_ref.NONE) for b in dec], np.uint32)
                assert {layout_ref.OK, layout_ref.STREAM, layout_ref.HEADER} <= set(verdicts[:, 0].tolist()), verdicts

                def same_check(got, state, what, verdicts=verdicts):
                    bad = np.flatnonzero((got != verdicts).any(axis=1))
                    assert bad.size == 0, (what, [(int(i), tuple(got[i]), tuple(verdicts[i])) for i in bad[:5]])
                yield Route(group, "check_batch " + tag, lambda c, m=method, s=comps, B=B: check_batch(c, m, s, B), same_check,
                            "cryo_codec_check_batch", ("d_vfy",) + zs, opts)
                yield Route(group, "check_blocks " + tag, lambda c, m=method, s=comps, B=B: c.check_blocks(m, s, B), same_check,
                            "cryo_codec_check_blocks", ("d_vfy",) + HOST_IN + zs, opts)
                requests = [[1, 2, 3], [1], [], [1, 64, 65, 290], list(range(1, 40)), [2, 1], [1], [1, 5], [1], [3]][:len(comps)]
                fwant = fetch_ref.fetch_call(dec, requests)
                yield Route(group, "fetch_batch " + tag, lambda c, m=method, s=comps, B=B, q=requests: fetch_batch(c, m, s, B, q),
                            lambda got, state, what, w=fwant: same_fetch(got, w, what), "cryo_codec_fetch_batch", ("d_vfy",) + zs, opts)
                yield Route(group, "fetch_blocks " + tag,
                            lambda c, m=method, s=comps, B=B, q=requests: c.fetch_blocks(m, s, B, q, dst=np.full(len(s) * B, SENTINEL, np.uint8)),
                            lambda got, state, what, w=fwant: same_fetch(got, w, what), "cryo_codec_fetch_blocks", ("d_vfy",) + HOST_IN + zs, opts)
                to, param = (METHOD_ZSTD, 3) if method == METHOD_LZ4 else (METHOD_LZ4, 1)
                rwant = [None if b is None else encode(self.oracle, to, b, param) for b in dec]
                rbuf = ("d_rec", "d_ws")
                yield Route(group, "recode_batch " + tag, lambda c, m=method, s=comps, B=B, to=to, p=param: recode_batch(c, m, s, B, to, p),
                            lambda got, state, what, w=rwant, bd=cc.bound(to, B): same_recode_batch(got, w, what, bd), "cryo_codec_recode_batch", rbuf, opts)
                yield Route(group, "recode_blocks " + tag,
                            lambda c, m=method, s=comps, B=B, to=to, p=param: c.recode_blocks(
                                m, s, B, to, p, dst=np.full(len(s) * ((cc.bound(to, B) + 15) & ~15), SENTINEL, np.uint8)),
                            lambda got, state, what, w=rwant: same_recode_host(got, w, what), "cryo_codec_recode_blocks", rbuf + ("hb_src", "pin"), opts)

    def _stored_codec(self):
        """check, fetch and recode (LZ4 -> zstd 3, zstd -> LZ4), device-resident and host-buffer form, plus the host decodes"""
        yield from self._stored_routes("stored_codec", {})
        for method in (METHOD_LZ4, METHOD_ZSTD):
            comps, dec = self.stored(method, 32768)
            for each in (False, True):
                yield Route("stored_codec", "decompress_blocks%s method %d" % ("_to" if each else "", method),
                            lambda c, m=method, s=comps, e=each: decompress_host(c, m, s, 32768, e),
                            lambda got, state, what, w=dec, e=each: same_decode_host(got, w, what, e),
                            "cryo_codec_decompress_blocks_to" if each else "cryo_codec_decompress_blocks",
                            HOST_IO + (("d_ws",) if method == METHOD_ZSTD else lz4_ws(32768, len(comps))))
        # host calls of 128 blocks and more cut into pipelined chunks (CRYO_OPT_PIPE_MIN_BYTES = 0: whatever their size): the four
        # pinned staging buffers and the transfer stream
        piped = {cc.OPT_PIPE_MIN_BYTES: 0}
        raws = synth_mix(self.oracle, 4096, 130, 55)
        for method in (METHOD_LZ4, METHOD_ZSTD):
            comps = hurt([self.enc(method, r) for r in raws])
            dec = [decode(self.oracle, method, c, 4096) for c in comps]
            yield Route("stored_codec", "decompress_blocks pipelined method %d" % method, lambda c, m=method, s=comps: decompress_host(c, m, s, 4096),
                        lambda got, state, what, w=dec: same_decode_host(got, w, what, False), "cryo_codec_decompress_blocks",
                        HOST_IO + PIPE_PINS, piped)
            want = [self.enc(method, r) for r in raws]
            yield Route("stored_codec", "compress_blocks pipelined method %d" % method, lambda c, m=method: compress_host(c, m, 1, raws),
                        lambda got, state, what, w=want: same_streams(got, w, what), "cryo_codec_compress_blocks", HOST_IO + PIPE_PINS, piped)
        # the single-block calls: the handle's d_in / d_out scratch and its three scalar words
        raw = self.oracle.synth(61, 0, 32768, 0)
        for method in (METHOD_LZ4, METHOD_ZSTD):
            comp = encode(self.oracle, method, raw)

            def single(c, m=method, comp=comp):
                return c.compress_block(m, 1, raw), c.decompress_block(m, comp, 32768), c.decompress_block(m, comp[:-3], 32768)

            def same_single(got, state, what, comp=comp):
                assert np.array_equal(got[0], comp) and np.array_equal(got[1], raw) and got[2] is None, what
            yield Route("stored_codec", "single block method %d" % method, single, same_single, (), ("d_in", "d_out", "d_scalars"))

    def _stored_codec_chunked(self):
        """the same calls with so little workspace allowed that decode_pass takes one block per chunk: every chunk after the
        first runs in the side arrays, the stream tables and the decoded rows the chunk before left"""
        yield from self._stored_routes("stored_codec_chunked", {cc.OPT_WORKSPACE_MAX_BYTES: 1})

    # -- the four scans --
    INT_KEYS = [(1, fl.INT4, fl.GE, 3), (6, fl.INT8, fl.LE, 150)]
    INT_COLS = [(6, fl.INT8), (1, fl.INT4), (7, fl.INT2)]
    MIX_KEYS = [(2, fl.FLOAT8, fl.GT, 1.0), (4, fl.BYTES, fl.EQ, b"n"), (6, fl.INT8, fl.IN, [0, 7, 99, 1, 2, 3, 4, 5, -1, -2, -3])]
    MIX_TRUTH = fl.tr.dnf([1, 6], 3)                         # x > 1 OR (name = 'n' AND k IN (eleven members))
    MIX_COLS = fc.SIZED_COLS                                  # float8, float4, int8, float4 on (4, 8)
    BY = fc.SIZED_BY
    PCOLS = [2, 1, 3, 5]

    def _scan_routes(self, group, mixed, opts, sizes=(4096, 32768)):
        atts = fc.ATTS
        keys, W, cols = (self.MIX_KEYS, self.MIX_TRUTH, self.MIX_COLS) if mixed else (self.INT_KEYS, None, self.INT_COLS)
        for B in sizes:
            dec_by_method = {m: self.stored(m, B) for m in (METHOD_LZ4, METHOD_ZSTD)}
            dec = dec_by_method[METHOD_LZ4][1]
            assert all((a is None) == (b is None) and (a is None or np.array_equal(a, b)) for a, b in zip(dec, dec_by_method[METHOD_ZSTD][1]))
            if mixed:
                want = {"filter": fl.filter_call(dec, atts, keys, 0, W), "count": fl.filter_call(dec, atts, keys, fl.COUNT_ONLY, W),
                        "agg": fl.agg_call(dec, atts, keys, cols, W), "group": fl.group_call(dec, atts, keys, self.BY, cols, W),
                        "project": fl.project_call(dec, atts, keys, self.PCOLS, W)}
            else:
                want = {"filter": filter_ref.filter_call(dec, atts, keys), "count": filter_ref.filter_call(dec, atts, keys, filter_ref.COUNT_ONLY),
                        "agg": agg_ref.agg_call(dec, atts, keys, cols), "group": group_ref.group_call(dec, atts, keys, self.BY, cols),
                        "project": project_ref.project_call(dec, atts, keys, self.PCOLS)}
            assert want["filter"][3][1] > 0 and want["group"][3] > 0 and {0, 1, 2} <= set(want["agg"][0]["status"].tolist()), (mixed, B)
            for method in (METHOD_LZ4, METHOD_ZSTD):
                comps = dec_by_method[method][0]
                for host in (False, True):
                    chunk = 1 if opts.get(cc.OPT_WORKSPACE_MAX_BYTES) else len(comps)
                    buf = ("d_vfy",) + (HOST_IN if host else (("d_keytab",) if mixed else ()))
                    buf += ("d_ws",) if method == METHOD_ZSTD else lz4_ws(B, chunk)
                    tag = "%s method %d B%d %s" % ("host" if host else "device", method, B, "mixed keys" if mixed else "integer keys")
                    a = (method, comps, B, atts, keys)
                    calls = {
                        "filter": ((tcall.filter_host if host else tcall.filter_batch), a + (0, W), scan_calls.same_filter),
                        "count": ((tcall.filter_host if host else tcall.filter_batch), a + (fl.COUNT_ONLY, W), scan_calls.same_filter),
                        "agg": ((tcall.agg_host if host else tcall.agg_batch), a + (cols, W), scan_calls.same_agg),
                        "group": ((tcall.group_host if host else tcall.group_batch), a + (self.BY, cols, W), scan_calls.same_group),
                        "project": ((tcall.project_host if host else tcall.project_batch), a + (self.PCOLS, W), scan_calls.same_project)}
                    for kind, (fn, args, same) in calls.items():
                        entry = "cryo_codec_%s_%s" % ("filter" if kind == "count" else kind, "blocks" if host else "batch")

                        def check(got, state, what, same=same, w=want[kind]):
                            same(got, w, what)
                        yield Route(group, kind + " " + tag, lambda c, fn=fn, args=args: fn(c, *args), check, entry, buf, opts)

    def _scan_int(self):
        yield from self._scan_routes("scan_int", False, {})

    def _scan_keys(self):
        """a float key, a byte-string key and a set key of eleven members under a truth table; float columns through the
        aggregate and the grouped scan"""
        yield from self._scan_routes("scan_keys", True, {})

    def _scan_chunked(self):
        yield from self._scan_routes("scan_chunked", True, {cc.OPT_WORKSPACE_MAX_BYTES: 1}, sizes=(4096,))
        yield from self._scan_routes("scan_chunked", False, {cc.OPT_WORKSPACE_MAX_BYTES: 1}, sizes=(32768,))

    # -- the keyed pool --
    def _pool(self):
        """cryo_codec_decompress_blocks_keyed: every run reads six blocks the run before left in the pool (hits: the pool is not
        filled) and four under keys of its own (misses, decoded through the filled staging buffers), one of them rejected.  The pool
        has 256 slots: a run takes four, so the ring does not come round to the six within a session's runs"""
        B = 32768
        for method in (METHOD_LZ4, METHOD_ZSTD):
            raws = synth_mix(self.oracle, B, 10, 71)
            kept = [encode(self.oracle, method, r) for r in raws[:6]]
            fresh = [encode(self.oracle, method, r) for r in raws[6:]]
            fresh[1] = fresh[1][:len(fresh[1]) - 4].copy()
            want = raws[:6] + [decode(self.oracle, method, f, B) for f in fresh]
            assert want[7] is None

            turn = {"n": 0}
            hi = (9 + method) << 32

            def run(c, method=method, kept=kept, fresh=fresh, turn=turn, hi=hi):
                turn["n"] += 1
                c.set_option(cc.OPT_POOL_BYTES, POOL_SLOTS * B)
                if c.transfer_counters()["pool_capacity"] != POOL_SLOTS or not turn.get("primed"):
                    c.decompress_blocks_keyed(method, [hi | i for i in range(6)], kept, B)
                    turn["primed"] = True
                keys = [hi | i for i in range(6)] + [hi | (100 * turn["n"] + i) for i in range(4)]
                t0 = c.transfer_counters()
                outs, st = c.decompress_blocks_keyed(method, keys, kept + fresh, B)
                t1 = c.transfer_counters()
                return outs, st, t1["pool_hits"] - t0["pool_hits"], t1["pool_misses"] - t0["pool_misses"]

            def check(got, state, what, want=want):
                outs, st, hits, misses = got
                assert (hits, misses) == (6, 4), (what, hits, misses)
                for i, w in enumerate(want):
                    assert st[i] == (cc.OK if w is not None else cc.E_CORRUPT), (what, i, int(st[i]))
                    assert w is None or np.array_equal(outs[i], w), (what, i)
            yield Route("pool", "keyed method %d" % method, run, check, "cryo_codec_decompress_blocks_keyed",
                        HOST_IO + (("d_ws",) if method == METHOD_ZSTD else lz4_ws(B, 4)))


def one_route_per_kind(table):
    """the routes that follow a failed call: in every group one route of every entry point the group calls (and one of the
    group's routes that name none): the one with the most blocks -- of the batched decodes never a lone-block route -- and of
    equals the last, which is the larger block size and the second method"""
    chosen = {}
    for r in table.all():
        n = re.search(r"\bn(\d+)\b", r.name)
        size = int(n.group(1)) if n else 0
        for e in r.entry or {""}:
            key = (r.group, e)
            if key not in chosen or size >= chosen[key][0]:
                chosen[key] = (size, r)
    return [r for _, r in chosen.values()]


# ---- calls that fail ----
def failing_calls(codec, oracle):
    """a batch in which every stream is rejected (device and host form, both methods), a call refused with CRYO_E_ARG and one
    refused with CRYO_E_UNSUPPORTED; each is checked for what it must answer"""
    B = 32768
    for method in (METHOD_LZ4, METHOD_ZSTD):
        comps = [encode(oracle, method, r)[:-7].copy() for r in synth_mix(oracle, B, 5, 81)]
        assert all(decode(oracle, method, c, B) is None for c in comps)
        st, rows = decompress_batch(codec, method, comps, B)
        assert (st == cc.E_CORRUPT).all() and (rows[:, B:] == SENTINEL).all(), (method, st)
        st, rows = decompress_host(codec, method, comps, B, each=True)
        assert (st == cc.E_CORRUPT).all() and (rows == SENTINEL).all(), (method, st)
        assert (codec.check_blocks(method, comps, B)[:, 0] == layout_ref.STREAM).all()
        recs, dst, total = codec.fetch_blocks(method, comps, B, [[1]] * 5, dst=np.full(5 * B, SENTINEL, np.uint8))
        assert (recs["status"] == cc.FETCH_STREAM).all() and total == 0 and (dst == SENTINEL).all()
        assert (check_batch(codec, method, comps, B)[:, 0] == layout_ref.STREAM).all()
        same_fetch(fetch_batch(codec, method, comps, B, [[1, 2]] * 5), fetch_ref.fetch_call([None] * 5, [[1, 2]] * 5), "all rejected")
        atts, keys, cols = fc.ATTS, Table.INT_KEYS, Table.INT_COLS
        for calls in (tcall, ):
            scan_calls.same_filter(calls.filter_batch(codec, method, comps, B, atts, keys), filter_ref.filter_call([None] * 5, atts, keys))
            scan_calls.same_filter(calls.filter_host(codec, method, comps, B, atts, keys), filter_ref.filter_call([None] * 5, atts, keys))
            scan_calls.same_agg(calls.agg_host(codec, method, comps, B, atts, keys, cols), agg_ref.agg_call([None] * 5, atts, keys, cols))
            scan_calls.same_group(calls.group_batch(codec, method, comps, B, atts, keys, Table.BY, cols),
                                  group_ref.group_call([None] * 5, atts, keys, Table.BY, cols))
            scan_calls.same_project(calls.project_host(codec, method, comps, B, atts, keys, Table.PCOLS),
                                    project_ref.project_call([None] * 5, atts, keys, Table.PCOLS))
        st, sz, _ = recode_batch(codec, method, comps, B, METHOD_LZ4, 1)
        assert (st == cc.E_CORRUPT).all() and (sz == 0).all()
    raw = oracle.synth(82, 0, B, 0)
    for level, code in ((23, cc.E_UNSUPPORTED),):
        try:
            compress_batch(codec, METHOD_ZSTD, level, [raw])
            raise AssertionError("zstd level %d was taken" % level)
        except CryoError as e:
            assert e.code == code, e
    with Dev(codec) as d:
        src, off, sz = d.streams([encode(oracle, METHOD_LZ4, raw)])
        dst, st = d.alloc(B), d.alloc(16)
        for bad in (lambda: codec.decompress_batch(7, src, off, sz, dst, B, B, 1, st),               # no such method
                    lambda: codec.decompress_batch(METHOD_LZ4, src, off, sz, dst, B - 1, B, 1, st),   # a stride below the block
                    lambda: codec.check_batch(METHOD_LZ4, src, off, sz, B + 4, 1, dst)):              # not a multiple of 8
            try:
                bad()
                raise AssertionError("a call that must be refused was taken")
            except CryoError as e:
                assert e.code == cc.E_ARG, e
    codec.sync()
