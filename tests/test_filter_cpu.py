"""CPU tests of the scan filter: the rules (tests/filter_ref.py) against an independent statement on the generator's blocks and
on hand-made vectors (tests/filter_cases.py), the ABI surface, and cryo_filter_scan (host/filter.c) walking a mini-AM relation
through the test build, with a codec double whose filter_blocks decodes with the oracle and answers by the rules."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fetch_walk
import filter_cases as fc
import filter_ref as fr
import tuple_craft as tc
from mini_am import load_relation
from pg_cryogen_amd import codec, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B128 = 131072
E_UNSUPPORTED, E_ARG = -6, -1
SYNTH_ATTS = [(4, 4), (-1, 4)]
NAMES = ("cryo_codec_filter_batch", "cryo_codec_filter_blocks", "cryo_multi_filter_blocks")
KERNELS = ("k_filter_match", "k_filter_offsets", "k_filter_copy")


def positions(recs, status=fr.OK):
    return [r[0] for r in recs if r[1] == status]


# ---- the reference against an independent statement ----
@pytest.mark.parametrize("B", [131072, 1 << 20])
def test_reference_on_generator_blocks(oracle, B):
    """rowid = block x 290 + pos is the int4 column of `wide`, `narrow` and `int4` (include/cryo_synth.h): a range on column 1
    matches exactly the positions whose rowid lies in it; column 2 is a text in `wide` and `narrow` and missing in `int4`"""
    for d, block in ((0, 3), (1, 0), (2, 7)):
        raw = oracle.synth(21, block, B, d)
        for lo, hi in ((block * 290 + 40, block * 290 + 44), (block * 290 - 5, block * 290 + 3), (block * 290 + 289, block * 290 + 1000),
                       (0, 1 << 30), (5, 5)):
            st, n, recs = fr.filter_block(raw, SYNTH_ATTS, [(1, fr.INT4, fr.GE, lo), (1, fr.INT4, fr.LT, hi)])
            assert (st, n) == (fr.OK, 290) and positions(recs) == [p for p in range(1, 291) if lo <= block * 290 + p < hi]
            assert all(r[2] == struct.unpack_from("<II", raw, 8 + 8 * (r[0] - 1))[1] for r in recs)
        st, n, recs = fr.filter_block(raw, SYNTH_ATTS, [(2, 0, fr.NOTNULL, 0)])
        assert positions(recs) == ([] if d == 2 else list(range(1, 291)))
        st, n, recs = fr.filter_block(raw, SYNTH_ATTS, [(2, 0, fr.ISNULL, 0)])
        assert positions(recs) == (list(range(1, 291)) if d == 2 else [])
    assert fr.filter_block(oracle.synth(21, 1, B, 4), SYNTH_ATTS, [])[:2] == (fr.OK, 0)            # zeros: no item
    # random tuple bytes: whatever the verdicts, the reference reads nothing outside a tuple (Tuple asserts that)
    for block in range(3):
        st, n, recs = fr.filter_block(oracle.synth(21, block, B, 3), SYNTH_ATTS, [(2, 0, fr.NOTNULL, 0), (1, fr.INT4, fr.GE, 0)])
        assert st == fr.OK and n == 290 and {r[1] for r in recs} <= {fr.OK, fr.ITEM, fr.TUPLE}
    # a call: placement, packed bytes with zero pads, totals
    blocks = [oracle.synth(21, b, B, 1) for b in range(3)] + [None]
    table, recs, packed, (tb, tr) = fr.filter_call(blocks, SYNTH_ATTS, [(1, fr.INT4, fr.GE, 289), (1, fr.INT4, fr.LT, 293)])
    assert table["n_match"].tolist() == [2, 2, 0, 0] and table["status"].tolist() == [0, 0, 0, fr.STREAM]
    assert table["rec_first"].tolist() == [0, 2, 4, 4] and table["off"].tolist() == [0, 128, 256, 256] and (tb, tr) == (256, 4)
    assert recs["pos"].tolist() == [289, 290, 1, 2] and (recs["len"] == 61).all()
    assert [struct.unpack_from("<i", packed, 64 * i + 24)[0] for i in range(4)] == [289, 290, 291, 292]
    assert not packed.reshape(4, 64)[:, 61:].any()
    assert fr.tuples_of(table, recs, packed, 1)[0][0] == 1


def test_reference_on_hand_made_vectors():
    for name, blk, keys, matches, bad in fc.cases():
        assert fr.desc_ok(fc.ATTS, keys), name
        st, n, recs = fr.filter_block(blk, fc.ATTS, keys)
        assert st == fr.OK and positions(recs) == matches, (name, positions(recs), matches)
        assert {r[0]: r[1] for r in recs if r[1] != fr.OK} == bad, name
        assert [r[0] for r in recs] == sorted(r[0] for r in recs), name                            # position order
        ct = fr.filter_call([blk], fc.ATTS, keys, fr.COUNT_ONLY)
        assert tuple(ct[0][0]) == (0, n, len(matches), len(bad), 0, 0) and ct[1].size == 0 and ct[3] == (0, 0), name
    # each damaged tuple alone, under a key that walks every column
    for name, t in fc.tuple_cases():
        assert fr.filter_tuple(t, fc.ATTS, fc.WALK) == fr.TUPLE, name
    blk = tc.build_block(fc.B, fc.ops_block())
    for keys, att, op, value in fc.ops_keys():
        assert fr.desc_ok(fc.ATTS, keys), keys
        assert positions(fr.filter_block(blk, fc.ATTS, keys)[2]) == fc.ops_expected(att, op, value), keys
    # OVERLAP: the block delivers no tuple and no match record, the bad item keeps its record; COUNT_ONLY places nothing
    over = fc.overlap_block()
    assert fr.filter_block(over, fc.ATTS, fc.K6) == (fr.OVERLAP, 5, [(5, fr.ITEM, 0, 0)])
    good = tc.build_block(fc.B, [fc.T(*fc.GOOD)] * 3)
    table, recs, packed, total = fr.filter_call([good, over, good], fc.ATTS, fc.K6)
    assert table["status"].tolist() == [0, fr.OVERLAP, 0] and table["n_match"].tolist() == [3, 0, 3]
    assert table["rec_first"].tolist() == [0, 3, 4] and table["off"].tolist() == [0, 3 * 64, 3 * 64] and total == (6 * 64, 7)
    assert recs["status"].tolist() == [0, 0, 0, fr.ITEM, 0, 0, 0]
    table = fr.filter_call([good, over, good], fc.ATTS, fc.K6, fr.COUNT_ONLY)[0]
    assert table["status"].tolist() == [0, 0, 0] and table["n_match"].tolist() == [3, 4, 3] and table["n_bad"].tolist() == [0, 1, 0]
    # HEADER; several handles
    h = good.copy()
    h[0:4] = np.frombuffer(struct.pack("<I", 12), np.uint8)
    assert fr.filter_block(h, fc.ATTS, fc.K6) == (fr.HEADER, 0, [])
    table, regions, total = fr.multi_call([good, good, over, good, good], fc.ATTS, fc.K6, 2, fc.B)
    assert [(b0, r0) for b0, _, r0, _ in regions] == [(0, 0), (3 * fc.B, 3 * 290)]
    assert table["off"].tolist() == [0, 3 * fc.B, 192, 3 * fc.B + 192, 192] and table["rec_first"].tolist() == [0, 870, 3, 873, 4]
    assert total == (3 * fc.B + 6 * 64, 870 + 6)


def test_descriptor_rules():
    for name, atts, keys, flags, patch, ok in fc.descriptors():
        rsv = dict(rsv=1) if patch and patch[0] == "f" else {}
        if patch and patch[0] == "a":
            rsv = dict(att_rsv=[0] * patch[2] + [1])
        if patch and patch[0] == "k":
            rsv = dict(key_rsv=[1])
        assert fr.desc_ok(atts, keys, flags, **rsv) == ok, name


# ---- the surface ----
def test_header_declares_and_libraries_export():
    from pg_cryogen_amd import _loader
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cryo_codec.h")).read(), flags=re.S)
    L = codec.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in codec.ABI_SYMBOLS and hasattr(L, n), n
    _loader.load()
    for path in (host.HOST_LIB_PATH, host.HOST_TEST_LIB_PATH):
        lib = C.CDLL(path)
        assert hasattr(lib, "cryo_filter_scan") and hasattr(lib, "cryo_host_filter_ops"), path
    assert hasattr(C.CDLL(host.HOST_TEST_LIB_PATH), "cryo_host_set_filter_ops")
    assert not hasattr(C.CDLL(host.HOST_LIB_PATH), "cryo_host_set_filter_ops")      # the hooks are the test build's only
    assert not hasattr(C.CDLL(host.HOST_LIB_PATH), "cryo_filter_set_window")


def test_struct_sizes_and_values():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"typedef struct \{ int16_t attlen; uint8_t attalign; uint8_t rsv; \} cryo_att;", txt)
    assert re.search(r"typedef struct \{ uint16_t att; uint8_t type, op; uint32_t rsv; int64_t value; \} cryo_scan_key;", txt)
    assert re.search(r"typedef struct \{ uint32_t status, n_items, n_match, n_bad; uint64_t rec_first, off; \} cryo_filter_block;", txt)
    assert re.search(r"typedef struct \{ uint16_t pos, status; uint32_t len; \} cryo_filter_rec;", txt)
    assert (codec.FILTER_ATT.itemsize, codec.FILTER_KEY.itemsize, codec.FILTER_BLOCK.itemsize, codec.FILTER_REC.itemsize) == (4, 16, 32, 8)
    assert (fr.BLOCK, fr.REC) == (codec.FILTER_BLOCK, codec.FILTER_REC)
    assert C.sizeof(codec.CryoFilter) == 32 and C.sizeof(host.CryoCodecFilterOps) == 8
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define CRYO_FILTER_COUNT_ONLY 1u", body) and re.search(r"#define CRYO_FILTER_TUPLE 8u", body)
    assert re.search(r"CRYO_KEY_INT2 = 1, CRYO_KEY_INT4 = 2, CRYO_KEY_INT8 = 3", body)
    assert re.search(r"CRYO_OP_LT = 1, CRYO_OP_LE, CRYO_OP_EQ, CRYO_OP_GE, CRYO_OP_GT, CRYO_OP_NE, CRYO_OP_ISNULL, CRYO_OP_NOTNULL", body)
    assert (codec.KEY_INT2, codec.KEY_INT4, codec.KEY_INT8) == (fr.INT2, fr.INT4, fr.INT8) == (1, 2, 3)
    assert (codec.OP_LT, codec.OP_NOTNULL, codec.FILTER_TUPLE, codec.FILTER_COUNT_ONLY) == (fr.LT, fr.NOTNULL, fr.TUPLE, fr.COUNT_ONLY)
    assert (fr.STREAM, fr.HEADER, fr.ITEM, fr.OVERLAP) == (codec.FETCH_STREAM, codec.FETCH_HEADER, codec.FETCH_ITEM, codec.FETCH_OVERLAP)
    # CryoCodecOps keeps its layout: the filter is bound through a table of its own
    assert C.sizeof(host.CryoCodecOpsRecode) == C.sizeof(host.CryoCodecOps) + 16


def test_argument_errors_need_no_device():
    L = codec.lib()
    tot = (C.c_uint64 * 2)(7, 7)
    f = codec.filter_desc(SYNTH_ATTS, [])
    table = np.zeros(1, codec.FILTER_BLOCK)
    assert L.cryo_codec_filter_batch(None, 0, None, None, None, 4096, 0, C.byref(f[0]), None, 0, None, 0, None, tot) == codec.E_ARG
    assert L.cryo_codec_filter_blocks(None, 0, None, None, 0, 4096, C.byref(f[0]), None, 0, None, 0, table.ctypes.data, tot) == codec.E_ARG
    assert L.cryo_multi_filter_blocks(None, 0, None, None, 0, 4096, C.byref(f[0]), None, 0, None, 0, table.ctypes.data, tot) == codec.E_ARG
    assert L.cryo_codec_filter_blocks(None, 0, None, None, 0, 4096, None, None, 0, None, 0, table.ctypes.data, tot) == codec.E_ARG


def test_filter_source_is_in_the_build():
    txt = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "filter.hip")).read()
    for k in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, txt), k
    assert "asm" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)                     # plain C++ only
    mk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfilter\.hip\b", mk, flags=re.M)
    assert "launch_filter" in open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "kernels.h")).read()
    hmk = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfilter\.c\b", hmk, flags=re.M)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_filter_kernels_compile_for_gfx950(tmp_path):
    """device assembly of filter.hip: the three kernels are there, for gfx950, without scratch; LDS only in the scan"""
    out = tmp_path / "filter.s"
    csrc = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", os.path.join(csrc, "filter.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=csrc)
    assert r.returncode == 0, r.stderr
    asm = out.read_text()
    assert "gfx950" in asm
    for k in KERNELS:
        body = re.search(r"\.amdhsa_kernel \S*%s\S*\n(.*?)\.end_amdhsa_kernel" % k, asm, flags=re.S)
        assert body, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body.group(1)), k
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body.group(1)).group(1))
        assert lds == (64 if k == "k_filter_offsets" else 0), (k, lds)
    assert "global_store_dwordx4" in asm and "global_store_dwordx2" in asm      # table rows and side entries; records and bytes


# ---- the walk, through a codec double ----
class FilteringDouble:
    """the oracle double of tests/codec_double.py plus a filter table that decodes with the oracle and answers from filter_ref"""

    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self._filter = host.FILTER_BLOCKS_FN(self.filter_blocks)
        self.filter_ops = host.CryoCodecFilterOps(self._filter)

    def filter_blocks(self, ctx, method, srcs, sizes, n, bs, filt, dst, dst_cap, rec, rec_cap, rows, total):
        f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
        atts = np.ctypeslib.as_array(C.cast(f.atts, C.POINTER(C.c_uint8)), (4 * f.natts,)).view(codec.FILTER_ATT)
        keys = np.ctypeslib.as_array(C.cast(f.keys, C.POINTER(C.c_uint8)), (16 * f.nkeys,)).view(codec.FILTER_KEY) if f.nkeys else []
        atts = [(int(a["attlen"]), int(a["attalign"])) for a in atts]
        keys = [(int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"])) for k in keys]
        if not fr.desc_ok(atts, keys, f.flags, f.rsv):
            return E_ARG
        blocks = []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(fr.decode(self.base.ora, method, comp, bs))
        self.calls.append((method, n))
        table, recs, packed, (tb, tr) = fr.filter_call(blocks, atts, keys, f.flags)
        if tb > dst_cap or tr > rec_cap:
            return -5
        if tb:
            C.memmove(dst, packed.ctypes.data, tb)
        if tr:
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
        C.memmove(rows, table.ctypes.data, table.nbytes)
        total[0], total[1] = tb, tr
        return 0


@pytest.fixture()
def HF():
    L = host.lib()
    dbl = FilteringDouble()
    L.cryo_host_set_codec_ops(C.byref(dbl.base.ops))
    L.cryo_host_set_filter_ops(C.byref(dbl.filter_ops))
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B128)
    L.cryo_init_cache()
    yield L, dbl, errors
    L.cryo_filter_set_window(0, 0)
    L.cryo_cache_shutdown()
    L.cryo_host_set_filter_ops(None)
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


INT4 = [(4, 4)]


def _table(L):
    rows = [struct.pack("<i", i) for i in range(1, 2501)]                # 9 blocks of int4 rows, the last one partly filled
    return load_relation(L, rows, 1, host.COMP_LZ4, xid=777)


def _rows(events):
    return [struct.unpack_from("<i", e[4], 24)[0] for e in events if e[0] == "tuple"]


def test_filter_scan_walk_through_a_double(HF, oracle):
    L, dbl, errors = HF
    mem, rel, blocks, firsts = _table(L)
    raw = lambda i: np.frombuffer(blocks[i], np.uint8)                    # noqa: E731
    # a zstd block among the LZ4 ones; a block with a damaged item and a damaged tuple; then an unreadable chain and an unknown
    # method in the middle of the relation, and good chains behind them
    z_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 902, oracle.zstd_compress(raw(1), 1))
    bad = raw(2).copy()
    bad[12 + 8 * 4:16 + 8 * 4] = 0                                        # item 5: len 0
    off7 = struct.unpack_from("<I", bad, 8 + 8 * 6)[0]
    bad[off7 + 22] = 16                                                   # tuple 7: hoff 16
    item_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 901, oracle.lz4_compress(bad, 1))
    short_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 904, oracle.lz4_compress(raw(0), 1))
    odd_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 905, oracle.lz4_compress(raw(0), 1))
    dead_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_LZ4, 906, oracle.lz4_compress(raw(3), 1))
    tail_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 907, oracle.zstd_compress(raw(0), 1))
    page = L.cryo_memrel_page(mem, short_first)
    csize = struct.unpack_from("<I", C.string_at(page, 64), 40)[0]
    C.memmove(page + 40, struct.pack("<I", csize + 100000), 4)
    C.memmove(L.cryo_memrel_page(mem, odd_first) + 36, struct.pack("<i", 9), 4)
    C.memset(L.cryo_memrel_page(mem, dead_first) + 48, 0xFF, 64)

    keys = [(1, fr.INT4, fr.GE, 280), (1, fr.INT4, fr.LT, 600)]
    events, t = host.filter_scan(rel, INT4, keys)
    # rows 280 .. 599 from the table (blocks 0 .. 2), rows 291 .. 580 again from the zstd copy of block 1, rows 581 .. 599 but
    # for the two damaged ones from the damaged copy of block 2, rows 280 .. 290 from the zstd copy of block 0
    want = list(range(280, 600)) + list(range(291, 581)) + [r for r in range(581, 600) if r not in (585, 587)] + list(range(280, 291))
    assert _rows(events) == want
    reports = [e for e in events if e[0] == "report"]
    assert reports == [("report", item_first, fr.ITEM, 5), ("report", item_first, fr.TUPLE, 7),
                       ("report", short_first, fetch_walk.CHAIN, host.CRYO_ERR_DECOMPRESSION_FAILED),
                       ("report", odd_first, fetch_walk.METHOD, 9), ("report", dead_first, fr.STREAM, 0)]
    # order of delivery: block order, then position order; the reports between the tuples
    order = [(e[1], e[2] if e[0] == "tuple" else -1) for e in events]
    assert [b for b, _ in order] == sorted(b for b, _ in order)
    at = events.index(("report", item_first, fr.ITEM, 5))
    assert events[at - 1][:3] == ("tuple", item_first, 4) and events[at + 1][:3] == ("tuple", item_first, 6)
    assert all(e[3] == {z_first: 902, item_first: 901, tail_first: 907}.get(e[1], 777) for e in events if e[0] == "tuple")
    assert all(e[5] == 28 and len(e[4]) == 32 for e in events if e[0] == "tuple")
    assert dbl.calls == [(host.COMP_LZ4, 11), (host.COMP_ZSTD, 2)]        # both methods in one relation: one call each
    n_items = 2500 + 290 + 290 + 290                                      # the dead block shows no item
    assert (t["blocks"], t["items"], t["matches"], t["bad"], t["reports"], t["codec_calls"]) == (15, n_items, len(want), 2, 5, 2)
    assert t["bytes_back"] == 32 * 13 + 8 * (len(want) + 2) + 32 * len(want)
    # COUNT_ONLY: no tuple, the same counts; bad items are counted, not reported
    dbl.calls.clear()
    events, c = host.filter_scan(rel, INT4, keys, fr.COUNT_ONLY)
    assert [e for e in events if e[0] == "tuple"] == [] and len(events) == 3
    assert (c["items"], c["matches"], c["bad"], c["reports"]) == (n_items, len(want), 2, 3) and c["bytes_back"] == 32 * 13
    # no key: every well-formed tuple
    events, t = host.filter_scan(rel, INT4)
    assert t["matches"] == n_items - 2 == len(_rows(events))
    # a frozen block is handed over with FrozenTransactionId, as the read path does
    L.cryo_memrel_set_frozen(mem, firsts[3], True)
    events, _ = host.filter_scan(rel, INT4, [(1, fr.INT4, fr.EQ, 900)])
    assert [(e[1], e[2], e[3]) for e in events if e[0] == "tuple"] == [(firsts[3], 30, 2)]
    # a descriptor the codec refuses
    with pytest.raises(host.FilterScanError) as e:
        host.filter_scan(rel, INT4, [(2, fr.INT4, fr.EQ, 1)])
    assert e.value.code == E_ARG and not [x for x in e.value.events if x[0] == "tuple"]
    assert L.cryo_filter_scan(C.byref(rel), None, host.FETCH_TUPLE_FN(0), host.FETCH_REPORT_FN(0), None, None) == E_ARG
    assert not errors
    L.cryo_memrel_destroy(mem)


def test_filter_scan_windows(HF, oracle):
    """the window lowered to 4 chains, then to the compressed bytes of about three: several codec calls, the same delivery"""
    L, dbl, _ = HF
    mem, rel, blocks, firsts = _table(L)
    z_first, _ = fetch_walk.write_chain(L, mem, rel, host.COMP_ZSTD, 902, oracle.zstd_compress(np.frombuffer(blocks[1], np.uint8), 1))
    keys = [(1, fr.INT4, fr.GE, 100), (1, fr.INT4, fr.LT, 2400)]
    whole, t0 = host.filter_scan(rel, INT4, keys)
    assert dbl.calls == [(host.COMP_LZ4, 9), (host.COMP_ZSTD, 1)] and t0["codec_calls"] == 2
    dbl.calls.clear()
    L.cryo_filter_set_window(4, 0)
    got, t = host.filter_scan(rel, INT4, keys)
    assert got == whole and _rows(got) == list(range(100, 2400)) + list(range(291, 581))
    assert dbl.calls == [(host.COMP_LZ4, 4), (host.COMP_LZ4, 4), (host.COMP_LZ4, 1), (host.COMP_ZSTD, 1)] and t["codec_calls"] == 4
    assert {k: v for k, v in t.items() if k != "codec_calls"} == {k: v for k, v in t0.items() if k != "codec_calls"}
    dbl.calls.clear()
    csize = len(oracle.lz4_compress(np.frombuffer(blocks[0], np.uint8), 1))
    L.cryo_filter_set_window(0, 3 * csize + csize // 2)
    got, t = host.filter_scan(rel, INT4, keys)
    assert got == whole and t["codec_calls"] == len(dbl.calls) >= 3 and max(n for _, n in dbl.calls) <= 4
    L.cryo_memrel_destroy(mem)


def test_without_a_filter_table_the_scan_is_unsupported(HF):
    L, dbl, _ = HF
    mem, rel, blocks, firsts = _table(L)
    L.cryo_host_set_filter_ops(None)
    with pytest.raises(host.FilterScanError) as e:
        host.filter_scan(rel, INT4, [])
    assert e.value.code == E_UNSUPPORTED and e.value.events == [] and e.value.totals["blocks"] == 0
    L.cryo_memrel_destroy(mem)
