"""CPU tests of the grouped scan's surface: what include/cryo_codec.h declares, what the libraries export, the layouts of the
structures on both sides of the ABI, and the argument errors that need no device."""
import ctypes as C
import os
import re

import numpy as np

import agg_cases as ac
import group_cases as gc
import group_ref as gr
from pg_cryogen_amd import codec, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cryo_codec_group_batch", "cryo_codec_group_blocks", "cryo_multi_group_blocks")


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
        assert hasattr(lib, "cryo_group_scan") and hasattr(lib, "cryo_host_group_ops"), path
    for hook in ("cryo_host_set_group_ops", "cryo_group_set_window"):    # the hooks are the test build's only
        assert hasattr(C.CDLL(host.HOST_TEST_LIB_PATH), hook) and not hasattr(C.CDLL(host.HOST_LIB_PATH), hook), hook


def test_struct_sizes_and_values():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"typedef struct \{ uint32_t nby, rsv; const cryo_agg_col \*by; \} cryo_group;", txt)
    assert re.search(r"typedef struct \{ uint32_t status, n_items, n_match, n_bad; uint32_t n_groups, rsv; uint64_t first_group; \} "
                     r"cryo_group_block;", txt)
    assert re.search(r"typedef struct \{ int64_t key\[2\]; uint32_t n_rows, nulls; \} cryo_group_rec;", txt)
    assert re.search(r"#define CRYO_GROUP_MAX_BY 2u", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert (C.sizeof(codec.CryoGroup), codec.GROUP_BLOCK.itemsize, codec.GROUP_REC.itemsize) == (16, 32, 24)
    assert (gr.ROW, gr.REC, gr.CELL) == (codec.GROUP_BLOCK, codec.GROUP_REC, codec.AGG_CELL) and codec.GROUP_MAX_BY == gr.MAX_BY == 2
    assert [codec.GROUP_BLOCK.fields[f][1] for f in ("n_groups", "first_group")] == [16, 24]
    assert [codec.GROUP_REC.fields[f][1] for f in ("key", "n_rows", "nulls")] == [0, 16, 20]
    assert C.sizeof(host.CryoGroupRec) == 24 and C.sizeof(host.CryoGroupBlock) == 40 and C.sizeof(host.CryoCodecGroupOps) == 8
    assert C.sizeof(host.CryoGroupTotals) == 9 * 8
    # the other tables keep their layouts: the grouping is bound through a table of its own
    assert C.sizeof(host.CryoCodecAggOps) == 8 and C.sizeof(host.CryoCodecFilterOps) == 8 and C.sizeof(host.CryoAggTotals) == 8 * 8 + 4 * 40
    # the section that states the rules comes after the aggregate's
    assert txt.index("aggregating a scan") < txt.index("grouping a scan") < txt.index("int cryo_codec_group_batch")


def test_descriptor_helpers():
    g, a = codec.group_desc([(4, codec.KEY_INT4), (2, codec.KEY_INT8)])
    assert g.nby == 2 and g.rsv == 0 and g.by == a.ctypes.data
    assert [(int(c["att"]), int(c["type"])) for c in a] == [(4, codec.KEY_INT4), (2, codec.KEY_INT8)]
    assert not a["rsv"].any() and not a["rsv2"].any()


def test_argument_errors_need_no_device():
    """a null handle and every bad descriptor: CRYO_E_ARG from the host-buffer calls before a device is touched"""
    L = codec.lib()
    rows, recs, cells = np.zeros(1, codec.GROUP_BLOCK), np.zeros(290, codec.GROUP_REC), np.zeros(4 * 290, codec.AGG_CELL)
    total = C.c_uint64()
    f, r, g = codec.filter_desc(ac.ATTS, []), codec.group_desc([(4, codec.KEY_INT4)]), codec.agg_desc([(2, codec.KEY_INT8)])
    assert L.cryo_codec_group_batch(None, 0, None, None, None, 4096, 0, C.byref(f[0]), C.byref(r[0]), C.byref(g[0]), None, None, 0,
                                    None, None) == codec.E_ARG
    out = (rows.ctypes.data, recs.ctypes.data, 290, cells.ctypes.data, C.byref(total))
    for fn in (L.cryo_codec_group_blocks, L.cryo_multi_group_blocks):
        assert fn(None, 0, None, None, 0, 4096, C.byref(f[0]), C.byref(r[0]), C.byref(g[0]), *out) == codec.E_ARG
        assert fn(None, 0, None, None, 0, 4096, None, C.byref(r[0]), C.byref(g[0]), *out) == codec.E_ARG
        assert fn(None, 0, None, None, 0, 4096, C.byref(f[0]), None, C.byref(g[0]), *out) == codec.E_ARG
        assert fn(None, 0, None, None, 0, 4096, C.byref(f[0]), C.byref(r[0]), C.byref(g[0]), *out[:4], None) == codec.E_ARG


def test_every_descriptor_rule_is_refused_without_a_device():
    """every entry of group_cases.descriptors(): the reference's verdict is the table's, and the host-buffer calls, given the
    descriptor without a handle, return CRYO_E_ARG without touching a device or reading past an array (on a device the same
    table separates CRYO_OK from CRYO_E_ARG: tests/test_gpu_group.py)"""
    L = codec.lib()
    rows, recs, cells = np.zeros(1, codec.GROUP_BLOCK), np.zeros(290, codec.GROUP_REC), np.zeros(4 * 290, codec.AGG_CELL)
    total = C.c_uint64()
    for name, atts, keys, by, cols, flags, patch, ok in gc.descriptors():
        assert gc.ref_ok(gr, atts, keys, by, cols, flags, patch) == ok, name
        f, a, k = codec.filter_desc(atts, keys, flags)
        r, b = codec.group_desc(by)
        g, c = codec.agg_desc(cols or [])
        if patch:
            which, field, index, value = patch
            if which in "frg":
                {"f": f, "r": r, "g": g}[which].rsv = value
            else:
                {"a": a, "k": k, "b": b, "c": c}[which][field][index] = value
        for fn in (L.cryo_codec_group_blocks, L.cryo_multi_group_blocks):
            assert fn(None, 0, None, None, 0, ac.B, C.byref(f), C.byref(r), None if cols is None else C.byref(g), rows.ctypes.data,
                      recs.ctypes.data, 290, cells.ctypes.data, C.byref(total)) == codec.E_ARG, name


def test_group_source_is_in_the_build():
    csrc = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
    txt = open(os.path.join(csrc, "group.hip")).read()
    for kernel in ("k_group_block", "k_group_offsets", "k_group_copy"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, txt), kernel
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "asm" not in code and "atomic" not in code.replace("__ATOMIC_", "")        # plain C++ only, no global atomics
    assert re.search(r"^SRCS\s*:=.*\bgroup\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    assert "launch_group" in open(os.path.join(csrc, "kernels.h")).read()
    # the walk exists once and is called once, from the sweep header; the grouped scan's turn (six capture slots) is in group_lds.h
    walk = open(os.path.join(csrc, "filter_walk.h")).read()
    assert len(re.findall(r"\bwalk_tuple\s*\(const uint8_t", walk)) == 1
    sweep = open(os.path.join(csrc, "scan_sweep.h")).read()
    assert '#include "filter_walk.h"' in sweep and len(re.findall(r"\bwalk_tuple<", sweep)) == 1
    lds = open(os.path.join(csrc, "group_lds.h")).read()
    assert '#include "scan_sweep.h"' in lds and "sweep_turn<true, kGroupSlots, BYTES" in lds and "walk_tuple<" not in lds
    # the kernel is group_lds.h's body, which takes the three steps in turn
    assert '#include "group_lds.h"' in txt and "group_block<BYTES" in txt and "walk_tuple<" not in txt and "t[22]" not in txt
    assert all(len(re.findall(r"\b%s<" % step, lds)) == 1 for step in ("group_matches", "group_reduce")) and "group_rank(L" in lds
    hmk = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bgroup\.c\b", hmk, flags=re.M)
