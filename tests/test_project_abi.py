"""CPU tests of the projecting scan's surface: what include/cryo_codec.h declares, what the libraries export, the layouts of the
structures on both sides of the ABI, and the argument errors that need no device."""
import ctypes as C
import os
import re

import numpy as np

import project_cases as pc
import project_ref as pr
from pg_cryogen_amd import codec, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cryo_codec_project_batch", "cryo_codec_project_blocks", "cryo_multi_project_blocks")


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
        assert hasattr(lib, "cryo_project_scan") and hasattr(lib, "cryo_host_project_ops"), path
    for hook in ("cryo_host_set_project_ops", "cryo_project_set_window"):    # the hooks are the test build's only
        assert hasattr(C.CDLL(host.HOST_TEST_LIB_PATH), hook) and not hasattr(C.CDLL(host.HOST_LIB_PATH), hook), hook


def test_struct_sizes_and_values():
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"typedef struct \{ uint16_t att; uint16_t rsv; uint32_t rsv2; \} cryo_project_col;", txt)
    assert re.search(r"typedef struct \{ uint32_t ncols, rsv; const cryo_project_col \*cols; \} cryo_project;", txt)
    assert re.search(r"typedef struct \{ uint32_t status, n_items, n_match, n_bad; uint64_t rec_first, row_first; \} cryo_project_block;",
                     txt)
    assert re.search(r"typedef struct \{ uint16_t pos, status; uint32_t nulls; \} cryo_project_rec;", txt)
    assert re.search(r"#define CRYO_PROJECT_MAX_COLS 8u", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    assert (codec.PROJECT_COL.itemsize, C.sizeof(codec.CryoProject), codec.PROJECT_BLOCK.itemsize, codec.PROJECT_REC.itemsize) == \
        (8, 16, 32, 8)
    assert (pr.COL, pr.BLOCK, pr.REC) == (codec.PROJECT_COL, codec.PROJECT_BLOCK, codec.PROJECT_REC)
    assert codec.PROJECT_MAX_COLS == pr.MAX_COLS == 8
    assert [codec.PROJECT_BLOCK.fields[f][1] for f in ("rec_first", "row_first")] == [16, 24]
    assert [codec.PROJECT_REC.fields[f][1] for f in ("pos", "status", "nulls")] == [0, 2, 4]
    assert C.sizeof(host.CryoCodecProjectOps) == 8 and C.sizeof(host.CryoProjectedRow) == 32 and C.sizeof(host.CryoProjectTotals) == 8 * 8
    # the other tables keep their layouts: the projection is bound through a table of its own
    assert C.sizeof(host.CryoCodecGroupOps) == 8 and C.sizeof(host.CryoCodecAggOps) == 8 and C.sizeof(host.CryoCodecFilterOps) == 8
    assert C.sizeof(host.CryoCodecFetchOps) == 8 and C.sizeof(host.CryoCodecOpsRecode) == 10 * 8
    # the section that states the rules comes after the grouping's
    assert txt.index("aggregating a scan") < txt.index("grouping a scan") < txt.index("int cryo_codec_group_batch") < \
        txt.index("projecting a scan") < txt.index("int cryo_codec_project_batch") < txt.index("single block, HOST buffers")


def test_descriptor_helpers():
    p, a = codec.project_desc([4, 2, 4])
    assert p.ncols == 3 and p.rsv == 0 and p.cols == a.ctypes.data
    assert [int(c["att"]) for c in a] == [4, 2, 4] and not a["rsv"].any() and not a["rsv2"].any()
    assert codec.project_row_layout(pc.ATTS, pc.MIX) == ([0, 8, 16, 18, 20, 24], 32)


def _outputs():
    rows, rec, table = np.zeros((290, 64), np.uint8), np.zeros(290, codec.PROJECT_REC), np.zeros(1, codec.PROJECT_BLOCK)
    total = (C.c_uint64 * 2)()
    return (rows, rec, table, total), (rows.ctypes.data, 290, rec.ctypes.data, 290, table.ctypes.data, total)


def test_argument_errors_need_no_device():
    """a null handle, a null filter, a null projection, null totals: CRYO_E_ARG from every call before a device is touched"""
    L = codec.lib()
    keep, out = _outputs()
    f, p = codec.filter_desc(pc.ATTS, []), codec.project_desc([1])
    assert L.cryo_codec_project_batch(None, 0, None, None, None, 4096, 0, C.byref(f[0]), C.byref(p[0]), None, 0, None, 0, None,
                                      None) == codec.E_ARG
    for fn in (L.cryo_codec_project_blocks, L.cryo_multi_project_blocks):
        assert fn(None, 0, None, None, 0, 4096, C.byref(f[0]), C.byref(p[0]), *out) == codec.E_ARG
        assert fn(None, 0, None, None, 0, 4096, None, C.byref(p[0]), *out) == codec.E_ARG
        assert fn(None, 0, None, None, 0, 4096, C.byref(f[0]), None, *out) == codec.E_ARG
        assert fn(None, 0, None, None, 0, 4096, C.byref(f[0]), C.byref(p[0]), *out[:5], None) == codec.E_ARG


def test_every_descriptor_rule_is_refused_without_a_device():
    """every entry of project_cases.descriptors(): the reference's verdict is the table's, and the host-buffer calls, given the
    descriptor without a handle, return CRYO_E_ARG without touching a device or reading past an array (on a device the same
    table separates CRYO_OK from CRYO_E_ARG: tests/test_gpu_project.py)"""
    L = codec.lib()
    keep, out = _outputs()
    names = [d[0] for d in pc.descriptors()]
    for must in ("no column", "nine columns", "att 0", "att beyond natts", "a varlena column", "attlen 3", "attlen 16",
                 "attalign below attlen", "reserved field of the projection", "reserved half of a column", "reserved word of a column",
                 "count only"):
        assert must in names, must
    for name, atts, keys, cols, flags, patch, ok in pc.descriptors():
        assert pc.ref_ok(pr, atts, keys, cols, flags, patch) == ok, name
        f, a, k = codec.filter_desc(atts, keys, flags)
        p, c = codec.project_desc(cols)
        if patch:
            which, field, index, value = patch
            if which in "fp":
                {"f": f, "p": p}[which].rsv = value
            else:
                {"a": a, "k": k, "c": c}[which][field][index] = value
        for fn in (L.cryo_codec_project_blocks, L.cryo_multi_project_blocks):
            assert fn(None, 0, None, None, 0, pc.B, C.byref(f), C.byref(p), *out) == codec.E_ARG, name


def test_project_source_is_in_the_build():
    csrc = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
    txt = open(os.path.join(csrc, "project.hip")).read()
    for kernel in ("k_project_block", "k_project_offsets", "k_project_copy"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, txt), kernel
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert "asm" not in code and "atomic" not in code                        # plain C++ only, no global atomics
    assert re.search(r"^SRCS\s*:=.*\bproject\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    assert "launch_project" in open(os.path.join(csrc, "kernels.h")).read()
    # the walk exists once and is called once, from the sweep header that the four kernels' sources take their turn from
    walk = open(os.path.join(csrc, "filter_walk.h")).read()
    assert len(re.findall(r"\bwalk_tuple\s*\(const uint8_t", walk)) == 1
    sweep = open(os.path.join(csrc, "scan_sweep.h")).read()
    assert '#include "filter_walk.h"' in sweep and len(re.findall(r"\bwalk_tuple<", sweep)) == 1
    assert '#include "scan_sweep.h"' in txt and "sweep_turn<true, kProjectMaxCols, BYTES" in txt and "walk_tuple<" not in txt
    assert "t[22]" not in txt
    assert "offsets_tile" in txt
    hmk = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bproject\.c\b", hmk, flags=re.M)
