"""CPU tests of the ordered scan's surface: the layouts of the header's structures as a C compiler lays them out against the numpy
dtypes and the ctypes structures, what the header declares and the libraries export, and the argument errors that need no device:
every bad descriptor is refused by the host-buffer calls with CRYO_E_ARG before a handle is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import topn_cases as tcs
import topn_ref as tr
from pg_cryogen_amd import codec, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cryo_codec.h")
NAMES = ("cryo_codec_topn_batch", "cryo_codec_topn_blocks", "cryo_multi_topn_blocks")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cryo_codec.h"
#define O(t, f) offsetof(t, f)
int main(void)
{
    printf("%zu %zu %zu %zu %zu\n", sizeof(cryo_order_col), O(cryo_order_col, att), O(cryo_order_col, type), O(cryo_order_col, flags),
           O(cryo_order_col, rsv));
    printf("%zu %zu %zu %zu\n", sizeof(cryo_order), O(cryo_order, nby), O(cryo_order, limit), O(cryo_order, by));
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(cryo_topn_block), O(cryo_topn_block, status), O(cryo_topn_block, n_items),
           O(cryo_topn_block, n_match), O(cryo_topn_block, n_bad), O(cryo_topn_block, n_rows), O(cryo_topn_block, rsv),
           O(cryo_topn_block, row_first));
    printf("%zu %zu %zu %zu %zu\n", sizeof(cryo_topn_rec), O(cryo_topn_rec, key), O(cryo_topn_rec, pos), O(cryo_topn_rec, key_nulls),
           O(cryo_topn_rec, nulls));
    printf("%u %u %u\n", CRYO_ORDER_DESC, CRYO_ORDER_NULLS_FIRST, CRYO_ORDER_MAX_BY);
    return 0;
}
"""


def test_layouts_as_a_c_compiler_sees_them(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    lines = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0] == [8, 0, 2, 3, 4]
    assert lines[1] == [16, 0, 4, 8]
    assert lines[2] == [32, 0, 4, 8, 12, 16, 20, 24]
    assert lines[3] == [24, 0, 16, 18, 20]
    assert lines[4] == [1, 2, 2] == [codec.ORDER_DESC, codec.ORDER_NULLS_FIRST, codec.ORDER_MAX_BY] == [tr.DESC, tr.NULLS_FIRST, tr.MAX_BY]
    # the Python side: numpy dtypes, the ctypes struct, the reference's dtypes
    for dtype, names, line in ((codec.ORDER_COL, ("att", "type", "flags", "rsv"), lines[0]),
                               (codec.TOPN_BLOCK, ("status", "n_items", "n_match", "n_bad", "n_rows", "rsv", "row_first"), lines[2]),
                               (codec.TOPN_REC, ("key", "pos", "key_nulls", "nulls"), lines[3])):
        assert dtype.itemsize == line[0] and [dtype.fields[f][1] for f in names] == line[1:] and dtype.names == names
    assert (tr.ORDER_COL, tr.BLOCK, tr.REC) == (codec.ORDER_COL, codec.TOPN_BLOCK, codec.TOPN_REC)
    assert C.sizeof(codec.CryoOrder) == 16 and [getattr(codec.CryoOrder, f).offset for f in ("nby", "limit", "by")] == lines[1][1:]
    assert C.sizeof(host.CryoCodecTopnOps) == 8 and C.sizeof(host.CryoTopnMerge) == 48 and C.sizeof(host.CryoTopnTotals) == 72
    assert C.sizeof(host.CryoTopnBlock) == 48


def test_header_declares_and_libraries_export():
    from pg_cryogen_amd import _loader
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = codec.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in codec.ABI_SYMBOLS and hasattr(L, n), n
    # the section that states the rules comes after the projection's, and says what is out of scope
    assert raw.index("projecting a scan") < raw.index("ordering a scan") < raw.index("int cryo_codec_topn_batch")
    section = raw[raw.index("ordering a scan"):raw.index("int cryo_codec_topn_batch")]
    for word in ("WITH TIES", "DISTINCT ON", "OFFSET", "bucketed", "more than two order columns"):
        assert word in section, word
    _loader.load()
    for path in (host.HOST_LIB_PATH, host.HOST_TEST_LIB_PATH):
        lib = C.CDLL(path)
        for n in ("cryo_topn_scan", "cryo_host_topn_ops", "cryo_topn_merge_init", "cryo_topn_merge_add", "cryo_topn_merge_finish",
                  "cryo_topn_merge_free"):
            assert hasattr(lib, n), (path, n)
    for hook in ("cryo_host_set_topn_ops", "cryo_topn_set_window"):       # the hooks are the test build's only
        assert hasattr(C.CDLL(host.HOST_TEST_LIB_PATH), hook) and not hasattr(C.CDLL(host.HOST_LIB_PATH), hook)


def test_descriptor_helpers():
    o, a = codec.order_desc([(2, codec.KEY_INT8, codec.ORDER_DESC), (3, codec.KEY_INT2, 3)], 100)
    assert (o.nby, o.limit, o.by) == (2, 100, a.ctypes.data)
    assert [tuple(int(x) for x in c) for c in a] == [(2, codec.KEY_INT8, 1, 0), (3, codec.KEY_INT2, 3, 0)]
    rec = np.zeros(1, codec.TOPN_REC)[0]
    rec["key"][0], rec["key_nulls"] = -(1 << 63), 2
    by = [(1, 3, codec.ORDER_DESC), (2, 3, codec.ORDER_NULLS_FIRST)]
    assert codec.topn_sort_key(by, rec) == ((1, (1 << 63) - 1), (0, 0))   # DESC of INT64_MIN is its complement; NULLS FIRST is class 0


def test_argument_errors_need_no_device():
    """a null handle and every bad descriptor: CRYO_E_ARG from the three calls before a device is touched"""
    L = codec.lib()
    table, rec, rows = np.zeros(1, codec.TOPN_BLOCK), np.zeros(290, codec.TOPN_REC), np.zeros((290, 64), np.uint8)
    total = C.c_uint64(7)

    def call(fn, f, o, p, tot=total):
        return fn(None, 0, None, None, 0, 4096, f, o, p, rows.ctypes.data, rec.ctypes.data, 290, table.ctypes.data, C.byref(tot) if tot else None)

    for name, atts, keys, by, limit, cols, patch, ok in tcs.descriptors():
        (f, a, k), (o, oa), (p, pa) = codec.filter_desc(atts, keys), codec.order_desc(by, limit), codec.project_desc(cols)
        if patch:
            which, index, value = patch
            if which == "p":
                p.rsv = value
            else:
                {"b": oa, "c": pa}[which]["rsv" if which == "b" else "rsv2"][index] = value
        for fn in (L.cryo_codec_topn_blocks, L.cryo_multi_topn_blocks):
            # a good descriptor gets as far as the null handle, a bad one not even there: CRYO_E_ARG either way, and the good
            # ones are told apart on the GPU (tests/test_gpu_topn.py)
            assert call(fn, C.byref(f), C.byref(o), C.byref(p)) == codec.E_ARG, name
    (f, a, k), (o, oa), (p, pa) = codec.filter_desc(tcs.ATTS, []), codec.order_desc([(tcs.K, codec.KEY_INT8, 0)], 5), codec.project_desc(tcs.COLS)
    for fn in (L.cryo_codec_topn_blocks, L.cryo_multi_topn_blocks):
        assert call(fn, None, C.byref(o), C.byref(p)) == codec.E_ARG
        assert call(fn, C.byref(f), None, C.byref(p)) == codec.E_ARG
        assert call(fn, C.byref(f), C.byref(o), None) == codec.E_ARG
        assert call(fn, C.byref(f), C.byref(o), C.byref(p), None) == codec.E_ARG
    assert L.cryo_codec_topn_batch(None, 0, None, None, None, 4096, 0, C.byref(f), C.byref(o), C.byref(p), None, None, 0, None,
                                   C.byref(total)) == codec.E_ARG
    assert total.value == 7                                               # nothing was written for a refused call


def test_topn_source_is_in_the_build():
    csrc = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
    txt = open(os.path.join(csrc, "topn.hip")).read()
    for kernel in ("k_topn_block", "k_topnf_block", "k_topn_offsets", "k_topn_copy"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % kernel, txt), kernel
    assert '#include "scan_sweep.h"' in open(os.path.join(csrc, "group_lds.h")).read() and '#include "group_lds.h"' in txt
    assert "sweep_turn<" in txt and "walk_tuple<" not in txt and "atomic" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"^SRCS\s*:=.*\btopn\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    assert "launch_topn" in open(os.path.join(csrc, "kernels.h")).read()
    hmk = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btopn\.c\b", hmk, flags=re.M)
