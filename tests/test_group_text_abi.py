"""CPU tests of the text grouping's surface: the layout of cryo_group_key as a C compiler lays out the header's text, against the
Python side's mirrors; cryo_group still has its 16 bytes and the entry points their prototypes; the header states the rules; and
codec.group_desc builds today's descriptor unless text is asked for."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import group_text_ref as gt
from pg_cryogen_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cryo_codec.h")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cryo_codec.h"
int main(void)
{
    printf("%zu %zu %zu %zu\n", sizeof(cryo_group_key), offsetof(cryo_group_key, bytes), offsetof(cryo_group_key, len),
           offsetof(cryo_group_key, rsv));
    printf("%zu %zu %zu %zu\n", sizeof(cryo_group), offsetof(cryo_group, nby), offsetof(cryo_group, rsv), offsetof(cryo_group, by));
    printf("%u %u %u %d %zu %zu\n", CRYO_GROUP_TEXT, CRYO_GROUP_TEXT_MAX, CRYO_GROUP_BUCKETS, (int)CRYO_KEY_BYTES, sizeof(cryo_agg_cell),
           sizeof(((cryo_group_key *)0)->bytes));
    return 0;
}
"""


def test_layouts_as_a_c_compiler_sees_them(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    lines = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0] == [40, 0, 32, 36]
    assert lines[1] == [16, 0, 4, 8]                                      # cryo_group is what it was
    assert lines[2] == [4, 32, 1, 16, 40, 32]                             # a key cell has an aggregate cell's room
    # the Python side: the library's dtype, the reference's, and the ctypes struct the flag rides in
    for dt in (codec.GROUP_KEY, gt.KEY):
        assert dt.itemsize == 40 and [dt.fields[f][1] for f in ("bytes", "len", "rsv")] == lines[0][1:]
        assert dt.fields["bytes"][0].shape == (32,)
    assert codec.AGG_CELL.itemsize == codec.GROUP_KEY.itemsize
    assert C.sizeof(codec.CryoGroup) == 16 and [getattr(codec.CryoGroup, f).offset for f in ("nby", "rsv", "by")] == lines[1][1:]
    assert (codec.GROUP_TEXT, codec.GROUP_TEXT_MAX, codec.GROUP_BUCKETS, codec.KEY_BYTES) == tuple(lines[2][:4]) == \
        (gt.TEXT, gt.TEXT_MAX, gt.BUCKETS, gt.BYTES)


def test_header_text():
    txt = open(HEADER).read()
    assert re.search(r"#define CRYO_GROUP_TEXT 4u\b", txt) and re.search(r"#define CRYO_GROUP_TEXT_MAX 32u\b", txt)
    assert re.search(r"typedef struct \{ uint8_t bytes\[32\]; uint32_t len, rsv; \} cryo_group_key;", txt)
    assert re.search(r"typedef struct \{ uint32_t nby, rsv; const cryo_agg_col \*by; \} cryo_group;", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("cryo_codec_group_batch", "cryo_codec_group_blocks", "cryo_multi_group_blocks"):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, code).group(1)
        assert "const cryo_group *grp" in proto and "cryo_agg_cell *" in proto and "cryo_group_key" not in proto, name
    assert txt.index("Bucketed group columns") < txt.index("Text group columns") < txt.index("int cryo_codec_group_batch")
    rules = re.sub(r"\s*\n \*\s*", " ", txt[txt.index("/* Text group columns"):txt.index("#define CRYO_GROUP_TEXT 4u")])
    for phrase in ("attlen == -1", "'' is a value, not NULL", "counted in n_bad and not in n_match", "NULLS LAST",
                   "memcmp on unsigned bytes over the shorter length, then by length", "any deterministic collation", 'under "C" only',
                   "ncols + ntext cells of 40 bytes", "only when ncols + ntext == 0", "24 + 40 * (ncols + ntext) bytes per possible group",
                   "exactly the bytes of the rsv == 0 call", "stays refused as an aggregate column", "both flags together (5)"):
        assert phrase in rules, phrase


def test_descriptor_helpers():
    by = [(2, codec.KEY_BYTES), (5, codec.KEY_INT4)]
    g, a = codec.group_desc(by)
    assert type(g) is codec.CryoGroup and g.rsv == 0                      # without text: today's descriptor
    g, a2 = codec.group_desc(by, text=True)
    assert type(g) is codec.CryoGroup and (g.nby, g.rsv, g.by) == (2, codec.GROUP_TEXT, a2.ctypes.data) and a2.tobytes() == a.tobytes()
    assert [tuple(c) for c in a2] == [(2, 16, 0, 0), (5, codec.KEY_INT4, 0, 0)]
    assert codec.group_text_count((g, a2)) == 1 and codec.group_text_count(codec.group_desc([(5, codec.KEY_INT4)], text=True)) == 0
    g, _ = codec.group_desc(by, [(0, 0, 0, 0)] * 2, text=True)
    assert type(g) is codec.CryoGroupB and g.rsv == 5                     # the library refuses it; the helper says what was asked
    # a call's cells apart: two aggregate cells and a key cell per group
    raw = np.zeros((3, 120), np.uint8)
    raw[1, 80:83] = list(b"abc")
    raw[1, 112] = 3
    raw[2, 0] = 7
    agg, key = codec.group_cells_split(raw, 2, 1)
    assert agg.shape == (3, 2) and key.shape == (3, 1) and agg.dtype == codec.AGG_CELL and key.dtype == codec.GROUP_KEY
    assert int(agg["n"][2, 0]) == 7 and bytes(key["bytes"][1, 0][:3]) == b"abc" and key["len"][:, 0].tolist() == [0, 3, 0]
    agg, key = codec.group_cells_split(np.zeros((2, 40), np.uint8), 0, 1)
    assert agg.shape == (2, 0) and key.shape == (2, 1)
