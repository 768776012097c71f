"""CPU tests of the bucketed grouping's surface: the layout of cryo_bucket and cryo_group_b as a C compiler lays out the header's
text, against the Python side's structures; cryo_group still has its 16 bytes and the entry points their prototypes; and the
descriptor helpers build today's descriptor when no buckets are given."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bucket_ref as bk
from pg_cryogen_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cryo_codec.h")

PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "cryo_codec.h"
int main(void)
{
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(cryo_bucket), offsetof(cryo_bucket, kind), offsetof(cryo_bucket, flags),
           offsetof(cryo_bucket, rsv), offsetof(cryo_bucket, n), offsetof(cryo_bucket, origin), offsetof(cryo_bucket, value));
    printf("%zu %zu %zu %zu %zu\n", sizeof(cryo_group_b), offsetof(cryo_group_b, nby), offsetof(cryo_group_b, rsv),
           offsetof(cryo_group_b, by), offsetof(cryo_group_b, buckets));
    printf("%zu %zu %zu %zu\n", sizeof(cryo_group), offsetof(cryo_group, nby), offsetof(cryo_group, rsv), offsetof(cryo_group, by));
    printf("%u %d %d %d %u %u %u\n", CRYO_GROUP_BUCKETS, CRYO_BUCKET_NONE, CRYO_BUCKET_WIDTH, CRYO_BUCKET_BOUNDS,
           CRYO_BUCKET_INFINITE, CRYO_BUCKET_BOUNDS_MAX, CRYO_KEY_SET_MAX);
    return 0;
}
"""


def test_layouts_as_a_c_compiler_sees_them(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    lines = [[int(x) for x in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert lines[0] == [24, 0, 1, 2, 4, 8, 16]
    assert lines[1] == [24, 0, 4, 8, 16]
    assert lines[2] == [16, 0, 4, 8]                                      # cryo_group is what it was: a cryo_group_b starts with one
    assert lines[3] == [1, 0, 1, 2, 1, 1024, 1024]
    # the Python side
    assert codec.BUCKET.itemsize == 24 and [codec.BUCKET.fields[f][1] for f in ("kind", "flags", "rsv", "n", "origin", "value")] == lines[0][1:]
    assert C.sizeof(codec.CryoGroup) == 16 and C.sizeof(codec.CryoGroupB) == 24
    assert [getattr(codec.CryoGroupB, f).offset for f in ("nby", "rsv", "by", "buckets")] == lines[1][1:]
    assert (codec.GROUP_BUCKETS, codec.BUCKET_NONE, codec.BUCKET_WIDTH, codec.BUCKET_BOUNDS, codec.BUCKET_INFINITE, codec.BUCKET_BOUNDS_MAX) == \
        tuple(lines[3][:6]) == (1, bk.NONE, bk.WIDTH, bk.BOUNDS, bk.INFINITE, bk.BOUNDS_MAX)


def test_header_text():
    txt = open(HEADER).read()
    assert re.search(r"typedef struct \{ uint32_t nby, rsv; const cryo_agg_col \*by; \} cryo_group;", txt)
    assert re.search(r"typedef struct \{ uint8_t kind, flags; uint16_t rsv; uint32_t n; int64_t origin; int64_t value; \} cryo_bucket;", txt)
    assert re.search(r"typedef struct \{ uint32_t nby, rsv; const cryo_agg_col \*by; const cryo_bucket \*buckets; \} cryo_group_b;", txt)
    # the entry points take a cryo_group as before
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("cryo_codec_group_batch", "cryo_codec_group_blocks", "cryo_multi_group_blocks"):
        proto = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, code).group(1)
        assert "const cryo_group *grp" in proto and not re.search(r"\bcryo_group_b\b", proto), name
    assert txt.index("grouping a scan") < txt.index("Bucketed group columns") < txt.index("int cryo_codec_group_batch")


def test_descriptor_helpers():
    by = [(4, codec.KEY_INT4), (2, codec.KEY_INT8)]
    g, a = codec.group_desc(by)
    assert type(g) is codec.CryoGroup and g.rsv == 0                      # without buckets: today's descriptor
    members = [7, -3, 7, (1 << 63) - 1, -(1 << 63)]
    g, a2 = codec.group_desc(by, [bk.width(-5, 86400, bk.INFINITE), bk.bounds(members)])
    assert type(g) is codec.CryoGroupB and (g.nby, g.rsv, g.by) == (2, codec.GROUP_BUCKETS, a2.ctypes.data) and a2.tobytes() == a.tobytes()
    b = g.bucket_arr
    assert g.buckets == b.ctypes.data and b.ctypes.data % 8 == 0
    assert tuple(b[0]) == (bk.WIDTH, bk.INFINITE, 0, 0, -5, 86400)
    assert tuple(b[1])[:5] == (bk.BOUNDS, 0, 0, 5, 0)
    at = int(b[1]["value"])
    assert at % 8 != 0                                                    # the helper hands the list over at no alignment
    assert list(np.frombuffer(C.string_at(at, 40), "<i8")) == members     # as given: the library sorts its own copy
    # the device form: the same array, rebased to where the caller put the lists
    arr, lists, rebase = codec.bucket_array([bk.RAW, bk.bounds([1, 2])])
    assert tuple(arr[0]) == (0, 0, 0, 0, 0, 0) and int(rebase(0x1000)[1]["value"]) == 0x1001 and lists.nbytes == 17
