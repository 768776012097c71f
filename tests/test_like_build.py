"""Build check of every block kernel of the scan calls with the pattern keys (CRYO_OP_LIKE, CRYO_OP_NOT_LIKE) in the walk, CPU
only: the nine scan sources are cross-compiled for gfx950 with the compiler's resource-usage remarks.  The matcher (walk_like,
filter_walk.h) inlined into the existing instantiations cost waves -- k_filter_match<true>, k_filterf_match and the two
projection kernels fell from eight waves per SIMD to seven, k_agg_block<true> from seven to five -- so descriptors with a pattern
key run kernels of their own names, each alone in a unit of its own: its source compiled a second time with CRYO_LIKE_UNIT.
Every source must hold exactly the kernels it held at the parent commit, each without scratch, without a spill and with not a
wave per SIMD fewer than there; every second unit exactly its one kernel, without scratch and without a spill.  Resource
figures only: no instruction is looked at.

Figures found for the new kernels (waves per SIMD, LDS bytes, VGPRs, SGPRs):
    k_filterl_match   7, 0, 66, 96        k_projectl_block  7, 0, 70, 102       k_topnl_block    6, 13920, 76, 105
    k_aggl_block      5, 0, 92, 98        k_groupl_block    3, 32480, 74, 93    k_groupbl_block  3, 32480, 74, 99
    k_grouptl_block   1, 34800, 84, 98"""
import os
import re
import subprocess

import pytest

from test_bytes_key_build import CSRC, ROOT

# {source: {kernel name as mangled: waves per SIMD}} at the parent commit, acd8add (hipcc -O3, -Rpass-analysis=kernel-resource-usage)
PARENT = {
    "filter.hip": {"k_filter_matchILb0E": 8, "k_filter_matchILb1E": 8, "k_filterf_match": 8, "k_filter_offsets": 8, "k_filter_copy": 8},
    "project.hip": {"k_project_blockILb0E": 7, "k_project_blockILb1E": 8, "k_projectf_block": 8, "k_project_offsets": 8, "k_project_copy": 8},
    "agg.hip": {"k_agg_blockILb0E": 8, "k_agg_blockILb1E": 7},
    "agg_float.hip": {"k_aggf_block": 7},
    "group.hip": {"k_group_blockILb0E": 3, "k_group_blockILb1E": 3, "k_group_offsets": 8, "k_group_copy": 8},
    "group_float.hip": {"k_groupf_block": 3},
    "group_bucket.hip": {"k_groupb_blockILb0E": 3, "k_groupb_blockILb1E": 3},
    "group_text.hip": {"k_groupt_blockILb0E": 1, "k_groupt_blockILb1E": 1},
    "topn.hip": {"k_topn_blockILb0E": 6, "k_topn_blockILb1E": 6, "k_topnf_block": 6, "k_topn_offsets": 8, "k_topn_copy": 8},
}
# the kernels of descriptors with a pattern key: one per call and kind of grouping, float keys and float columns included
NEW = {"filter.hip": "k_filterl_match", "project.hip": "k_projectl_block", "agg_float.hip": "k_aggl_block", "group_float.hip": "k_groupl_block",
       "group_bucket.hip": "k_groupbl_block", "group_text.hip": "k_grouptl_block", "topn.hip": "k_topnl_block"}
SOURCES = sorted(PARENT)


def resource_usage(source, tmp_path, like_unit=False):
    """test_bytes_key_build.resource_usage, for the source's second unit too: {mangled kernel name: {figure: value}}"""
    out_name = source + (".like.o" if like_unit else ".o")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage"] + (["-DCRYO_LIKE_UNIT"] if like_unit else []) +
                       ["-c", os.path.join(CSRC, source), "-o", str(tmp_path / out_name)], capture_output=True, text=True, timeout=600, cwd=CSRC)
    assert r.returncode == 0, r.stderr
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s+([A-Za-z][A-Za-z ]*?)(?: \[[^\]]*\])?: (\d+))", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2)] = int(m.group(3))
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("like_build")


def test_the_tables_name_every_kernel():
    assert len(SOURCES) == 9 and sum(len(v) for v in PARENT.values()) == 27 and len(NEW) == 7
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^%_like\.o: %\.hip .*\n\t.*-DCRYO_LIKE_UNIT", mk, flags=re.M)
    assert sorted(re.search(r"^LIKE_SRCS\s*:=(.*)$", mk, flags=re.M).group(1).split()) == sorted(NEW)


def check(figures, kernel, waves=None):
    print(kernel, figures)
    assert figures["ScratchSize"] == 0, (kernel, figures)
    assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (kernel, figures)
    if waves is not None:
        assert figures["Occupancy"] >= waves, (kernel, figures)


@pytest.mark.parametrize("source", SOURCES)
def test_every_source_holds_what_it_held_and_loses_no_wave(tmp, source):
    found = resource_usage(source, tmp)
    assert len(found) == len(PARENT[source]), (sorted(found), sorted(PARENT[source]))     # not an instantiation more
    for kernel, waves in PARENT[source].items():
        mine = {k: v for k, v in found.items() if kernel in k}
        assert len(mine) == 1, (kernel, sorted(found))
        check(next(iter(mine.values())), kernel, waves)


@pytest.mark.parametrize("source", sorted(NEW))
def test_the_second_unit_holds_the_pattern_kernel_alone(tmp, source):
    found = resource_usage(source, tmp, like_unit=True)
    assert len(found) == 1 and NEW[source] in next(iter(found)), sorted(found)
    check(next(iter(found.values())), NEW[source])
