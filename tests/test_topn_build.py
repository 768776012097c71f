"""Build check of the ordered scan's kernels, CPU only: topn.hip is cross-compiled for gfx950 with the compiler's resource-usage
remarks.  It holds exactly the three block kernels of its own name (k_topn_block with and without byte-string keys, k_topnf_block)
beside its offsets and copy kernels and none of the other scans' kernels; the three need no scratch and spill nothing, stay within
k_group_block's 32 480 bytes of LDS per workgroup and reach at least its 3 waves per SIMD; and project.hip, group.hip, agg.hip and
filter.hip instantiate no kernel of this call.  Resource figures only: no instruction is looked at.

Figures at the commit that added the call (VGPRs, SGPRs, scratch, occupancy):
    k_topn_block<false>  48, 99, 0, 6      k_topn_block<true>  56, 97, 0, 6      k_topnf_block  55, 99, 0, 6      LDS 13 920"""
import pytest

from test_bytes_key_build import resource_usage

OLD = ("k_filter", "k_agg", "k_group", "k_project")
LDS_MAX, WAVES_MIN = 32480, 3


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("topn_build")
    return {src: resource_usage(src, tmp) for src in ("topn.hip", "project.hip", "group.hip", "agg.hip", "filter.hip")}


def test_exactly_the_three_block_kernels(usage):
    mine = usage["topn.hip"]
    blocks = sorted(k for k in mine if "k_topn_block" in k or "k_topnf_block" in k)
    assert len(blocks) == 3 and sum("k_topn_blockILb0E" in k for k in blocks) == 1 and sum("k_topn_blockILb1E" in k for k in blocks) == 1 \
        and sum("k_topnf_block" in k for k in blocks) == 1, sorted(mine)
    others = sorted(k for k in mine if k not in blocks)
    assert len(others) == 2 and any("k_topn_offsets" in k for k in others) and any("k_topn_copy" in k for k in others), others
    assert not [k for k in mine if any(o in k for o in OLD)], sorted(mine)


def test_no_scratch_no_spill_lds_and_occupancy(usage):
    for name, figures in usage["topn.hip"].items():
        print(name, figures)
        assert figures["ScratchSize"] == 0, (name, figures)
        assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (name, figures)
        assert figures["LDS Size"] <= LDS_MAX, (name, figures)
        assert figures["Occupancy"] >= WAVES_MIN, (name, figures)


@pytest.mark.parametrize("source", ["project.hip", "group.hip", "agg.hip", "filter.hip"])
def test_the_other_scans_instantiate_no_topn_kernel(usage, source):
    assert usage[source] and not [k for k in usage[source] if "topn" in k], sorted(usage[source])
