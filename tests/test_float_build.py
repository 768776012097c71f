"""Build check of the float kernels (k_filterf_match, k_projectf_block, k_aggf_block, k_groupf_block), CPU only: filter.hip,
project.hip, agg.hip, agg_float.hip, group.hip and group_float.hip are cross-compiled for gfx950 with the compiler's resource-usage
remarks.  The four old kernels keep exactly two instantiations each -- float descriptors run kernels of their own, under names
that do not contain the old ones --, and each new kernel needs no scratch and no spill and keeps the waves per SIMD the contract
derives for it.  Resource figures only: no instruction is looked at.

Figures found (hipcc -O3, -Rpass-analysis=kernel-resource-usage; waves per SIMD, LDS bytes, VGPRs, SGPRs):
    k_filter_match<true>   8, 0, 46, 84        k_filterf_match   8, 0, 46, 89
    k_project_block<true>  8, 0, 49, 89        k_projectf_block  8, 0, 49, 94
    k_agg_block<true>      7, 0, 71, 77        k_aggf_block      7, 0, 72, 91
    k_group_block<true>    3, 32480, 56, 82    k_groupf_block    3, 32480, 74, 87
(the SGPR figures since the kernels share the sweep of scan_sweep.h; 82 / 87, 76 / 88 and 80 / 85 before; the group kernels' VGPR
figures since they share group_lds.h's group_reduce; 62 and 88 before)
k_groupf_block is bound by LDS (two waves' share of 64 KiB is 32 480 bytes: 3 workgroups of 2 waves on 4 SIMDs), not by its
registers."""
import pytest

from test_bytes_key_build import resource_usage

OLD = {"filter.hip": "k_filter_match", "agg.hip": "k_agg_block", "group.hip": "k_group_block", "project.hip": "k_project_block"}
NEW = {"filter.hip": "k_filterf_match", "agg_float.hip": "k_aggf_block", "group_float.hip": "k_groupf_block", "project.hip": "k_projectf_block"}
GROUP_LDS, GROUP_WAVES = 32480, 3


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("float_build")
    return {source: resource_usage(source, tmp) for source in sorted(set(OLD) | set(NEW))}


def one(usage, source, kernel):
    mine = {k: v for k, v in usage[source].items() if kernel in k}
    assert len(mine) == 1, (kernel, sorted(usage[source]))
    return next(iter(mine.values()))


def sibling(usage, source, kernel):
    """the <true> instantiation of an old kernel"""
    mine = {k: v for k, v in usage[source].items() if kernel in k and "ILb1E" in k}
    assert len(mine) == 1, (kernel, sorted(usage[source]))
    return next(iter(mine.values()))


@pytest.mark.parametrize("source", sorted(OLD))
def test_old_kernels_keep_two_instantiations(usage, source):
    mine = [k for k in usage[source] if OLD[source] in k]
    assert len(mine) == 2 and {("ILb1E" in k) for k in mine} == {False, True}, sorted(usage[source])
    for other in usage:                                                    # and no float source instantiates one
        if other != source:
            assert not [k for k in usage[other] if OLD[source] in k], (other, sorted(usage[other]))


@pytest.mark.parametrize("source", sorted(NEW))
def test_float_kernels_need_no_scratch_and_no_spill(usage, source):
    figures = one(usage, source, NEW[source])
    print(NEW[source], figures)
    assert figures["ScratchSize"] == 0, figures
    assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, figures


def test_filter_and_projection_keep_their_siblings_waves(usage):
    for source in ("filter.hip", "project.hip"):
        new, old = one(usage, source, NEW[source]), sibling(usage, source, OLD[source])
        assert new["Occupancy"] == old["Occupancy"] and new["LDS Size"] == old["LDS Size"], (source, new, old)


def test_group_keeps_its_lds_and_waves(usage):
    new, old = one(usage, "group_float.hip", "k_groupf_block"), sibling(usage, "group.hip", "k_group_block")
    assert new["LDS Size"] == old["LDS Size"] == GROUP_LDS, (new, old)
    assert new["Occupancy"] == old["Occupancy"] == GROUP_WAVES, (new, old)


def test_aggregate_loses_at_most_one_wave(usage):
    new, old = one(usage, "agg_float.hip", "k_aggf_block"), sibling(usage, "agg.hip", "k_agg_block")
    assert new["LDS Size"] == 0 and new["Occupancy"] >= old["Occupancy"] - 1, (new, old)
