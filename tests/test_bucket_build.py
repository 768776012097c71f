"""Build check of the bucketed grouping's kernels (k_groupb_block<false>, k_groupb_block<true>), CPU only: group.hip and
group_bucket.hip are cross-compiled for gfx950 with the compiler's resource-usage remarks.  The two new kernels need no scratch
and no spill and keep k_group_block's LDS and waves per SIMD -- LDS bounds all of them (two waves' share of 64 KiB is 32 480 bytes:
3 workgroups of 2 waves on 4 SIMDs) --, and group_bucket.hip instantiates neither of the old names.  Resource figures only: no
instruction is looked at.

Figures found (hipcc -O3, -Rpass-analysis=kernel-resource-usage; waves per SIMD, LDS bytes, VGPRs, SGPRs):
    k_group_block<true>    3, 32480, 56, 82    k_groupb_block<false>  3, 32480, 56, 88
    k_groupf_block         3, 32480, 74, 87    k_groupb_block<true>   3, 32480, 74, 93
(the VGPR figures since the grouped scan's kernels share group_lds.h's group_reduce; 62 and 88 before)"""
import pytest

from test_bytes_key_build import resource_usage

GROUP_LDS, GROUP_WAVES = 32480, 3


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bucket_build")
    return {source: resource_usage(source, tmp) for source in ("group.hip", "group_bucket.hip")}


def bucket_kernels(usage):
    mine = {k: v for k, v in usage["group_bucket.hip"].items() if "k_groupb_block" in k}
    assert len(mine) == 2 and {("ILb1E" in k) for k in mine} == {False, True}, sorted(usage["group_bucket.hip"])
    return mine


def test_bucket_source_has_two_kernels_of_its_own_name(usage):
    bucket_kernels(usage)
    for old in ("k_group_block", "k_groupf_block"):
        assert not [k for k in usage["group_bucket.hip"] if old in k], sorted(usage["group_bucket.hip"])
    assert not [k for k in usage["group.hip"] if "k_groupb_block" in k], sorted(usage["group.hip"])


def test_bucket_kernels_need_no_scratch_and_no_spill(usage):
    for name, figures in bucket_kernels(usage).items():
        print(name, figures)
        assert figures["ScratchSize"] == 0, (name, figures)
        assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (name, figures)


def test_bucket_kernels_keep_the_groupings_lds_and_waves(usage):
    old = {k: v for k, v in usage["group.hip"].items() if "k_group_block" in k and "ILb1E" in k}
    assert len(old) == 1, sorted(usage["group.hip"])
    old = next(iter(old.values()))
    for name, new in bucket_kernels(usage).items():
        assert new["LDS Size"] == old["LDS Size"] == GROUP_LDS, (name, new, old)
        assert new["Occupancy"] == old["Occupancy"] == GROUP_WAVES, (name, new, old)
