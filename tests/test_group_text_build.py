"""Build check of the text grouping's kernels (k_groupt_block<false>, k_groupt_block<true>), CPU only: group.hip,
group_float.hip, group_bucket.hip and group_text.hip are cross-compiled for gfx950 with the compiler's resource-usage remarks.
The two new kernels need no scratch and no spill, their static LDS -- GroupLds and the text keys' words, one wave per workgroup --
stays within 64 KiB, group_text.hip instantiates none of the old names and the old sources none of the new.  Resource figures
only: no instruction is looked at.

Figures found (hipcc -O3, -Rpass-analysis=kernel-resource-usage; waves per SIMD, LDS bytes, VGPRs, SGPRs):
    k_groupt_block<false>  1, 34800, 60, 86    k_groupt_block<true>   1, 34800, 84, 91
(the VGPR figures since the grouped scan's kernels share group_lds.h's group_reduce; 64 and 90 before)
One wave per SIMD is what the remark reports for a workgroup of one wave with 34 800 bytes of LDS: four workgroups share a CU's 160 KiB."""
import pytest

from test_bytes_key_build import resource_usage

OLD = {"group.hip": ("k_group_block",), "group_float.hip": ("k_groupf_block",), "group_bucket.hip": ("k_groupb_block",)}
TEXT_LDS = 16240 + 2 * 4 * 290 * 8                      # GroupLds, then four words per match and group column


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("group_text_build")
    return {source: resource_usage(source, tmp) for source in list(OLD) + ["group_text.hip"]}


def text_kernels(usage):
    mine = {k: v for k, v in usage["group_text.hip"].items() if "k_groupt_block" in k}
    assert len(mine) == 2 and {("ILb1E" in k) for k in mine} == {False, True}, sorted(usage["group_text.hip"])
    return mine


def test_text_source_has_two_kernels_of_its_own_name(usage):
    text_kernels(usage)
    for names in OLD.values():
        for old in names:
            assert not [k for k in usage["group_text.hip"] if old in k], sorted(usage["group_text.hip"])
    for source in OLD:
        assert not [k for k in usage[source] if "k_groupt_block" in k], sorted(usage[source])


def test_old_sources_keep_their_kernels(usage):
    for source, names in OLD.items():
        for old in names:
            assert [k for k in usage[source] if old in k], (source, sorted(usage[source]))


def test_text_kernels_need_no_scratch_and_no_spill(usage):
    for name, figures in text_kernels(usage).items():
        print(name, figures)
        assert figures["ScratchSize"] == 0, (name, figures)
        assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (name, figures)


def test_text_kernels_lds_is_one_waves_and_within_64_kib(usage):
    for name, figures in text_kernels(usage).items():
        assert figures["LDS Size"] == TEXT_LDS <= 65536, (name, figures)
