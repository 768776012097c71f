"""Build check of the grouped scan's block kernels on the one run reduction (group_lds.h: group_reduce) and of the two offsets
kernels on the one scan (heap_block.h: offsets_of_rows), CPU only: group.hip, group_float.hip, group_bucket.hip, group_text.hip and
topn.hip are cross-compiled for gfx950 with the compiler's resource-usage remarks.  Each of the seven block instantiations needs no
scratch and no spill, keeps the LDS and the waves per SIMD it had with a reduction of its own, and needs no more vector and no more
scalar registers than it did; the two offsets kernels keep their figures; each group source holds exactly the block kernels of its
own name.  Resource figures only: no instruction is looked at.

Figures with a reduction per kernel, the bounds here (waves per SIMD, LDS bytes, VGPRs, SGPRs), and the VGPRs found since:
    k_group_block<false>   3, 32480, 62, 82  -> 56     k_group_block<true>    3, 32480, 62, 82  -> 56
    k_groupf_block         3, 32480, 88, 87  -> 74
    k_groupb_block<false>  3, 32480, 62, 88  -> 56     k_groupb_block<true>   3, 32480, 88, 93  -> 74
    k_groupt_block<false>  1, 34800, 64, 86  -> 60     k_groupt_block<true>   1, 34800, 90, 91  -> 84
    k_group_offsets, k_topn_offsets: 36 VGPRs, 36 SGPRs, 32 bytes of LDS, before and since
The SGPRs did not move."""
import pytest

from test_bytes_key_build import resource_usage

# source -> {(kernel, mangled template argument or None): (waves per SIMD, LDS bytes, VGPRs, SGPRs)}
BLOCKS = {
    "group.hip": {("k_group_block", "ILb0E"): (3, 32480, 62, 82), ("k_group_block", "ILb1E"): (3, 32480, 62, 82)},
    "group_float.hip": {("k_groupf_block", None): (3, 32480, 88, 87)},
    "group_bucket.hip": {("k_groupb_block", "ILb0E"): (3, 32480, 62, 88), ("k_groupb_block", "ILb1E"): (3, 32480, 88, 93)},
    "group_text.hip": {("k_groupt_block", "ILb0E"): (1, 34800, 64, 86), ("k_groupt_block", "ILb1E"): (1, 34800, 90, 91)},
}
OFFSETS = {"group.hip": "k_group_offsets", "topn.hip": "k_topn_offsets"}
OFFSETS_FIGURES = (36, 36, 32)                          # VGPRs, SGPRs, LDS bytes


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("group_reduce_build")
    return {source: resource_usage(source, tmp) for source in sorted(set(BLOCKS) | set(OFFSETS))}


def instantiation(usage, source, kernel, arg):
    mine = {k: v for k, v in usage[source].items() if kernel + (arg or "E") in k}
    assert len(mine) == 1, (kernel, arg, sorted(usage[source]))
    return next(iter(mine.values()))


CASES = [(source, kernel, arg) for source in sorted(BLOCKS) for kernel, arg in sorted(BLOCKS[source], key=str)]


@pytest.mark.parametrize("source,kernel,arg", CASES, ids=["%s%s" % (k, {None: "", "ILb0E": "<false>", "ILb1E": "<true>"}[a]) for _, k, a in CASES])
def test_block_kernels_keep_their_figures(usage, source, kernel, arg):
    waves, lds, vgprs, sgprs = BLOCKS[source][(kernel, arg)]
    figures = instantiation(usage, source, kernel, arg)
    print(kernel, arg, figures)
    assert figures["ScratchSize"] == 0, figures
    assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, figures
    assert figures["LDS Size"] == lds, figures
    assert figures["Occupancy"] == waves, figures
    assert figures["VGPRs"] <= vgprs, figures
    assert figures["TotalSGPRs"] <= sgprs, figures


@pytest.mark.parametrize("source", sorted(OFFSETS))
def test_offsets_kernels_keep_their_figures(usage, source):
    figures = instantiation(usage, source, OFFSETS[source], None)
    print(OFFSETS[source], figures)
    assert figures["ScratchSize"] == 0, figures
    assert (figures["VGPRs"], figures["TotalSGPRs"], figures["LDS Size"]) == OFFSETS_FIGURES, figures


@pytest.mark.parametrize("source", sorted(BLOCKS))
def test_each_group_source_holds_the_block_kernels_of_its_own_name(usage, source):
    blocks = sorted(k for k in usage[source] if "_block" in k)
    assert len(blocks) == len(BLOCKS[source]), blocks
    for kernel, arg in BLOCKS[source]:
        instantiation(usage, source, kernel, arg)
