"""Build check of the twelve block kernels of the scan calls after they came to share the sweep (scan_sweep.h), the cell
(agg_cell.h) and the grouped scan's first two steps (group_lds.h), CPU only: filter.hip, project.hip, agg.hip, agg_float.hip,
group.hip and group_float.hip are cross-compiled for gfx950 with the compiler's resource-usage remarks.  Sharing text must cost
no kernel scratch, a spill, LDS, a wave per SIMD or a vector register; scalar registers may move and are printed.  BEFORE holds
the figures of the commit before the sharing (hipcc -O3, -Rpass-analysis=kernel-resource-usage).  Resource figures only: no
instruction is looked at.

Figures found (waves per SIMD, LDS bytes, VGPRs, SGPRs; SGPRs before -> after where they moved):
    k_filter_match<false>   8, 0, 38, 82 -> 84      k_filter_match<true>   8, 0, 46, 82 -> 84     k_filterf_match   8, 0, 46, 87 -> 89
    k_project_block<false>  7, 0, 42, 105           k_project_block<true>  8, 0, 49, 89           k_projectf_block  8, 0, 49, 94
    k_agg_block<false>      8, 0, 64, 77            k_agg_block<true>      7, 0, 71, 76 -> 77     k_aggf_block      7, 0, 72, 88 -> 91
    k_group_block<false>    3, 32480, 62, 81 -> 82  k_group_block<true>    3, 32480, 62, 80 -> 82 k_groupf_block    3, 32480, 88, 85 -> 87
The scalar registers that moved hold the block's status through the sweep: a prologue that hands the status back keeps it live
where the nested branches it replaced implied it.  k_agg_block<false> has one register of room below the ceiling
test_truth_key_build.py holds it to, so agg.hip states the status again after its sweep (its comment has the figures).
Since the group kernels share their third step as well (group_reduce; test_group_reduce_build.py) they need 56, 56 and 74 VGPRs."""
import pytest

from test_bytes_key_build import resource_usage

# {source: {kernel name as mangled: (waves per SIMD, LDS bytes, VGPRs, SGPRs)}} before the sharing
BEFORE = {
    "filter.hip": {"k_filter_matchILb0E": (8, 0, 38, 82), "k_filter_matchILb1E": (8, 0, 46, 82), "k_filterf_match": (8, 0, 46, 87)},
    "project.hip": {"k_project_blockILb0E": (7, 0, 42, 105), "k_project_blockILb1E": (8, 0, 49, 89), "k_projectf_block": (8, 0, 49, 94)},
    "agg.hip": {"k_agg_blockILb0E": (8, 0, 64, 77), "k_agg_blockILb1E": (7, 0, 71, 76)},
    "agg_float.hip": {"k_aggf_block": (7, 0, 72, 88)},
    "group.hip": {"k_group_blockILb0E": (3, 32480, 62, 81), "k_group_blockILb1E": (3, 32480, 62, 80)},
    "group_float.hip": {"k_groupf_block": (3, 32480, 88, 85)},
}
CASES = [(source, kernel) for source in sorted(BEFORE) for kernel in sorted(BEFORE[source])]


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scan_sweep_build")
    return {source: resource_usage(source, tmp) for source in sorted(BEFORE)}


def test_the_table_names_twelve_kernels():
    assert len(CASES) == 12


@pytest.mark.parametrize("source,kernel", CASES)
def test_sharing_costs_no_scratch_no_lds_no_wave_and_no_vector_register(usage, source, kernel):
    mine = {k: v for k, v in usage[source].items() if kernel in k}
    assert len(mine) == 1, (kernel, sorted(usage[source]))
    figures = next(iter(mine.values()))
    waves, lds, vgprs, sgprs = BEFORE[source][kernel]
    print(source, kernel, "SGPRs", sgprs, "->", figures["TotalSGPRs"], figures)
    assert figures["ScratchSize"] == 0, (kernel, figures)
    assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (kernel, figures)
    assert figures["LDS Size"] == lds, (kernel, figures)
    assert figures["Occupancy"] == waves, (kernel, figures)
    assert figures["VGPRs"] <= vgprs, (kernel, figures)
