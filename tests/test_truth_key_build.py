"""Build check of the four kernels that walk tuples with the truth table in their second instantiation, CPU only: filter.hip,
agg.hip, group.hip and project.hip are cross-compiled for gfx950 with the compiler's resource-usage remarks.  The table must not
cost a third instantiation, scratch, a spill, LDS or a wave per SIMD, and the first instantiation -- the code a flag-less
descriptor of integer keys and null tests runs -- must need no more registers than it did before the table existed.  The figures
of the commit before are written out below (hipcc -O3, -Rpass-analysis=kernel-resource-usage).  Resource figures only: no
instruction is looked at."""
import pytest

from test_bytes_key_build import resource_usage

WALKERS = {"filter.hip": "k_filter_match", "agg.hip": "k_agg_block", "group.hip": "k_group_block", "project.hip": "k_project_block"}
# {source: {instantiation: (waves per SIMD, LDS bytes, VGPRs, SGPRs)}} before the truth table
BEFORE = {
    "filter.hip": {False: (8, 0, 38, 84), True: (8, 0, 44, 95)},
    "agg.hip": {False: (8, 0, 64, 78), True: (7, 0, 71, 89)},
    "group.hip": {False: (3, 32480, 62, 82), True: (3, 32480, 62, 93)},
    "project.hip": {False: (7, 0, 44, 106), True: (7, 0, 48, 102)},
}


@pytest.mark.parametrize("source", sorted(WALKERS))
def test_the_table_costs_no_instantiation_no_scratch_and_no_wave(source, tmp_path):
    usage = resource_usage(source, tmp_path)
    mine = {k: v for k, v in usage.items() if WALKERS[source] in k}
    assert len(mine) == 2, sorted(usage)                                  # <false> and <true>: the table lives in <true>
    by_flag = {("ILb1E" in name): figures for name, figures in mine.items()}
    assert set(by_flag) == {False, True}, sorted(mine)
    for flag, figures in by_flag.items():
        waves, lds, vgprs, sgprs = BEFORE[source][flag]
        print(source, flag, figures)
        assert figures["ScratchSize"] == 0, (source, flag, figures)
        assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (source, flag, figures)
        assert figures["Occupancy"] >= waves, (source, flag, figures)
        assert figures["LDS Size"] == lds, (source, flag, figures)
        if not flag:                                                       # the code of integer-only descriptors
            assert figures["VGPRs"] <= vgprs and figures["TotalSGPRs"] <= sgprs, (source, flag, figures)
