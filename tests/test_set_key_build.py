"""Build check of the four kernels that walk tuples (k_filter_match, k_agg_block, k_group_block, k_project_block), CPU only: the
four sources are cross-compiled for gfx950 with the compiler's resource-usage remarks, and both instantiations of each -- the one
that knows byte-string keys and set keys and the one that knows neither -- must need no scratch and spill no register, vector or
scalar.  Resource figures only: no instruction is looked at."""
import pytest

from test_bytes_key_build import resource_usage

WALKERS = {"filter.hip": "k_filter_match", "agg.hip": "k_agg_block", "group.hip": "k_group_block", "project.hip": "k_project_block"}


@pytest.mark.parametrize("source", sorted(WALKERS))
def test_walking_kernels_need_no_scratch_and_spill_nothing(source, tmp_path):
    usage = resource_usage(source, tmp_path)
    mine = {k: v for k, v in usage.items() if WALKERS[source] in k}
    assert len(mine) == 2, sorted(usage)                                  # with a key table and without
    for name, figures in mine.items():
        print(name, figures)
        assert figures["ScratchSize"] == 0, (name, figures)
        assert figures["VGPRs Spill"] == 0 and figures["SGPRs Spill"] == 0, (name, figures)
