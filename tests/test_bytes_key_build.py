"""Build check of the three kernels that walk tuples (k_filter_match, k_agg_block, k_group_block), CPU only: filter.hip, agg.hip
and group.hip are cross-compiled for gfx950 with the compiler's resource-usage remarks, and every instantiation of the three --
with and without byte-string keys -- must need no scratch.  Resource figures only: no instruction is looked at."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
WALKERS = {"filter.hip": "k_filter_match", "agg.hip": "k_agg_block", "group.hip": "k_group_block"}


def resource_usage(source, tmp_path):
    """{mangled kernel name: {figure: value}} from -Rpass-analysis=kernel-resource-usage"""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source), "-o",
                        str(tmp_path / (source + ".o"))], capture_output=True, text=True, timeout=600, cwd=CSRC)
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


@pytest.mark.parametrize("source", sorted(WALKERS))
def test_walking_kernels_need_no_scratch(source, tmp_path):
    usage = resource_usage(source, tmp_path)
    mine = {k: v for k, v in usage.items() if WALKERS[source] in k}
    assert len(mine) == 2, sorted(usage)                                  # with byte-string keys and without
    for name, figures in mine.items():
        print(name, figures)
        assert figures["ScratchSize"] == 0, (name, figures)
        assert figures.get("VGPRs Spill", 0) == 0 and figures.get("SGPRs Spill", 0) == 0, (name, figures)
