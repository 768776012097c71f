"""The host-only part of the scan calls' launch layer (pg_cryogen_amd/csrc/kernels.h: scan_route, group_route, scan_nkeys_arg,
scan_copy_grid, the five *_launch_ok predicates, topn_pack): tests/scan_launch_check.cpp, a program of its own that includes
that header and launches nothing, built with the host sanitizers and run as a child process.  The cases and the values worked
out by hand are in that file's header.  The program also prints the kernel of every route; here those lines are held against
the route table in the docstring of tests/test_gpu_group_routes.py."""
import ast
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the docstring's routes as group_route's arguments: (text, buckets, truth, floats, like)
DOC_ROUTES = {"plain": (0, 0, 0, 0, 0), "truth": (0, 0, 1, 0, 0), "float": (0, 0, 1, 1, 0), "buckets": (0, 1, 1, 0, 0),
              "buckets, float": (0, 1, 1, 1, 0), "text": (2, 0, 1, 0, 0), "text, float": (2, 0, 1, 1, 0)}


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("scan_launch") / "scan_launch_check"
    obj = str(exe) + ".o"
    # the sanitizers are the host side's alone (-Xarch_host: the device side has none), so the link is a step of its own
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-Wno-unused-function", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-c", os.path.join(ROOT, "tests", "scan_launch_check.cpp"),
                    "-o", obj], check=True, capture_output=True, timeout=300)
    subprocess.run([HIPCC, "-fno-gpu-sanitize", "-fsanitize=address,undefined", obj, "-o", str(exe)], check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in r.stderr:
        # the leak check cannot start where the process is traced: the rest of the checks without it
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    return r.stdout


def test_routes_packing_grid_predicates_and_the_topn_pack(output):
    assert output.strip().splitlines()[-1] == "scan launch check ok", output[-4000:]
    assert len(re.findall(r"^scan truth=", output, re.M)) == 8 and len(re.findall(r"^group text=", output, re.M)) == 64


def test_the_group_routes_are_the_gpu_tests_docstring(output):
    doc = ast.get_docstring(ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_group_routes.py")).read()), clean=False)
    table = doc[doc.index("The routes and the kernel each reaches"):].splitlines()[1:]
    rows = {line[:26].strip(): line.split()[-1] for line in table if line.strip()}
    assert set(rows) == set(DOC_ROUTES), rows
    printed = dict(re.findall(r"^group (text=\d buckets=\d truth=\d floats=\d like=\d): (\S+)$", output, re.M))
    for name, (text, buckets, truth, floats, like) in DOC_ROUTES.items():
        assert printed["text=%d buckets=%d truth=%d floats=%d like=%d" % (text, buckets, truth, floats, like)] == rows[name], name
    # every kernel the docstring names is a route's, and the three it leaves out are the pattern kernels'
    assert set(printed.values()) - set(rows.values()) == {"k_groupl_block", "k_groupbl_block", "k_grouptl_block"}
