"""What the host-buffer codec calls share (pg_cryogen_amd/csrc/host_stage.h: the layout of the staged streams, the chunk cut of
the pipelined staging) against brute force: tests/host_stage_check.cpp, a program of its own that includes that header alone,
built with the host sanitizers and run as a child process.  The cases are listed in that file's header."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
# the runtimes linked into the program: it then runs whatever else the environment has the loader bring in first
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _sanitizers_build(tmp_path):
    src = tmp_path / "trivial.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + SANITIZE + [str(src), "-o", str(tmp_path / "trivial")], capture_output=True, timeout=120)
    return r.returncode == 0


def test_the_stream_layout_and_the_chunk_cut_against_brute_force(tmp_path):
    if not _sanitizers_build(tmp_path):
        pytest.skip("this g++ cannot link a program with -fsanitize=address")
    exe = tmp_path / "host_stage_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + SANITIZE
                   + ["-I" + CSRC, os.path.join(ROOT, "tests", "host_stage_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in r.stderr:
        # the leak check cannot start where the process is traced: the rest of the checks without it
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "host stage check ok", r.stderr[-4000:]
