"""What the host walks share (pg_cryogen_amd/host/walk.h: the read and sort of a block, the relation walk, the window) at a window
of 4 entries and 3.5 streams' bytes, by itself and under cryo_recompress_relation and cryo_fetch_tuples: tests/host_walk_check.c, a
program of its own with stub codec calls, built with the host sanitizers and run as a child process.  The cases and the expected
flushes, slots and calls are worked out in that file's header."""
import ctypes as C
import os
import subprocess

import pytest

from pg_cryogen_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "pg_cryogen_amd", "host")
SOURCES = [os.path.join(ROOT, "tests", "host_walk_check.c")] + [
    os.path.join(HOST, f) for f in ("walk.c", "staging.c", "storage.c", "scan_iterator.c", "recompress.c", "fetch.c")]
# the runtimes linked into the program: it then runs whatever else the environment has the loader bring in first
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _sanitizers_build(tmp_path):
    src = tmp_path / "trivial.c"
    src.write_text("int main(void) { return 0; }\n")
    r = subprocess.run(["gcc"] + SANITIZE + [str(src), "-o", str(tmp_path / "trivial")], capture_output=True, timeout=120)
    return r.returncode == 0


def test_the_shared_walk_at_a_small_window(tmp_path):
    if not _sanitizers_build(tmp_path):
        pytest.skip("this gcc cannot link a program with -fsanitize=address")
    exe = tmp_path / "host_walk_check"
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-DCRYO_HOST_TEST_HOOKS"] + SANITIZE
                   + ["-I" + HOST, "-I" + os.path.join(ROOT, "include")] + SOURCES + ["-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in r.stderr:
        # the leak check cannot start where the process is traced: the rest of the checks without it
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip() == "host walk check ok", r.stderr[-4000:]


def test_the_window_hooks_are_the_test_builds_only():
    from pg_cryogen_amd import _loader
    _loader.load()
    for hook in ("cryo_recompress_set_window", "cryo_fetch_set_window"):
        assert hasattr(C.CDLL(host.HOST_TEST_LIB_PATH), hook)
        assert not hasattr(C.CDLL(host.HOST_LIB_PATH), hook)
    assert not hasattr(C.CDLL(host.HOST_LIB_PATH), "cryo_window_limits")
