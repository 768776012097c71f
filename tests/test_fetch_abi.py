"""CPU tests of the tuple-fetch surface: the header declares the three codec entry points, both shared libraries export them
and cryo_fetch_tuples, the record is 16 bytes, and fetch.hip holds the three kernels and compiles for gfx950 without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cryo_codec_fetch_batch", "cryo_codec_fetch_blocks", "cryo_multi_fetch_blocks")
KERNELS = ("k_fetch_items", "k_fetch_offsets", "k_fetch_copy")


def test_header_declares_and_libraries_export():
    from pg_cryogen_amd import _loader, codec, host
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cryo_codec.h")).read(), flags=re.S)
    L = codec.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in codec.ABI_SYMBOLS and hasattr(L, n), n
    _loader.load()
    for path in (host.HOST_LIB_PATH, host.HOST_TEST_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "cryo_fetch_tuples") and hasattr(lib, "cryo_host_fetch_ops"), path
    assert hasattr(ctypes.CDLL(host.HOST_TEST_LIB_PATH), "cryo_host_set_fetch_ops")
    assert not hasattr(ctypes.CDLL(host.HOST_LIB_PATH), "cryo_host_set_fetch_ops")      # the hook is the test build's only


def test_record_and_status_values():
    from pg_cryogen_amd import codec, host
    txt = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    m = re.search(r"typedef struct \{\s*uint32_t status, len;\s*uint64_t off;\s*\} cryo_fetch_result;", txt)
    assert m, "cryo_fetch_result is {u32 status, u32 len, u64 off}"
    assert codec.FETCH_RESULT.itemsize == 16 and codec.FETCH_RESULT.fields["off"][1] == 8
    body = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    enum = {k: int(v) for k, v in re.findall(r"CRYO_FETCH_(\w+)\s*=\s*(\d+)", body)}
    assert enum == {"OK": 0, "STREAM": 1, "HEADER": 2, "ITEM": 3, "NOITEM": 5, "BADREQ": 6, "OVERLAP": 7}
    assert (codec.FETCH_OK, codec.FETCH_STREAM, codec.FETCH_HEADER, codec.FETCH_ITEM, codec.FETCH_NOITEM, codec.FETCH_BADREQ,
            codec.FETCH_OVERLAP) == (0, 1, 2, 3, 5, 6, 7)
    assert (codec.FETCH_STREAM, codec.FETCH_HEADER, codec.FETCH_ITEM) == (codec.CHECK_STREAM, codec.CHECK_HEADER, codec.CHECK_ITEM)
    assert ctypes.sizeof(host.CryoCodecFetchOps) == 8
    # CryoCodecOps keeps its layout: the fetch is bound through a table of its own
    assert ctypes.sizeof(host.CryoCodecOpsRecode) == ctypes.sizeof(host.CryoCodecOps) + 16


def test_calls_without_a_handle_are_argument_errors():
    from pg_cryogen_amd import codec
    L = codec.lib()
    tot = ctypes.c_uint64(7)
    assert L.cryo_codec_fetch_batch(None, 0, None, None, None, 4096, 0, None, None, 0, None, 0, None, None) == codec.E_ARG
    assert L.cryo_codec_fetch_blocks(None, 0, None, None, 0, 4096, None, None, None, 0, None, ctypes.byref(tot)) == codec.E_ARG
    assert L.cryo_multi_fetch_blocks(None, 0, None, None, 0, 4096, None, None, None, 0, None, ctypes.byref(tot)) == codec.E_ARG


def test_fetch_source_is_in_the_build():
    src = os.path.join(ROOT, "pg_cryogen_amd", "csrc", "fetch.hip")
    txt = open(src).read()
    for k in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, txt), k
    assert "asm" not in re.sub(r"/\*.*?\*/", "", txt, flags=re.S)                     # plain C++ only
    mk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfetch\.hip\b", mk, flags=re.M)
    assert "launch_fetch" in open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "kernels.h")).read()
    hmk = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bfetch\.c\b", hmk, flags=re.M)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_fetch_kernels_compile_for_gfx950(tmp_path):
    """device assembly of fetch.hip: the three kernels are there, for gfx950, without scratch"""
    out = tmp_path / "fetch.s"
    csrc = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", os.path.join(csrc, "fetch.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=csrc)
    assert r.returncode == 0, r.stderr
    asm = out.read_text()
    assert "gfx950" in asm
    for k in KERNELS:
        body = re.search(r"\.amdhsa_kernel \S*%s\S*\n(.*?)\.end_amdhsa_kernel" % k, asm, flags=re.S)
        assert body, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body.group(1)), k
    assert "global_store_dwordx4" in asm        # the 16-byte records
    assert "global_load_dwordx2" in asm and "global_store_dwordx2" in asm      # the 8-byte copies
