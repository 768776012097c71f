"""CPU tests of the recompression surface: the header declares the three codec entry points, both shared libraries export
them and cryo_recompress_relation, and recode.hip holds the two kernels and compiles for gfx950 without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cryo_codec_recode_batch", "cryo_codec_recode_blocks", "cryo_multi_recode_blocks")


def test_header_declares_and_libraries_export():
    from pg_cryogen_amd import _loader, codec, host
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cryo_codec.h")).read(), flags=re.S)
    L = codec.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in codec.ABI_SYMBOLS and hasattr(L, n), n
    _loader.load()
    for path in (host.HOST_LIB_PATH, host.HOST_TEST_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "cryo_recompress_relation"), path
    hdr = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "compression.h")).read()
    ops = hdr[hdr.index("typedef struct CryoCodecOps {"):hdr.index("} CryoCodecOps;")]
    members = re.findall(r"\(\*(\w+)\)\(", ops)
    assert members[-2:] == ["check_blocks", "recode_blocks"]          # one more trailing member, the rest as they were
    assert ctypes.sizeof(host.CryoCodecOpsRecode) == ctypes.sizeof(host.CryoCodecOpsCheck) + 8
    assert ctypes.sizeof(host.CryoCodecOpsCheck) == ctypes.sizeof(host.CryoCodecOps) + 8


def test_calls_without_a_handle_are_argument_errors():
    from pg_cryogen_amd import codec
    L = codec.lib()
    assert L.cryo_codec_recode_blocks(None, 0, None, None, 0, 4096, 1, 1, None, 0, None, None, None) == codec.E_ARG
    assert L.cryo_codec_recode_batch(None, 0, None, None, None, 4096, 0, 1, 1, None, 0, None, None) == codec.E_ARG
    assert L.cryo_multi_recode_blocks(None, 0, None, None, 0, 4096, 1, 1, None, 0, None, None, None) == codec.E_ARG


def test_recode_source_is_in_the_build():
    src = os.path.join(ROOT, "pg_cryogen_amd", "csrc", "recode.hip")
    txt = open(src).read()
    for k in ("k_recode_offsets", "k_recode_pack"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, txt), k
    mk = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\brecode\.hip\b", mk, flags=re.M)
    kh = open(os.path.join(ROOT, "pg_cryogen_amd", "csrc", "kernels.h")).read()
    assert "launch_recode_offsets" in kh and "launch_recode_pack" in kh


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_recode_kernels_compile_for_gfx950(tmp_path):
    """device assembly of recode.hip: both kernels are there, for gfx950, without scratch"""
    out = tmp_path / "recode.s"
    csrc = os.path.join(ROOT, "pg_cryogen_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "--cuda-device-only", "-S", os.path.join(csrc, "recode.hip"), "-o", str(out)],
                       capture_output=True, text=True, timeout=600, cwd=csrc)
    assert r.returncode == 0, r.stderr
    asm = out.read_text()
    assert "gfx950" in asm
    for k in ("k_recode_offsets", "k_recode_pack"):
        body = re.search(r"\.amdhsa_kernel \S*%s\S*\n(.*?)\.end_amdhsa_kernel" % k, asm, flags=re.S)
        assert body, k
        assert re.search(r"\.amdhsa_private_segment_fixed_size 0\b", body.group(1)), k
    assert "global_load_dwordx4" in asm and "global_store_dwordx4" in asm      # the 16-byte copies of the pack
