"""CPU tests of zstd content checksums (CRYO_OPT_ZSTD_CHECKSUM): the ABI constant, the Python constant, the host shim's GUC,
and the fact about libzstd the GPU encoder rests on."""
import os
import re

import numpy as np
import pytest

import oracle_lib
from pg_cryogen_amd import codec as cc, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_option():
    src = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"\bCRYO_OPT_ZSTD_CHECKSUM\s*=\s*13\b", src)


def test_python_constant():
    assert cc.OPT_ZSTD_CHECKSUM == 13


def test_guc_registered_default_off():
    src = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "compression.c")).read()
    m = re.search(r'DefineCustomEnumVariable\("pg_cryogen\.zstd_checksum",(.*?)\);', src, re.S)
    assert m, "pg_cryogen.zstd_checksum is not registered"
    args = [a.strip() for a in re.split(r",\s*(?![^\"]*\"\s*\")", m.group(1).replace("\n", " ")) if a.strip()]
    assert "&cryo_gpu_zstd_checksum_guc" in args and "PGC_USERSET" in args
    assert args[args.index("&cryo_gpu_zstd_checksum_guc") + 1] == "0"   # boot value: off
    opts = args[args.index("&cryo_gpu_zstd_checksum_guc") + 2]
    entries = dict((k, int(v)) for k, v in re.findall(r'\{"([^"]+)", (\d),', re.search(opts + r"\[\] = \{(.*?)\};", src, re.S).group(1)))
    assert entries["off"] == 0 and entries["on"] == 1
    pg = src[src.index("void cryo_define_compression_gucs"):]
    assert pg.index("zstd_checksum") < pg.index("#else")   # PostgreSQL branch only
    assert "CRYO_OPT_ZSTD_CHECKSUM" in src   # pushed to the handles of the binding
    L = host.lib()
    L.cryo_define_compression_gucs()
    assert host.get_int("cryo_gpu_zstd_checksum_guc") == 0


@pytest.fixture(scope="module")
def stock():
    s = oracle_lib.StockLibs()
    if s.zstd is None:
        pytest.skip("libzstd.so.1 not present")
    return s


@pytest.mark.parametrize("B", [1000, 4096, 65536, 131072, 1 << 20])
def test_libzstd_checksum_frame_is_plain_frame_plus_flag_and_xxh64(stock, oracle, B):
    """ZSTD_compress2 with ZSTD_c_checksumFlag = 1 = ZSTD_compress + descriptor bit 2 + (uint32) XXH64(input, seed 0): what
    lets the GPU encoder add checksums without touching the byte-identical encoders"""
    import ctypes as C
    f = stock.zstd.ZSTD_XXH64
    f.restype, f.argtypes = C.c_uint64, [C.c_void_p, C.c_size_t, C.c_ulonglong]
    raw = np.ascontiguousarray(oracle.synth(2, B & 0xFFFF, B, 0))
    for level in (-5, -1, 1, 3, 9, 19):
        plain = stock.zstd_compress(raw, level)
        ck = stock.zstd_compress2(raw, {oracle_lib.ZSTD_C_COMPRESSION_LEVEL: level, oracle_lib.ZSTD_C_CHECKSUM_FLAG: 1})
        want = plain.copy()
        want[4] |= 0x04
        trailer = np.frombuffer((int(f(raw.ctypes.data, raw.nbytes, 0)) & 0xFFFFFFFF).to_bytes(4, "little"), np.uint8)
        assert np.array_equal(ck, np.concatenate([want, trailer])), (B, level)
