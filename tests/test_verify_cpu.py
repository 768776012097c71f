"""CPU tests of write verification (CRYO_OPT_ENCODE_VERIFY, cryo_codec_verify_batch, pg_cryogen.gpu_verify_writes): the ABI
additions exist in the header and the built library, the GUC is registered with its default, and the host layer turns a
CRYO_E_VERIFY from the codec into its ERROR text -- through a small codec stand-in whose compress call fails verification."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pg_cryogen_amd import codec as cc, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 131072


def _header():
    return open(os.path.join(ROOT, "include", "cryo_codec.h")).read()


def test_header_declares_status_option_and_entry_points():
    h = _header()
    assert re.search(r"CRYO_E_VERIFY\s*=\s*-8\b", h)
    assert re.search(r"CRYO_OPT_ENCODE_VERIFY\s*=\s*12\b", h)
    for name in ("cryo_codec_verify_batch", "cryo_codec_last_verify_failure", "cryo_multi_last_verify_failure"):
        assert re.search(r"\bint\s+%s\s*\(" % name, h), name
    decl = re.search(r"int cryo_codec_verify_batch\((.*?)\);", h, re.S).group(1)
    assert len([a for a in decl.split(",") if a.strip()]) == 11
    # the contract says what verification does not prove
    assert "identically in an encoder and its decoder" in h


def test_library_exports_and_python_constants():
    L = cc.lib()
    for name in ("cryo_codec_verify_batch", "cryo_codec_last_verify_failure", "cryo_multi_last_verify_failure"):
        assert hasattr(L, name) and name in cc.ABI_SYMBOLS
    assert cc.E_VERIFY == -8 and cc.OPT_ENCODE_VERIFY == 12 and cc.VERIFY_NONE == 0xFFFFFFFF
    assert "CRYO_E_VERIFY" in str(cc.CryoError(cc.E_VERIFY, "compress_blocks"))
    # the new member of CryoCodecOps sits behind the ones the doubles fill
    assert [f for f, _ in host.CryoCodecOps._fields_][-1] == "last_verify_failure"


def test_verify_calls_reject_bad_arguments_without_a_gpu():
    L = cc.lib()
    assert L.cryo_codec_verify_batch(None, 0, None, 0, B, 1, None, None, None, None, None) == cc.E_ARG
    b, o = C.c_uint64(), C.c_uint32()
    assert L.cryo_codec_last_verify_failure(None, C.byref(b), C.byref(o)) == cc.E_ARG
    assert L.cryo_multi_last_verify_failure(None, C.byref(b), C.byref(o)) == cc.E_ARG


def test_guc_registered_default_off():
    src = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "compression.c")).read()
    m = re.search(r'DefineCustomEnumVariable\("pg_cryogen\.gpu_verify_writes",(.*?)\);', src, re.S)
    assert m, "pg_cryogen.gpu_verify_writes is not registered"
    args = [a.strip() for a in re.split(r",\s*(?![^\"]*\"\s*\")", m.group(1).replace("\n", " ")) if a.strip()]
    assert "&cryo_gpu_verify_writes_guc" in args and "PGC_USERSET" in args
    assert args[args.index("&cryo_gpu_verify_writes_guc") + 1] == "0"   # boot value: off
    opts = re.search(r"verify_writes_options\[\] = \{(.*?)\};", src, re.S).group(1)
    entries = dict((k, int(v)) for k, v in re.findall(r'\{"([^"]+)", (\d),', opts))
    # every value PostgreSQL's parse_bool() accepts: true / false / yes / no and their prefixes, on, of / off, 1 / 0
    want = {w[:k]: v for w, v in (("true", 1), ("false", 0), ("yes", 1), ("no", 0)) for k in range(1, len(w) + 1)}
    want.update({"on": 1, "of": 0, "off": 0, "1": 1, "0": 0})
    assert entries == want
    pg = src[src.index("void cryo_define_compression_gucs"):]
    assert pg.index("gpu_verify_writes") < pg.index("#else")   # PostgreSQL branch only
    L = host.lib()
    L.cryo_define_compression_gucs()
    assert host.get_int("cryo_gpu_verify_writes_guc") == 0


class VerifyFailingOps:
    """compress_blocks reports CRYO_E_VERIFY for block `bad` (as the GPU codec does with verification on and a block that
    does not decode back to its input); last_verify_failure reports (bad, offset)"""

    def __init__(self, bad=0, offset=1234, report=True):
        self.bad, self.offset, self.calls = bad, offset, 0
        self._bound = host.BOUND_FN(lambda m, n: n + n // 255 + 16 if m == 0 else n + (n >> 8) + 64)
        self._comp = host.COMPRESS_FN(self.compress)
        self._decomp = host.DECOMPRESS_FN(lambda *a: -1)
        self._vf = host.VERIFY_FAILURE_FN(self.failure)
        self.ops = host.CryoCodecOps(self._bound, self._comp, self._decomp, None)
        if report:
            self.ops.last_verify_failure = C.cast(self._vf, C.c_void_p)

    def compress(self, ctx, method, param, src, bs, n, dst, stride, out_size):
        self.calls += 1
        for i in range(n):
            out_size[i] = 100
        return cc.E_VERIFY

    def failure(self, ctx, block, offset):
        block[0], offset[0] = self.bad, self.offset
        return 1


@pytest.fixture()
def H():
    L = host.lib()
    errors = []
    handler = host.ERROR_HANDLER(lambda lvl, msg: errors.append((lvl, msg.decode())) if lvl >= 20 else None)
    L.cryo_compat_set_error_handler(handler)
    host.set_block_size(B)
    L.cryo_define_compression_gucs()
    yield L, errors
    L.cryo_host_set_codec_ops(None)
    L.cryo_compat_set_error_handler(host.ERROR_HANDLER(0))
    host.set_block_size(1 << 20)


@pytest.mark.parametrize("method", [host.COMP_LZ4, host.COMP_ZSTD])
def test_cryo_compress_raises_verification_error_with_offset(H, method):
    L, errors = H
    dbl = VerifyFailingOps(offset=4321)
    L.cryo_host_set_codec_ops(C.byref(dbl.ops))
    raw = np.arange(B, dtype=np.uint32).astype(np.uint8)
    n = C.c_size_t(0)
    p = L.cryo_compress(method, raw.ctypes.data, C.byref(n))
    assert not p and dbl.calls == 1
    assert errors == [(20, "pg_cryogen: compressed block failed verification at byte 4321")]


def test_cryo_compress_verification_error_without_offset(H):
    """a stream the decoders reject has no first differing byte; a codec without the optional member reports none either"""
    L, errors = H
    for dbl in (VerifyFailingOps(offset=0xFFFFFFFF), VerifyFailingOps(report=False)):
        errors.clear()
        L.cryo_host_set_codec_ops(C.byref(dbl.ops))
        raw = np.zeros(B, np.uint8)
        n = C.c_size_t(0)
        assert not L.cryo_compress(host.COMP_LZ4, raw.ctypes.data, C.byref(n))
        assert errors == [(20, "pg_cryogen: compressed block failed verification (its stream does not decode)")]


def test_write_behind_reports_verification_failure_and_writes_no_page(H):
    L, errors = H
    dbl = VerifyFailingOps(bad=1)
    L.cryo_host_set_codec_ops(C.byref(dbl.ops))
    mem = L.cryo_memrel_create()
    try:
        rel = host.CryoRel()
        L.cryo_memrel_bind(mem, 9, C.byref(rel))
        fb = (C.c_uint32 * 2)(host.InvalidBlockNumber, host.InvalidBlockNumber)
        data = np.zeros(2 * B, np.uint8)
        before = L.cryo_memrel_nblocks(mem)
        assert L.cryo_stage_write_batch(C.byref(rel), data.ctypes.data, 2, host.COMP_ZSTD, 7, fb) == cc.E_VERIFY
        assert L.cryo_memrel_nblocks(mem) == before and list(fb) == [host.InvalidBlockNumber] * 2
        assert dbl.calls == 1
    finally:
        L.cryo_memrel_destroy(mem)
