"""Child process of tests/test_gpu_encode_verify.py::test_failure_paths_with_injected_fault (not collected by pytest).

It runs against a CRYO_DEBUG build of the codec library (CRYO_CODEC_LIB), whose compress calls flip one byte of the encoded
slot named by CRYO_VERIFY_FAULT="block:byte" before verification.  Every compress entry point must then report
CRYO_E_VERIFY for that block, with the offset of its first differing byte: the one the oracle finds in the flipped stream.
Prints "verify-fault ok" when every check passed."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib  # noqa: E402
from pg_cryogen_amd import Codec, METHOD_LZ4, METHOD_ZSTD, codec as cc  # noqa: E402

B, FLIP = 131072, 5000


def expected(ora, method, raw):
    """first differing byte of the block whose stream has byte FLIP flipped (the GPU encoders' output is the oracle's)"""
    comp = (ora.lz4_compress(raw, 1) if method == METHOD_LZ4 else ora.zstd_compress(raw, 1)).copy()
    comp[FLIP] ^= 0x5A
    r, dec = (ora.lz4_decompress if method == METHOD_LZ4 else ora.zstd_decompress)(comp, B)
    assert r == B
    d = np.nonzero(dec[:B] != raw)[0]
    assert len(d)
    return int(d[0])


def fault(block):
    os.environ["CRYO_VERIFY_FAULT"] = "%d:%d" % (block, FLIP)


def main():
    ora = oracle_lib.Oracle()
    rng = np.random.default_rng(31)
    n = 160
    raw = rng.integers(0, 256, n * B, dtype=np.uint8)   # incompressible: one literal run / raw blocks, FLIP lands in data
    blk = lambda i: raw[i * B:(i + 1) * B]
    with Codec(0) as c:
        L = c.L
        c.set_option(cc.OPT_ENCODE_VERIFY, 1)
        for method in (METHOD_LZ4, METHOD_ZSTD):
            cap = cc.bound(method, B)
            # device batch: the status of the damaged block only
            fault(2)
            d_src, d_dst, d_sz, d_st = c.alloc(4 * B), c.alloc(4 * cap), c.alloc(16), c.alloc(16)
            d_src.upload(raw[:4 * B])
            c.compress_batch(method, 1, d_src, B, B, 4, d_dst, cap, d_sz, d_st)
            c.sync()
            st = d_st.download(dtype=np.int32)
            assert list(st) == [0, 0, cc.E_VERIFY, 0], st
            for x in (d_src, d_dst, d_sz, d_st):
                x.free()
            # single block
            fault(0)
            out = np.zeros(cap, np.uint8)
            osz = C.c_size_t()
            rc = L.cryo_codec_compress_block(c.h, method, 1, blk(7).ctypes.data, B, out.ctypes.data, cap, C.byref(osz))
            assert rc == cc.E_VERIFY, rc
            want = expected(ora, method, blk(7))
            assert c.last_verify_failure() == (0, want), (c.last_verify_failure(), want)
            assert ("block 0 failed verification at byte %d" % want) in L.cryo_codec_last_error(c.h).decode()
            # K blocks, one-shot and pipelined
            for count, bad, pipe_min in ((8, 5, 64 << 20), (n, 131, 1 << 20)):
                c.set_option(cc.OPT_PIPE_MIN_BYTES, pipe_min)
                fault(bad)
                dst = np.zeros(count * cap, np.uint8)
                sz = (C.c_uint32 * count)()
                rc = L.cryo_codec_compress_blocks(c.h, method, 1, raw.ctypes.data, B, count, dst.ctypes.data, cap, sz)
                assert rc == cc.E_VERIFY, rc
                assert c.last_verify_failure() == (bad, expected(ora, method, blk(bad))), (count, c.last_verify_failure())
            c.set_option(cc.OPT_PIPE_MIN_BYTES, 64 << 20)
            # no fault: the next call reports no failure
            os.environ.pop("CRYO_VERIFY_FAULT")
            dst = np.zeros(4 * cap, np.uint8)
            sz = (C.c_uint32 * 4)()
            assert L.cryo_codec_compress_blocks(c.h, method, 1, raw.ctypes.data, B, 4, dst.ctypes.data, cap, sz) == 0
            assert c.last_verify_failure() is None
            # two handles: block i goes to handle i mod 2, the fault hits local block 1 of each share (global blocks 2 and
            # 3); the multi call reports the lowest global index
            h = C.c_void_p()
            assert L.cryo_multi_open((C.c_int * 2)(0, 0), 2, C.byref(h)) == 0
            try:
                assert L.cryo_multi_set_option(h, cc.OPT_ENCODE_VERIFY, 1) == 0
                fault(1)
                dst = np.zeros(6 * cap, np.uint8)
                sz = (C.c_uint32 * 6)()
                assert L.cryo_multi_compress_blocks(h, method, 1, raw.ctypes.data, B, 6, dst.ctypes.data, cap, sz) == cc.E_VERIFY
                b, o = C.c_uint64(), C.c_uint32()
                assert L.cryo_multi_last_verify_failure(h, C.byref(b), C.byref(o)) == 1
                assert (b.value, o.value) == (2, expected(ora, method, blk(2))), (b.value, o.value)
                os.environ.pop("CRYO_VERIFY_FAULT")
                assert L.cryo_multi_compress_blocks(h, method, 1, raw.ctypes.data, B, 6, dst.ctypes.data, cap, sz) == 0
                assert L.cryo_multi_last_verify_failure(h, C.byref(b), C.byref(o)) == 0
            finally:
                L.cryo_multi_close(h)
    print("verify-fault ok")


if __name__ == "__main__":
    main()
