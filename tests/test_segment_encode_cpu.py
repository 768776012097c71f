"""CPU tests of the segment-parallel encode switch: the option number in the C header and its Python mirror, and the GUC
pg_cryogen.gpu_encode_segment_kb of the host layer (default 0, allowed values 0 and the powers of two 4 .. 128)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_constant_in_header_and_mirror():
    from pg_cryogen_amd import codec
    hdr = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"\bCRYO_OPT_ENCODE_SEGMENT_BYTES\s*=\s*10\b", hdr)
    assert codec.OPT_ENCODE_SEGMENT_BYTES == 10


def test_guc_default_and_range():
    from pg_cryogen_amd import host
    host.use(production=False)
    try:
        L = host.lib()
        L.cryo_define_compression_gucs()
        assert host.get_int("cryo_gpu_encode_segment_kb_guc") == 0
        ok = {v for v in range(-8, 300) if L.cryo_encode_segment_kb_valid(v)}
        assert ok == {0, 4, 8, 16, 32, 64, 128}
    finally:
        host.use(production=None)


def test_guc_registration():
    """name, default 0, bounds 0 .. 128 and a check hook in the PostgreSQL branch of compression.c"""
    src = open(os.path.join(ROOT, "pg_cryogen_amd", "host", "compression.c")).read()
    m = re.search(r'DefineCustomIntVariable\("pg_cryogen\.gpu_encode_segment_kb",(.*?)\);', src, re.S)
    assert m, "GUC not registered"
    args = [a.strip() for a in re.sub(r'"[^"]*"', '""', m.group(1)).split(",")]
    # short_desc, long_desc, &var, boot, min, max, context, flags, check, assign, show
    assert args[2] == "&cryo_gpu_encode_segment_kb_guc"
    assert args[3:6] == ["0", "0", "128"]
    assert args[6] == "PGC_USERSET" and args[8] == "check_encode_segment_kb"
