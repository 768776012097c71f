"""CPU tests of the strategy switch of segment-parallel zstd encode: the option number in the C header and its Python
mirror, and the GUC pg_cryogen.gpu_encode_segment_zstd_strategy of the host layer (enum fast .. btlazy2 = 1 .. 6, default
fast)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPRESSION_C = os.path.join(ROOT, "pg_cryogen_amd", "host", "compression.c")


def test_option_constant_in_header_and_mirror():
    from pg_cryogen_amd import codec
    hdr = open(os.path.join(ROOT, "include", "cryo_codec.h")).read()
    assert re.search(r"\bCRYO_OPT_ENCODE_SEGMENT_ZSTD_STRATEGY\s*=\s*11\b", hdr)
    assert codec.OPT_ENCODE_SEGMENT_ZSTD_STRATEGY == 11


def test_guc_default_and_valid_set():
    from pg_cryogen_amd import host
    host.use(production=False)
    try:
        L = host.lib()
        L.cryo_define_compression_gucs()
        assert host.get_int("cryo_gpu_encode_segment_zstd_strategy_guc") == 1
        ok = {v for v in range(-8, 300) if L.cryo_encode_segment_zstd_strategy_valid(v)}
        assert ok == {1, 2, 3, 4, 5, 6}
    finally:
        host.use(production=None)


def test_guc_registration():
    """name, variable, default `fast`, PGC_USERSET and the six entries in the PostgreSQL branch of compression.c"""
    src = open(COMPRESSION_C).read()
    m = re.search(r'DefineCustomEnumVariable\("pg_cryogen\.gpu_encode_segment_zstd_strategy",(.*?)\);', src, re.S)
    assert m, "GUC not registered"
    args = [a.strip() for a in re.sub(r'"[^"]*"', '""', m.group(1)).split(",")]
    # short_desc, long_desc, &var, boot, options, context, flags, check, assign, show
    assert args[2] == "&cryo_gpu_encode_segment_zstd_strategy_guc"
    assert args[3] == "1"
    assert args[5] == "PGC_USERSET"
    opts = args[4]
    t = re.search(r"config_enum_entry\s+%s\[\]\s*=\s*\{(.*?)\};" % re.escape(opts), src, re.S)
    assert t, "option table not found"
    entries = re.findall(r'\{"(\w+)",\s*(\d+),\s*false\}', t.group(1))
    assert entries == [("fast", "1"), ("dfast", "2"), ("greedy", "3"), ("lazy", "4"), ("lazy2", "5"), ("btlazy2", "6")]
    assert re.search(r"\{NULL,\s*0,\s*false\}\s*$", t.group(1).strip())
    # the PostgreSQL branch is where it is registered
    pg = src[src.index("#ifdef CRYO_HAVE_POSTGRES\n    static const struct config_enum_entry compression_method_options"):]
    assert pg.index("gpu_encode_segment_zstd_strategy") < pg.index("#else")
