"""ctypes binding of libcryo_host.so: the C host side that mirrors the reference's
compression.h / storage.c / cache.h surfaces plus the page-chain staging
(pg_cryogen_amd/host/*.h).  Driver for tests; the library itself is plain C."""
import ctypes as C
import os

from . import _loader

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libcryo_host.so")            # production: no test hooks exported
HOST_TEST_LIB_PATH = os.path.join(_HERE, "libcryo_host_test.so")  # + cryo_host_set_codec_ops (tests/conftest.py asks for it)

COMP_LZ4, COMP_ZSTD = 0, 1
(CRYO_ERR_SUCCESS, CRYO_ERR_DECOMPRESSION_FAILED, CRYO_ERR_WRONG_STARTING_BLOCK, CRYO_ERR_EMPTY_BLOCK,
 CRYO_ERR_CACHE_IS_FULL) = range(5)
InvalidBlockNumber = 0xFFFFFFFF
BLCKSZ = 8192

BOUND_FN = C.CFUNCTYPE(C.c_size_t, C.c_int, C.c_size_t)
COMPRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                          C.c_size_t, C.POINTER(C.c_uint32))
DECOMPRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                            C.c_void_p, C.c_size_t, C.POINTER(C.c_int32))
ERROR_HANDLER = C.CFUNCTYPE(None, C.c_int, C.c_char_p)
VERIFY_FAILURE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32))
CHECK_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                              C.c_size_t, C.POINTER(C.c_uint32))
RECODE_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                               C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint32), C.POINTER(C.c_int32))
FETCH_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                              C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint16), C.c_void_p, C.c_size_t, C.c_void_p,
                              C.POINTER(C.c_uint64))
FILTER_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                               C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                               C.POINTER(C.c_uint64))
AGG_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                            C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
GROUP_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                              C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                              C.POINTER(C.c_uint64))
PROJECT_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t,
                                C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                C.POINTER(C.c_uint64))
TOPN_BLOCKS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64))
CRYO_CHECK_CHAIN, CRYO_CHECK_METHOD = 16, 17   # host-only reasons of check.h (beside cryo_check_reason 0..4)


class CryoCodecOps(C.Structure):
    """host/compression.h's CryoCodecOps WITHOUT its last member, check_blocks: 8 bytes shorter than the C struct.  Enough
    for every host call except cryo_check_relation, which reads check_blocks and would read it past the end of an object of
    this layout.  A double that may reach cryo_check_relation must be built from CryoCodecOpsCheck."""
    _fields_ = [("bound", BOUND_FN), ("compress_blocks", COMPRESS_FN), ("decompress_blocks", DECOMPRESS_FN),
                ("ctx", C.c_void_p), ("decompress_blocks_scatter", C.c_void_p),      # optional members: NULL in test doubles
                ("decompress_blocks_keyed", C.c_void_p), ("pool_invalidate", C.c_void_p),
                ("last_verify_failure", C.c_void_p)]


class CryoCodecOpsCheck(CryoCodecOps):
    """CryoCodecOps with its last optional member, check_blocks (CHECK_BLOCKS_FN or NULL), which cryo_check_relation reads:
    a double that reaches cryo_check_relation is built from this layout"""
    _fields_ = [("check_blocks", C.c_void_p)]


class CryoCodecOpsRecode(CryoCodecOpsCheck):
    """CryoCodecOpsCheck with the last optional member, recode_blocks (RECODE_BLOCKS_FN or NULL), which only
    cryo_recompress_relation reads: a double that reaches it is built from this layout"""
    _fields_ = [("recode_blocks", C.c_void_p)]


class CryoCodecFetchOps(C.Structure):
    """host/compression.h's one-function table of the tuple fetch (FETCH_BLOCKS_FN), bound beside a CryoCodecOps double with
    cryo_host_set_fetch_ops (test build)"""
    _fields_ = [("fetch_blocks", FETCH_BLOCKS_FN)]


class CryoCodecFilterOps(C.Structure):
    """host/compression.h's one-function table of the scan filter (FILTER_BLOCKS_FN), bound beside a CryoCodecOps double with
    cryo_host_set_filter_ops (test build)"""
    _fields_ = [("filter_blocks", FILTER_BLOCKS_FN)]


class CryoCodecAggOps(C.Structure):
    """host/compression.h's one-function table of the scan aggregate (AGG_BLOCKS_FN), bound beside a CryoCodecOps double with
    cryo_host_set_agg_ops (test build)"""
    _fields_ = [("agg_blocks", AGG_BLOCKS_FN)]


class CryoCodecGroupOps(C.Structure):
    """host/compression.h's one-function table of the grouped scan (GROUP_BLOCKS_FN), bound beside a CryoCodecOps double with
    cryo_host_set_group_ops (test build)"""
    _fields_ = [("group_blocks", GROUP_BLOCKS_FN)]


class CryoCodecProjectOps(C.Structure):
    """host/compression.h's one-function table of the projecting scan (PROJECT_BLOCKS_FN), bound beside a CryoCodecOps double
    with cryo_host_set_project_ops (test build)"""
    _fields_ = [("project_blocks", PROJECT_BLOCKS_FN)]


class CryoCodecTopnOps(C.Structure):
    """host/compression.h's one-function table of the ordered scan (TOPN_BLOCKS_FN), bound beside a CryoCodecOps double with
    cryo_host_set_topn_ops (test build)"""
    _fields_ = [("topn_blocks", TOPN_BLOCKS_FN)]


class CryoRel(C.Structure):
    _fields_ = [("relid", C.c_uint), ("handle", C.c_void_p), ("ops", C.c_void_p)]


class CryoCheckReport(C.Structure):
    _fields_ = [("block", C.c_uint32), ("reason", C.c_uint32), ("offset", C.c_uint32), ("npages", C.c_uint32)]


class CryoCheckTotals(C.Structure):
    _fields_ = [("blocks", C.c_uint64), ("empty_pages", C.c_uint64), ("bad", C.c_uint64), ("codec_calls", C.c_uint64)]


CHECK_REPORT_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoCheckReport))


class CryoRecompressTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("blocks", "recoded", "verbatim", "skipped", "empty_pages", "bytes_in", "bytes_out",
                                          "pages_in", "pages_out", "codec_calls")]


class CryoFetchPage(C.Structure):
    _fields_ = [("block", C.c_uint32), ("ntuples", C.c_int32), ("offsets", C.POINTER(C.c_uint16))]


class CryoFetchedTuple(C.Structure):
    _fields_ = [("block", C.c_uint32), ("pos", C.c_uint16), ("created_xid", C.c_uint32), ("data", C.c_void_p),
                ("len", C.c_uint32)]


class CryoFetchReport(C.Structure):
    _fields_ = [("block", C.c_uint32), ("reason", C.c_uint32), ("detail", C.c_uint32)]


class CryoFetchTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("pages", "not_block_starts", "blocks", "tuples", "bad", "codec_calls", "bytes_back")]


class CryoFilterTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("blocks", "empty_pages", "items", "matches", "bad", "reports", "codec_calls",
                                          "bytes_back")]


class CryoAggCell(C.Structure):
    """cryo_agg_cell (include/cryo_codec.h)"""
    _fields_ = [("n", C.c_uint64), ("min", C.c_int64), ("max", C.c_int64), ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64)]


class CryoAggBlock(C.Structure):
    _fields_ = [("block", C.c_uint32), ("created_xid", C.c_uint32), ("n_items", C.c_uint32), ("n_match", C.c_uint32),
                ("n_bad", C.c_uint32), ("cells", C.POINTER(CryoAggCell))]


class CryoAggTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("blocks", "empty_pages", "items", "matches", "bad", "reports", "codec_calls",
                                          "bytes_back")] + [("cells", CryoAggCell * 4)]


class CryoGroupRec(C.Structure):
    """cryo_group_rec (include/cryo_codec.h)"""
    _fields_ = [("key", C.c_int64 * 2), ("n_rows", C.c_uint32), ("nulls", C.c_uint32)]


class CryoGroupBlock(C.Structure):
    _fields_ = [("block", C.c_uint32), ("created_xid", C.c_uint32), ("n_items", C.c_uint32), ("n_match", C.c_uint32),
                ("n_bad", C.c_uint32), ("n_groups", C.c_uint32), ("recs", C.POINTER(CryoGroupRec)), ("cells", C.POINTER(CryoAggCell))]


class CryoGroupTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("blocks", "empty_pages", "items", "matches", "bad", "reports", "codec_calls",
                                          "bytes_back", "groups")]


class CryoProjectedRow(C.Structure):
    _fields_ = [("block", C.c_uint32), ("pos", C.c_uint16), ("created_xid", C.c_uint32), ("nulls", C.c_uint32),
                ("data", C.c_void_p), ("row_bytes", C.c_uint32)]


class CryoProjectTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("blocks", "empty_pages", "items", "matches", "bad", "reports", "codec_calls",
                                          "bytes_back")]


class CryoTopnBlock(C.Structure):
    _fields_ = [("block", C.c_uint32), ("created_xid", C.c_uint32), ("n_items", C.c_uint32), ("n_match", C.c_uint32),
                ("n_bad", C.c_uint32), ("n_rows", C.c_uint32), ("rec", C.c_void_p), ("rows", C.c_void_p), ("row_bytes", C.c_uint32)]


class CryoTopnTotals(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("blocks", "empty_pages", "items", "matches", "bad", "reports", "codec_calls",
                                          "bytes_back", "rows")]


class CryoTopnMerge(C.Structure):
    """host/topn.h's merge state: by (2 x cryo_order_col), nby, limit, row_bytes, n, rec, rows"""
    _fields_ = [("by", C.c_uint64 * 2), ("nby", C.c_uint32), ("limit", C.c_uint32), ("row_bytes", C.c_uint32), ("n", C.c_uint32),
                ("rec", C.c_void_p), ("rows", C.c_void_p)]


TOPN_BLOCK_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoTopnBlock))
PROJECT_ROW_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoProjectedRow))
AGG_BLOCK_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoAggBlock))
GROUP_BLOCK_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoGroupBlock))
FETCH_TUPLE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoFetchedTuple))
FETCH_REPORT_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(CryoFetchReport))
RECOMPRESS_MOVED_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32)


class HeapTupleData(C.Structure):
    _fields_ = [("t_len", C.c_uint32), ("t_data", C.c_void_p)]


_libs = {}
_production = None   # None: by the environment (CRYO_HOST_TEST_HOOKS=1 selects the test build)


def use(production):
    """Select which build lib() returns from now on: the shipped libcryo_host.so (True), the build with the
    codec-double hook for CPU-only plumbing tests (False), or by the environment (None)."""
    global _production
    _production = production


def lib():
    prod = _production if _production is not None else os.environ.get("CRYO_HOST_TEST_HOOKS") != "1"
    if prod in _libs:
        return _libs[prod]
    _loader.load()  # libcryo_codec.so + one HIP runtime first
    path = HOST_LIB_PATH if prod else HOST_TEST_LIB_PATH
    if not os.path.exists(path):
        raise ImportError("pg_cryogen_amd: %s is missing; build with `make -C pg_cryogen_amd/host`" % path)
    L = C.CDLL(path)
    vp, u32, i32, sz = C.c_void_p, C.c_uint32, C.c_int, C.c_size_t
    L.cryo_compress.argtypes = [i32, vp, C.POINTER(sz)]
    L.cryo_compress.restype = vp
    L.cryo_decompress.argtypes = [i32, vp, sz, vp]
    L.cryo_decompress.restype = C.c_bool
    L.cryo_define_compression_gucs.restype = None
    if hasattr(L, "cryo_host_set_codec_ops"):   # test build only
        L.cryo_host_set_codec_ops.argtypes = [C.POINTER(CryoCodecOps)]
        L.cryo_host_set_codec_ops.restype = None
    if hasattr(L, "cryo_host_set_fetch_ops"):   # test build only
        L.cryo_host_set_fetch_ops.argtypes = [C.POINTER(CryoCodecFetchOps)]
        L.cryo_host_set_fetch_ops.restype = None
    if hasattr(L, "cryo_host_set_filter_ops"):  # test build only
        L.cryo_host_set_filter_ops.argtypes = [C.POINTER(CryoCodecFilterOps)]
        L.cryo_host_set_filter_ops.restype = None
        L.cryo_filter_set_window.argtypes = [i32, sz]
        L.cryo_filter_set_window.restype = None
    if hasattr(L, "cryo_host_set_agg_ops"):     # test build only
        L.cryo_host_set_agg_ops.argtypes = [C.POINTER(CryoCodecAggOps)]
        L.cryo_host_set_agg_ops.restype = None
        L.cryo_aggregate_set_window.argtypes = [i32, sz]
        L.cryo_aggregate_set_window.restype = None
    if hasattr(L, "cryo_host_set_group_ops"):   # test build only
        L.cryo_host_set_group_ops.argtypes = [C.POINTER(CryoCodecGroupOps)]
        L.cryo_host_set_group_ops.restype = None
        L.cryo_group_set_window.argtypes = [i32, sz]
        L.cryo_group_set_window.restype = None
    if hasattr(L, "cryo_host_set_project_ops"):  # test build only
        L.cryo_host_set_project_ops.argtypes = [C.POINTER(CryoCodecProjectOps)]
        L.cryo_host_set_project_ops.restype = None
        L.cryo_project_set_window.argtypes = [i32, sz]
        L.cryo_project_set_window.restype = None
    if hasattr(L, "cryo_host_set_topn_ops"):     # test build only
        L.cryo_host_set_topn_ops.argtypes = [C.POINTER(CryoCodecTopnOps)]
        L.cryo_host_set_topn_ops.restype = None
        L.cryo_topn_set_window.argtypes = [i32, sz]
        L.cryo_topn_set_window.restype = None
    L.cryo_host_codec_error.restype = C.c_char_p
    L.cryo_compat_set_error_handler.argtypes = [ERROR_HANDLER]
    L.cryo_compat_set_error_handler.restype = None
    L.cryo_init_page.argtypes = [vp]
    L.cryo_init_page.restype = None
    L.cryo_storage_insert.argtypes = [vp, C.POINTER(HeapTupleData)]
    L.cryo_storage_fetch.argtypes = [vp, i32, C.POINTER(HeapTupleData)]
    L.cryo_storage_fetch.restype = C.POINTER(HeapTupleData)
    L.cryo_storage_ntuples.argtypes = [vp]
    L.cryo_pages_needed.argtypes = [sz]
    L.cryo_stage_write_chain.argtypes = [C.POINTER(CryoRel), u32, i32, u32, vp, sz, C.POINTER(u32), i32,
                                         C.POINTER(i32)]
    L.cryo_stage_write_batch.argtypes = [C.POINTER(CryoRel), vp, i32, i32, u32, C.POINTER(u32)]
    L.cryo_stage_read_chain.argtypes = [C.POINTER(CryoRel), u32, C.POINTER(vp), C.POINTER(sz), C.POINTER(i32),
                                        C.POINTER(u32), C.POINTER(u32), u32, C.POINTER(u32)]
    L.cryo_memrel_create.restype = vp
    L.cryo_memrel_destroy.argtypes = [vp]
    L.cryo_memrel_destroy.restype = None
    L.cryo_memrel_bind.argtypes = [vp, C.c_uint, C.POINTER(CryoRel)]
    L.cryo_memrel_bind.restype = None
    L.cryo_memrel_reserve.argtypes = [vp]
    L.cryo_memrel_reserve.restype = u32
    L.cryo_memrel_set_frozen.argtypes = [vp, u32, C.c_bool]
    L.cryo_memrel_set_frozen.restype = None
    L.cryo_memrel_page.argtypes = [vp, u32]
    L.cryo_memrel_page.restype = vp
    L.cryo_memrel_nblocks.argtypes = [vp]
    L.cryo_memrel_nblocks.restype = u32
    L.cryo_init_cache.restype = None
    L.cryo_cache_configure.argtypes = [i32]
    L.cryo_cache_shutdown.restype = None
    L.cryo_read_data.argtypes = [C.POINTER(CryoRel), vp, u32, C.POINTER(i32)]
    L.cryo_read_data_batch.argtypes = [C.POINTER(CryoRel), C.POINTER(u32), i32, C.POINTER(i32), C.POINTER(i32)]
    L.cryo_scan_next_batch.argtypes = [C.POINTER(CryoRel), vp, i32, C.POINTER(u32), C.POINTER(i32), C.POINTER(i32)]
    L.cryo_seqscan_iter_create.restype = vp
    L.cryo_seqscan_iter_free.argtypes = [vp]
    L.cryo_seqscan_iter_free.restype = None
    L.cryo_seqscan_iter_next.argtypes = [vp]
    L.cryo_seqscan_iter_next.restype = u32
    L.cryo_seqscan_iter_exclude.argtypes = [vp, u32, C.c_bool]
    L.cryo_seqscan_iter_exclude.restype = C.c_bool
    L.cryo_seqscan_iter_reset.argtypes = [vp]
    L.cryo_seqscan_iter_reset.restype = None
    L.cryo_seqscan_iter_nranges.argtypes = [vp]
    L.cryo_cache_allocate.argtypes = [C.POINTER(CryoRel), u32]
    L.cryo_cache_release.argtypes = [i32]
    L.cryo_cache_release.restype = None
    L.cryo_cache_invalidate_relation.argtypes = [C.c_uint]
    L.cryo_cache_invalidate_relation.restype = None
    L.cryo_cache_get_pg_nblocks.argtypes = [i32]
    L.cryo_cache_get_pg_nblocks.restype = u32
    L.cryo_cache_get_data.argtypes = [i32]
    L.cryo_cache_get_data.restype = vp
    L.cryo_cache_get_xid.argtypes = [i32]
    L.cryo_cache_get_xid.restype = u32
    L.cryo_cache_err.argtypes = [i32]
    L.cryo_cache_err.restype = C.c_char_p
    L.cryo_host_transfer_counters.argtypes = [C.POINTER(C.c_uint64)] * 4
    L.cryo_host_transfer_counters.restype = None
    L.cryo_check_relation.argtypes = [C.POINTER(CryoRel), CHECK_REPORT_FN, vp, C.POINTER(CryoCheckTotals)]
    L.cryo_recompress_relation.argtypes = [C.POINTER(CryoRel), C.POINTER(CryoRel), i32, i32, RECOMPRESS_MOVED_FN, CHECK_REPORT_FN,
                                           vp, C.POINTER(CryoRecompressTotals)]
    L.cryo_fetch_tuples.argtypes = [C.POINTER(CryoRel), C.POINTER(CryoFetchPage), sz, FETCH_TUPLE_FN, FETCH_REPORT_FN, vp,
                                    C.POINTER(CryoFetchTotals)]
    # CryoFilteredTuple and CryoFilterReport have the layouts of the fetch's CryoFetchedTuple and CryoFetchReport
    L.cryo_filter_scan.argtypes = [C.POINTER(CryoRel), vp, FETCH_TUPLE_FN, FETCH_REPORT_FN, vp, C.POINTER(CryoFilterTotals)]
    # CryoAggReport has the layout of the fetch's CryoFetchReport
    L.cryo_aggregate_scan.argtypes = [C.POINTER(CryoRel), vp, vp, AGG_BLOCK_FN, FETCH_REPORT_FN, vp, C.POINTER(CryoAggTotals)]
    # CryoGroupReport has the layout of the fetch's CryoFetchReport
    L.cryo_group_scan.argtypes = [C.POINTER(CryoRel), vp, vp, vp, GROUP_BLOCK_FN, FETCH_REPORT_FN, vp, C.POINTER(CryoGroupTotals)]
    # CryoProjectReport has the layout of the fetch's CryoFetchReport
    L.cryo_project_scan.argtypes = [C.POINTER(CryoRel), vp, vp, PROJECT_ROW_FN, FETCH_REPORT_FN, vp, C.POINTER(CryoProjectTotals)]
    L.cryo_topn_scan.argtypes = [C.POINTER(CryoRel), vp, vp, vp, TOPN_BLOCK_FN, FETCH_REPORT_FN, vp, C.POINTER(CryoTopnTotals)]
    L.cryo_topn_merge_init.argtypes = [C.POINTER(CryoTopnMerge), vp, C.c_uint32, C.c_uint32]
    L.cryo_topn_merge_add.argtypes = [C.POINTER(CryoTopnMerge), vp, vp, C.c_uint32]
    L.cryo_topn_merge_finish.argtypes = [C.POINTER(CryoTopnMerge), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.cryo_topn_merge_finish.restype = C.c_uint32
    L.cryo_topn_merge_free.argtypes = [C.POINTER(CryoTopnMerge)]
    L.cryo_topn_merge_free.restype = None
    for n in ("cryo_cache_hits", "cryo_cache_misses", "cryo_cache_codec_calls"):
        getattr(L, n).restype = C.c_uint64
    _libs[prod] = L
    return L


class CheckRelationError(RuntimeError):
    def __init__(self, code):
        self.code = code
        super().__init__("cryo_check_relation failed: %d" % code)


def check_relation(rel):
    """cryo_check_relation (host/check.h): (reports, totals) -- reports a list of (block, reason, offset, npages) in ascending
    block order, totals a dict of blocks, empty_pages, bad, codec_calls.  A nonzero status raises CheckRelationError."""
    reports = []
    cb = CHECK_REPORT_FN(lambda arg, r: reports.append((r.contents.block, r.contents.reason, r.contents.offset,
                                                        r.contents.npages)))
    t = CryoCheckTotals()
    rc = lib().cryo_check_relation(C.byref(rel), cb, None, C.byref(t))
    if rc != 0:
        raise CheckRelationError(rc)
    return reports, {f: getattr(t, f) for f, _ in CryoCheckTotals._fields_}


class RecompressRelationError(RuntimeError):
    def __init__(self, code):
        self.code = code
        super().__init__("cryo_recompress_relation failed: %d" % code)


def recompress_relation(src, dst, method, param):
    """cryo_recompress_relation (host/recompress.h): (moved, reports, totals) -- moved a list of (old_first, new_first,
    old_npages, new_npages) in the order written, reports a list of (block, reason, offset, npages) in walk order, totals a
    dict.  A nonzero status raises RecompressRelationError."""
    moved, reports = [], []
    mcb = RECOMPRESS_MOVED_FN(lambda arg, a, b, c, d: moved.append((a, b, c, d)))
    rcb = CHECK_REPORT_FN(lambda arg, r: reports.append((r.contents.block, r.contents.reason, r.contents.offset,
                                                         r.contents.npages)))
    t = CryoRecompressTotals()
    rc = lib().cryo_recompress_relation(C.byref(src), C.byref(dst), method, param, mcb, rcb, None, C.byref(t))
    if rc != 0:
        raise RecompressRelationError(rc)
    return moved, reports, {f: getattr(t, f) for f, _ in CryoRecompressTotals._fields_}


class FetchTuplesError(RuntimeError):
    def __init__(self, code, events, totals):
        self.code, self.events, self.totals = code, events, totals
        super().__init__("cryo_fetch_tuples failed: %d" % code)


def fetch_tuples(rel, pages):
    """cryo_fetch_tuples (host/fetch.h).  pages: a list of (block, positions) in ascending block order, positions a list of
    1-based item positions or None for a lossy page.  Returns (events, totals): events in delivery order, ("tuple", block, pos,
    created_xid, bytes of MAXALIGN(len), len) or ("report", block, reason, detail); totals a dict.  A nonzero status raises
    FetchTuplesError (which carries what was delivered)."""
    keep = [None if p is None else (C.c_uint16 * max(len(p), 1))(*p) for _, p in pages]
    arr = (CryoFetchPage * max(len(pages), 1))()
    for i, (b, p) in enumerate(pages):
        arr[i].block = b
        arr[i].ntuples = -1 if p is None else len(p)
        arr[i].offsets = None if p is None else C.cast(keep[i], C.POINTER(C.c_uint16))
    events = []

    def on_tuple(arg, t):
        t = t.contents
        events.append(("tuple", t.block, t.pos, t.created_xid, C.string_at(t.data, (t.len + 7) & ~7), t.len))

    tcb = FETCH_TUPLE_FN(on_tuple)
    rcb = FETCH_REPORT_FN(lambda arg, r: events.append(("report", r.contents.block, r.contents.reason, r.contents.detail)))
    t = CryoFetchTotals()
    rc = lib().cryo_fetch_tuples(C.byref(rel), arr, len(pages), tcb, rcb, None, C.byref(t))
    totals = {f: getattr(t, f) for f, _ in CryoFetchTotals._fields_}
    if rc != 0:
        raise FetchTuplesError(rc, events, totals)
    return events, totals


class FilterScanError(RuntimeError):
    def __init__(self, code, events, totals):
        self.code, self.events, self.totals = code, events, totals
        super().__init__("cryo_filter_scan failed: %d" % code)


def filter_scan(rel, atts, keys=(), flags=0, truth=None):
    """cryo_filter_scan (host/filter.h) with the descriptor codec.filter_desc makes of atts [(attlen, attalign)], keys [(att,
    type, op, value)], flags and truth (a truth table over the keys, codec.truth_dnf).  Returns (events, totals): events in delivery order, ("tuple", block, pos, created_xid, bytes of
    MAXALIGN(len), len) or ("report", block, reason, detail); totals a dict.  A nonzero status raises FilterScanError (which
    carries what was delivered)."""
    from . import codec
    desc = codec.filter_desc(atts, keys, flags, truth)
    events = []

    def on_tuple(arg, t):
        t = t.contents
        events.append(("tuple", t.block, t.pos, t.created_xid, C.string_at(t.data, (t.len + 7) & ~7), t.len))

    tcb = FETCH_TUPLE_FN(on_tuple)
    rcb = FETCH_REPORT_FN(lambda arg, r: events.append(("report", r.contents.block, r.contents.reason, r.contents.detail)))
    t = CryoFilterTotals()
    rc = lib().cryo_filter_scan(C.byref(rel), C.byref(desc[0]), tcb, rcb, None, C.byref(t))
    totals = {f: getattr(t, f) for f, _ in CryoFilterTotals._fields_}
    if rc != 0:
        raise FilterScanError(rc, events, totals)
    return events, totals


class AggregateScanError(RuntimeError):
    def __init__(self, code, events, totals):
        self.code, self.events, self.totals = code, events, totals
        super().__init__("cryo_aggregate_scan failed: %d" % code)


def _cell(c):
    """(n, min, max, sum) of a CryoAggCell, the sum as a Python integer"""
    return (c.n, c.min, c.max, (c.sum_hi << 64) + c.sum_lo)


def aggregate_scan(rel, atts, keys, cols, truth=None):
    """cryo_aggregate_scan (host/aggregate.h) with the descriptors codec.filter_desc and codec.agg_desc make of atts [(attlen,
    attalign)], keys [(att, type, op, value)] and cols [(att, type)].  Returns (events, totals): events in delivery order,
    ("block", block, created_xid, n_items, n_match, n_bad, [(n, min, max, sum) per column]) or ("report", block, reason, detail);
    totals a dict whose "cells" are the combined [(n, min, max, sum) per column].  A nonzero status raises AggregateScanError
    (which carries what was delivered)."""
    from . import codec
    desc, adesc = codec.filter_desc(atts, keys, 0, truth), codec.agg_desc(cols)
    ncols = len(cols)
    events = []

    def on_block(arg, b):
        b = b.contents
        events.append(("block", b.block, b.created_xid, b.n_items, b.n_match, b.n_bad, [_cell(b.cells[j]) for j in range(ncols)]))

    bcb = AGG_BLOCK_FN(on_block)
    rcb = FETCH_REPORT_FN(lambda arg, r: events.append(("report", r.contents.block, r.contents.reason, r.contents.detail)))
    t = CryoAggTotals()
    rc = lib().cryo_aggregate_scan(C.byref(rel), C.byref(desc[0]), C.byref(adesc[0]), bcb, rcb, None, C.byref(t))
    totals = {f: getattr(t, f) for f, _ in CryoAggTotals._fields_ if f != "cells"}
    totals["cells"] = [_cell(t.cells[j]) for j in range(min(ncols, 4))]
    if rc != 0:
        raise AggregateScanError(rc, events, totals)
    return events, totals


class GroupScanError(RuntimeError):
    def __init__(self, code, events, totals):
        self.code, self.events, self.totals = code, events, totals
        super().__init__("cryo_group_scan failed: %d" % code)


def group_scan(rel, atts, keys, by, cols=None, truth=None, buckets=None, text=False):
    """cryo_group_scan (host/group.h) with the descriptors codec.filter_desc, codec.group_desc and codec.agg_desc make of atts
    [(attlen, attalign)], keys [(att, type, op, value)], by and cols [(att, type)] (cols None: a null aggregate descriptor);
    buckets: one (kind, flags, origin, value) per group column, as for codec.group_desc.  text: the descriptor carries
    codec.GROUP_TEXT, a group column may be (att, codec.KEY_BYTES), and such a column's place in a key tuple holds the value's
    bytes, taken from the group's key cell.
    Returns (events, totals): events in delivery order, ("block", block, created_xid, n_items, n_match, n_bad, [(key tuple with
    None for NULL, n_rows, [(n, min, max, sum) per column]) per group]) or ("report", block, reason, detail); totals a dict.  A
    nonzero status raises GroupScanError (which carries what was delivered)."""
    from . import codec
    desc, gdesc = codec.filter_desc(atts, keys, 0, truth), codec.group_desc(by, buckets, text)
    adesc = None if cols is None else codec.agg_desc(cols)
    nby, ncols = len(by), len(cols or ())
    texts = [j for j, (_, typ) in enumerate(by) if typ == codec.KEY_BYTES] if text else []
    cpg = ncols + len(texts)                      # a group's cells: the aggregate cells, then a key cell per text column
    events = []

    def key_bytes(b, g, t):
        raw = C.string_at(C.addressof(b.cells[g * cpg + ncols + t]), 40)
        return raw[:int.from_bytes(raw[32:36], "little")]

    def on_block(arg, b):
        b = b.contents
        groups = []
        for g in range(b.n_groups):
            r = b.recs[g]
            key = tuple(None if (r.nulls >> j) & 1 else key_bytes(b, g, texts.index(j)) if j in texts else r.key[j]
                        for j in range(min(nby, 2)))
            groups.append((key, r.n_rows, [_cell(b.cells[g * cpg + j]) for j in range(ncols)]))
        events.append(("block", b.block, b.created_xid, b.n_items, b.n_match, b.n_bad, groups))

    bcb = GROUP_BLOCK_FN(on_block)
    rcb = FETCH_REPORT_FN(lambda arg, r: events.append(("report", r.contents.block, r.contents.reason, r.contents.detail)))
    t = CryoGroupTotals()
    rc = lib().cryo_group_scan(C.byref(rel), C.byref(desc[0]), C.byref(gdesc[0]), C.byref(adesc[0]) if adesc else None, bcb, rcb,
                               None, C.byref(t))
    totals = {f: getattr(t, f) for f, _ in CryoGroupTotals._fields_}
    if rc != 0:
        raise GroupScanError(rc, events, totals)
    return events, totals


class ProjectScanError(RuntimeError):
    def __init__(self, code, events, totals):
        self.code, self.events, self.totals = code, events, totals
        super().__init__("cryo_project_scan failed: %d" % code)


def project_scan(rel, atts, keys, cols, truth=None):
    """cryo_project_scan (host/project.h) with the descriptors codec.filter_desc and codec.project_desc make of atts [(attlen,
    attalign)], keys [(att, type, op, value)] and cols [att].  Returns (events, totals): events in delivery order, ("row", block,
    pos, created_xid, nulls, the row's bytes) or ("report", block, reason, detail); totals a dict.  A nonzero status raises
    ProjectScanError (which carries what was delivered)."""
    from . import codec
    desc, pdesc = codec.filter_desc(atts, keys, 0, truth), codec.project_desc(cols)
    events = []

    def on_row(arg, r):
        r = r.contents
        events.append(("row", r.block, r.pos, r.created_xid, r.nulls, C.string_at(r.data, r.row_bytes)))

    wcb = PROJECT_ROW_FN(on_row)
    rcb = FETCH_REPORT_FN(lambda arg, r: events.append(("report", r.contents.block, r.contents.reason, r.contents.detail)))
    t = CryoProjectTotals()
    rc = lib().cryo_project_scan(C.byref(rel), C.byref(desc[0]), C.byref(pdesc[0]), wcb, rcb, None, C.byref(t))
    totals = {f: getattr(t, f) for f, _ in CryoProjectTotals._fields_}
    if rc != 0:
        raise ProjectScanError(rc, events, totals)
    return events, totals


class TopnScanError(RuntimeError):
    def __init__(self, code, events, totals):
        self.code, self.events, self.totals = code, events, totals
        super().__init__("cryo_topn_scan failed: %d" % code)


def topn_scan(rel, atts, keys, by, limit, cols, truth=None):
    """cryo_topn_scan (host/topn.h) with the descriptors codec.filter_desc, codec.order_desc and codec.project_desc make of atts
    [(attlen, attalign)], keys [(att, type, op, value)], by [(att, type, flags)] and cols [att].  Returns (events, totals): events
    in delivery order, ("block", block, created_xid, (n_items, n_match, n_bad), records: a TOPN_REC array, rows: a uint8 array of
    shape (n_rows, row_bytes)) or ("report", block, reason, detail); totals a dict.  A nonzero status raises TopnScanError (which
    carries what was delivered)."""
    import numpy as np
    from . import codec
    desc, odesc, pdesc = codec.filter_desc(atts, keys, 0, truth), codec.order_desc(by, limit), codec.project_desc(cols)
    events = []

    def on_block(arg, b):
        b = b.contents
        recs = np.frombuffer(C.string_at(b.rec, 24 * b.n_rows), codec.TOPN_REC).copy() if b.n_rows else np.zeros(0, codec.TOPN_REC)
        rows = np.frombuffer(C.string_at(b.rows, b.row_bytes * b.n_rows), np.uint8).reshape(b.n_rows, b.row_bytes).copy() \
            if b.n_rows else np.zeros((0, b.row_bytes), np.uint8)
        events.append(("block", b.block, b.created_xid, (b.n_items, b.n_match, b.n_bad), recs, rows))

    bcb = TOPN_BLOCK_FN(on_block)
    rcb = FETCH_REPORT_FN(lambda arg, r: events.append(("report", r.contents.block, r.contents.reason, r.contents.detail)))
    t = CryoTopnTotals()
    rc = lib().cryo_topn_scan(C.byref(rel), C.byref(desc[0]), C.byref(odesc[0]), C.byref(pdesc[0]), bcb, rcb, None, C.byref(t))
    totals = {f: getattr(t, f) for f, _ in CryoTopnTotals._fields_}
    if rc != 0:
        raise TopnScanError(rc, events, totals)
    return events, totals


def topn_merge(by, limit, blocks):
    """host/topn.h's merge (cryo_topn_merge_init / _add / _finish / _free) over blocks, a sequence of (TOPN_REC array, rows of
    shape (n, row_bytes)) in the order they are added: (records, rows) of the first `limit` rows"""
    import numpy as np
    from . import codec
    L = lib()
    row_bytes = next((np.asarray(rows).shape[1] for _, rows in blocks if len(rows)), 8)
    odesc = codec.order_desc(by, limit)
    m = CryoTopnMerge()
    rc = L.cryo_topn_merge_init(C.byref(m), C.byref(odesc[0]), limit, row_bytes)
    if rc != 0:
        raise RuntimeError("cryo_topn_merge_init failed: %d" % rc)
    try:
        for recs, rows in blocks:
            recs, rows = np.ascontiguousarray(recs, codec.TOPN_REC), np.ascontiguousarray(rows, np.uint8)
            rc = L.cryo_topn_merge_add(C.byref(m), recs.ctypes.data if len(recs) else None, rows.ctypes.data if len(recs) else None, len(recs))
            if rc != 0:
                raise RuntimeError("cryo_topn_merge_add failed: %d" % rc)
        rp, wp = C.c_void_p(), C.c_void_p()
        n = L.cryo_topn_merge_finish(C.byref(m), C.byref(rp), C.byref(wp))
        out_rec = np.frombuffer(C.string_at(rp, 24 * n), codec.TOPN_REC).copy() if n else np.zeros(0, codec.TOPN_REC)
        out_rows = np.frombuffer(C.string_at(wp, row_bytes * n), np.uint8).reshape(n, row_bytes).copy() if n else np.zeros((0, row_bytes), np.uint8)
        return out_rec, out_rows
    finally:
        L.cryo_topn_merge_free(C.byref(m))


def transfer_counters():
    """(h2d_bytes, d2h_bytes, pool_hits, pool_misses) of the bound GPU codec"""
    v = [C.c_uint64() for _ in range(4)]
    lib().cryo_host_transfer_counters(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def set_int(name, value):
    C.c_int.in_dll(lib(), name).value = value


def get_int(name):
    return C.c_int.in_dll(lib(), name).value


def set_block_size(n):
    C.c_size_t.in_dll(lib(), "cryo_blcksz").value = n


def get_block_size():
    return C.c_size_t.in_dll(lib(), "cryo_blcksz").value
