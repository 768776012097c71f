"""ctypes binding of the C ABI in include/cryo_codec.h.

This module is the test/bench driver's view of the library: it adds nothing to
the codec, it only marshals numpy arrays and device pointers.  Names follow the
reference's domain (cryo blocks, methods, acceleration/level), see
reference compression.h:7-24.
"""
import ctypes as C
import struct

import numpy as np

from . import _loader

METHOD_LZ4 = 0   # COMP_LZ4, reference compression.h:9
METHOD_ZSTD = 1  # COMP_ZSTD, reference compression.h:10

OK = 0
E_ARG, E_HIP, E_NODEV, E_CORRUPT, E_DSTSIZE, E_UNSUPPORTED, E_NOMEM, E_VERIFY = -1, -2, -3, -4, -5, -6, -7, -8
_ERR_NAMES = {0: "CRYO_OK", -1: "CRYO_E_ARG", -2: "CRYO_E_HIP", -3: "CRYO_E_NODEV",
              -4: "CRYO_E_CORRUPT", -5: "CRYO_E_DSTSIZE", -6: "CRYO_E_UNSUPPORTED",
              -7: "CRYO_E_NOMEM", -8: "CRYO_E_VERIFY"}

# cryo_option (include/cryo_codec.h)
OPT_LZ4_DECODE_PATH, OPT_LZ4_INDEX_WALKERS, OPT_PIPE_MIN_BYTES, OPT_POOL_BYTES, OPT_ZSTD_DECODE_PATH = 1, 2, 3, 4, 5
OPT_LZ4_DECODE_WAVES = 9
OPT_WORKSPACE_KEEP_BYTES, OPT_WORKSPACE_MAX_BYTES, OPT_NUMA_LOCAL = 6, 7, 8
OPT_ENCODE_SEGMENT_BYTES = 10  # 0 = byte-identical encoders; 4 KiB .. 128 KiB (power of two) = segment-parallel encode
OPT_ENCODE_SEGMENT_ZSTD_STRATEGY = 11  # highest zstd strategy of segment mode: 1 fast (default) .. 6 btlazy2
OPT_ENCODE_VERIFY = 12  # 0 (default) = none; 1 = every compress call decodes its output and compares it with the input
OPT_ZSTD_CHECKSUM = 13  # 0 (default) = none; 1 = every zstd frame written carries a content checksum (XXH64)
OPT_LZ4_INDEX_FORM = 14  # one-walker index pass: 0 automatic, 1 one wave walks and feeds, 2 a walker wave and a feeder wave
LZ4_INDEX_AUTO, LZ4_INDEX_SINGLE, LZ4_INDEX_PAIR = 0, 1, 2
VERIFY_NONE = 0xFFFFFFFF  # first-mismatch offset of a block that verified (or whose stream the decoders reject)
# cryo_check_reason (include/cryo_codec.h): the verdict of the stored-block check, with the offset it reports
CHECK_OK, CHECK_STREAM, CHECK_HEADER, CHECK_ITEM, CHECK_NONZERO = 0, 1, 2, 3, 4
CHECK_NONE = 0xFFFFFFFF  # offset of CHECK_OK and CHECK_STREAM
# cryo_fetch_status (include/cryo_codec.h): the verdict on one requested tuple; 1 .. 3 equal CHECK_*'s, 4 is unused
FETCH_OK, FETCH_STREAM, FETCH_HEADER, FETCH_ITEM, FETCH_NOITEM, FETCH_BADREQ, FETCH_OVERLAP = 0, 1, 2, 3, 5, 6, 7
# cryo_fetch_result, 16 bytes per request
FETCH_RESULT = np.dtype([("status", "<u4"), ("len", "<u4"), ("off", "<u8")])
# the scan filter (include/cryo_codec.h): a record's statuses are 0, FETCH_ITEM and FILTER_TUPLE, a block's 0, FETCH_STREAM,
# FETCH_HEADER and FETCH_OVERLAP
FILTER_TUPLE = 8
FILTER_UNDECIDED = 9        # a record's status: a byte-string key met a compressed or external value
FILTER_COUNT_ONLY = 1
FILTER_MAX_KEYS = 4
FILTER_TRUTH = 4            # the descriptor's rsv is a truth table over its keys (truth_dnf), not reserved
KEY_INT2, KEY_INT4, KEY_INT8 = 1, 2, 3
KEY_FLOAT4, KEY_FLOAT8 = 8, 9   # float4 / float8 columns: a comparison key's value is a Python float (or the bits of a double)
KEY_BYTES = 16              # a byte string: the key's value is bytes, compared unsigned, then by length
KEY_BYTES_MAX = 256
OP_LT, OP_LE, OP_EQ, OP_GE, OP_GT, OP_NE, OP_ISNULL, OP_NOTNULL = range(1, 9)
OP_IN, OP_NOT_IN = 9, 10    # a set key: the key's value is a sequence of ints, its type KEY_INT2 / KEY_INT4 / KEY_INT8
KEY_SET_MAX = 1024
OP_LIKE, OP_NOT_LIKE = 11, 12   # a pattern key: type KEY_BYTES, the key's value a like(...) object
LIKE_UTF8 = 0x10000         # bit 16 of a pattern key's rsv: a character is a byte and the bytes 10xxxxxx behind it
LIKE_TEXT_MAX = 2048        # the longest payload a pattern key is matched against; a longer one is undecided
FILTER_ATT = np.dtype([("attlen", "<i2"), ("attalign", "u1"), ("rsv", "u1")])                                  # cryo_att
FILTER_KEY = np.dtype([("att", "<u2"), ("type", "u1"), ("op", "u1"), ("rsv", "<u4"), ("value", "<i8")])        # cryo_scan_key
FILTER_BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"),
                         ("rec_first", "<u8"), ("off", "<u8")])                                                # cryo_filter_block
FILTER_REC = np.dtype([("pos", "<u2"), ("status", "<u2"), ("len", "<u4")])                                     # cryo_filter_rec
# the scan aggregate (include/cryo_codec.h): a block's statuses are 0, FETCH_STREAM and FETCH_HEADER
AGG_MAX_COLS = 4
AGG_COL = np.dtype([("att", "<u2"), ("type", "u1"), ("rsv", "u1"), ("rsv2", "<u4")])                            # cryo_agg_col
AGG_BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4")])             # cryo_agg_block
AGG_CELL = np.dtype([("n", "<u8"), ("min", "<i8"), ("max", "<i8"), ("sum_lo", "<u8"), ("sum_hi", "<i8")])       # cryo_agg_cell
AGG_CELL_F = np.dtype([("n", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sum", "<f8"), ("err", "<f8")])               # cryo_agg_cell_f
# the grouped scan (include/cryo_codec.h): a block's statuses are the aggregate's; cells are AGG_CELL, one per group and column
GROUP_MAX_BY = 2
GROUP_BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"),
                        ("n_groups", "<u4"), ("rsv", "<u4"), ("first_group", "<u8")])                             # cryo_group_block
GROUP_REC = np.dtype([("key", "<i8", (2,)), ("n_rows", "<u4"), ("nulls", "<u4")])                                # cryo_group_rec
# bucketed group columns: a bucket is (kind, flags, origin, value); the value of a BUCKET_BOUNDS bucket is a sequence of ints
GROUP_BUCKETS = 1           # cryo_group.rsv: the struct is a cryo_group_b
BUCKET_NONE, BUCKET_WIDTH, BUCKET_BOUNDS = 0, 1, 2
BUCKET_INFINITE = 1         # a bucket's flag: the column type's extremes are -infinity and +infinity, each its own bucket
BUCKET_BOUNDS_MAX = 1024
# text group columns: group columns may be KEY_BYTES; a group then has a GROUP_KEY cell per such column behind its AGG_CELLs
GROUP_TEXT = 4              # cryo_group.rsv
GROUP_TEXT_MAX = 32         # the longest payload that is a key
GROUP_KEY = np.dtype([("bytes", "u1", (32,)), ("len", "<u4"), ("rsv", "<u4")])                                   # cryo_group_key
BUCKET = np.dtype([("kind", "u1"), ("flags", "u1"), ("rsv", "<u2"), ("n", "<u4"), ("origin", "<i8"), ("value", "<i8")])  # cryo_bucket
# the projecting scan (include/cryo_codec.h): a block's statuses are the aggregate's, a record's the filter's
PROJECT_MAX_COLS = 8
PROJECT_COL = np.dtype([("att", "<u2"), ("rsv", "<u2"), ("rsv2", "<u4")])                                       # cryo_project_col
PROJECT_BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"),
                          ("rec_first", "<u8"), ("row_first", "<u8")])                                          # cryo_project_block
PROJECT_REC = np.dtype([("pos", "<u2"), ("status", "<u2"), ("nulls", "<u4")])                                   # cryo_project_rec
# the ordered scan (include/cryo_codec.h): a block's statuses are the aggregate's; rows are the projection's
ORDER_DESC, ORDER_NULLS_FIRST = 1, 2    # cryo_order_col.flags
ORDER_MAX_BY = 2
ORDER_COL = np.dtype([("att", "<u2"), ("type", "u1"), ("flags", "u1"), ("rsv", "<u4")])                          # cryo_order_col
TOPN_BLOCK = np.dtype([("status", "<u4"), ("n_items", "<u4"), ("n_match", "<u4"), ("n_bad", "<u4"),
                       ("n_rows", "<u4"), ("rsv", "<u4"), ("row_first", "<u8")])                                 # cryo_topn_block
TOPN_REC = np.dtype([("key", "<i8", (2,)), ("pos", "<u2"), ("key_nulls", "<u2"), ("nulls", "<u4")])              # cryo_topn_rec
LZ4_PATH_AUTO, LZ4_PATH_RING, LZ4_PATH_INDEXED, LZ4_PATH_FEW_BLOCKS = 0, 1, 2, 3

DIST_WIDE, DIST_NARROW, DIST_INT4, DIST_RANDOM, DIST_ZEROS = range(5)
DIST_NAMES = ["wide", "narrow", "int4", "random", "zeros"]

# every symbol include/cryo_codec.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "cryo_codec_version", "cryo_codec_device_count", "cryo_codec_open", "cryo_codec_close",
    "cryo_codec_last_error", "cryo_codec_stream", "cryo_codec_sync", "cryo_codec_bound",
    "cryo_codec_set_option", "cryo_codec_get_option",
    "cryo_dev_alloc", "cryo_dev_free", "cryo_dev_upload", "cryo_dev_download", "cryo_dev_memset",
    "cryo_codec_compress_batch", "cryo_codec_decompress_batch", "cryo_codec_compress_block",
    "cryo_codec_decompress_block", "cryo_codec_compress_blocks", "cryo_codec_decompress_blocks",
    "cryo_codec_decompress_blocks_to",
    "cryo_multi_open", "cryo_multi_close", "cryo_multi_count", "cryo_multi_last_error",
    "cryo_multi_compress_blocks", "cryo_multi_decompress_blocks", "cryo_multi_decompress_blocks_to",
    "cryo_multi_decompress_blocks_keyed", "cryo_multi_set_option", "cryo_multi_pool_invalidate",
    "cryo_multi_get_transfer_counters",
    "cryo_codec_decompress_blocks_keyed", "cryo_codec_pool_invalidate", "cryo_codec_get_transfer_counters",
    "cryo_codec_trim", "cryo_multi_trim",
    "cryo_codec_synth_batch", "cryo_codec_checksum_batch",
    "cryo_codec_compare_batch", "cryo_checksum64", "cryo_codec_timer_start",
    "cryo_codec_timer_stop", "cryo_codec_get_counters",
    "cryo_codec_verify_batch", "cryo_codec_last_verify_failure", "cryo_multi_last_verify_failure",
    "cryo_codec_check_batch", "cryo_codec_check_blocks", "cryo_multi_check_blocks",
    "cryo_codec_recode_batch", "cryo_codec_recode_blocks", "cryo_multi_recode_blocks",
    "cryo_codec_fetch_batch", "cryo_codec_fetch_blocks", "cryo_multi_fetch_blocks",
    "cryo_codec_filter_batch", "cryo_codec_filter_blocks", "cryo_multi_filter_blocks",
    "cryo_codec_agg_batch", "cryo_codec_agg_blocks", "cryo_multi_agg_blocks",
    "cryo_codec_group_batch", "cryo_codec_group_blocks", "cryo_multi_group_blocks",
    "cryo_codec_project_batch", "cryo_codec_project_blocks", "cryo_multi_project_blocks",
    "cryo_codec_topn_batch", "cryo_codec_topn_blocks", "cryo_multi_topn_blocks",
    "cryo_codec_lz4_index_cap", "cryo_codec_lz4_index_rows", "cryo_codec_debug_fill",
]


class CryoError(RuntimeError):
    def __init__(self, code, what="", detail=""):
        self.code = code
        super().__init__("%s failed: %s (%d) %s" % (what, _ERR_NAMES.get(code, "?"), code, detail))


class CryoFilter(C.Structure):
    """cryo_filter: atts / keys point to device arrays for filter_batch, to host arrays for filter_blocks"""
    _fields_ = [("natts", C.c_uint32), ("nkeys", C.c_uint32), ("flags", C.c_uint32), ("rsv", C.c_uint32),
                ("atts", C.c_void_p), ("keys", C.c_void_p)]


class CryoAgg(C.Structure):
    """cryo_agg: cols points to a device array for agg_batch, to a host array for agg_blocks"""
    _fields_ = [("ncols", C.c_uint32), ("rsv", C.c_uint32), ("cols", C.c_void_p)]


class CryoGroup(C.Structure):
    """cryo_group: by points to a device array for group_batch, to a host array for group_blocks"""
    _fields_ = [("nby", C.c_uint32), ("rsv", C.c_uint32), ("by", C.c_void_p)]


class CryoGroupB(CryoGroup):
    """cryo_group_b: cryo_group with rsv = GROUP_BUCKETS and, behind by, the buckets array (device / host memory as by is)"""
    _fields_ = [("buckets", C.c_void_p)]


class CryoProject(C.Structure):
    """cryo_project: cols points to a device array for project_batch, to a host array for project_blocks"""
    _fields_ = [("ncols", C.c_uint32), ("rsv", C.c_uint32), ("cols", C.c_void_p)]


class CryoOrder(C.Structure):
    """cryo_order: by points to a device array for topn_batch, to a host array for topn_blocks"""
    _fields_ = [("nby", C.c_uint32), ("limit", C.c_uint32), ("by", C.c_void_p)]


class TransferCounters(C.Structure):
    _fields_ = [("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64), ("pool_hits", C.c_uint64),
                ("pool_misses", C.c_uint64), ("pool_blocks", C.c_uint64), ("pool_capacity", C.c_uint64)]


class FillReport(C.Structure):
    """cryo_codec_fill_report: the bytes cryo_codec_debug_fill filled per handle-owned buffer"""
    _fields_ = [("d_ws", C.c_uint64), ("d_vfy", C.c_uint64), ("d_rec", C.c_uint64), ("hb_src", C.c_uint64),
                ("hb_dst", C.c_uint64), ("hb_meta", C.c_uint64), ("d_in", C.c_uint64), ("d_out", C.c_uint64),
                ("d_scalars", C.c_uint64), ("d_keytab", C.c_uint64), ("pin", C.c_uint64), ("pipe_pin", C.c_uint64 * 4)]


class Counters(C.Structure):
    _fields_ = [("blocks_compressed", C.c_uint64), ("blocks_decompressed", C.c_uint64),
                ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("launches", C.c_uint64)]


_bound = False


def lib():
    """The loaded library with argtypes/restypes set."""
    global _bound
    L = _loader.load()
    if _bound:
        return L
    vp, u64, u32, i32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_size_t
    L.cryo_codec_version.restype = C.c_char_p
    L.cryo_codec_device_count.restype = i32
    L.cryo_codec_open.argtypes = [i32, C.POINTER(vp)]
    L.cryo_codec_close.argtypes = [vp]
    L.cryo_codec_close.restype = None
    L.cryo_codec_last_error.argtypes = [vp]
    L.cryo_codec_last_error.restype = C.c_char_p
    L.cryo_codec_stream.argtypes = [vp]
    L.cryo_codec_stream.restype = vp
    L.cryo_codec_sync.argtypes = [vp]
    L.cryo_codec_set_option.argtypes = [vp, i32, C.c_int64]
    L.cryo_codec_get_option.argtypes = [vp, i32, C.POINTER(C.c_int64)]
    L.cryo_codec_bound.argtypes = [i32, sz]
    L.cryo_codec_bound.restype = sz
    L.cryo_dev_alloc.argtypes = [vp, sz, C.POINTER(vp)]
    L.cryo_dev_free.argtypes = [vp, vp]
    L.cryo_dev_upload.argtypes = [vp, vp, vp, sz]
    L.cryo_dev_download.argtypes = [vp, vp, vp, sz]
    L.cryo_dev_memset.argtypes = [vp, vp, i32, sz]
    L.cryo_codec_compress_batch.argtypes = [vp, i32, i32, vp, u64, u32, u64, vp, u64, vp, vp]
    L.cryo_codec_decompress_batch.argtypes = [vp, i32, vp, vp, vp, vp, u64, u32, u64, vp]
    L.cryo_codec_compress_block.argtypes = [vp, i32, i32, vp, sz, vp, sz, C.POINTER(sz)]
    L.cryo_codec_decompress_block.argtypes = [vp, i32, vp, sz, vp, sz]
    L.cryo_codec_compress_blocks.argtypes = [vp, i32, i32, vp, sz, sz, vp, sz, vp]
    L.cryo_codec_decompress_blocks.argtypes = [vp, i32, vp, vp, sz, vp, sz, vp]
    L.cryo_codec_decompress_blocks_to.argtypes = [vp, i32, vp, vp, sz, vp, sz, vp]
    L.cryo_multi_open.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    L.cryo_multi_close.argtypes = [vp]
    L.cryo_multi_close.restype = None
    L.cryo_multi_count.argtypes = [vp]
    L.cryo_multi_last_error.argtypes = [vp]
    L.cryo_multi_last_error.restype = C.c_char_p
    L.cryo_multi_compress_blocks.argtypes = [vp, i32, i32, vp, sz, sz, vp, sz, vp]
    L.cryo_multi_decompress_blocks.argtypes = [vp, i32, vp, vp, sz, vp, sz, vp]
    L.cryo_multi_decompress_blocks_to.argtypes = [vp, i32, vp, vp, sz, vp, sz, vp]
    L.cryo_multi_decompress_blocks_keyed.argtypes = [vp, i32, vp, vp, vp, sz, vp, sz, vp]
    L.cryo_multi_set_option.argtypes = [vp, i32, C.c_int64]
    L.cryo_multi_pool_invalidate.argtypes = [vp, u32, i32]
    L.cryo_codec_trim.argtypes = [vp]
    L.cryo_multi_trim.argtypes = [vp]
    L.cryo_multi_get_transfer_counters.argtypes = [vp, C.POINTER(TransferCounters)]
    L.cryo_codec_decompress_blocks_keyed.argtypes = [vp, i32, vp, vp, vp, sz, vp, sz, vp]
    L.cryo_codec_pool_invalidate.argtypes = [vp, u32, i32]
    L.cryo_codec_get_transfer_counters.argtypes = [vp, C.POINTER(TransferCounters)]
    L.cryo_codec_synth_batch.argtypes = [vp, u64, u64, u64, u64, u32, i32, vp, u64]
    L.cryo_codec_checksum_batch.argtypes = [vp, vp, u64, vp, u32, u64, vp]
    L.cryo_codec_compare_batch.argtypes = [vp, vp, u64, vp, u64, u32, u64, vp]
    L.cryo_checksum64.argtypes = [vp, sz]
    L.cryo_checksum64.restype = u64
    L.cryo_codec_timer_start.argtypes = [vp]
    L.cryo_codec_timer_stop.argtypes = [vp, C.POINTER(C.c_float)]
    L.cryo_codec_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.cryo_codec_verify_batch.argtypes = [vp, i32, vp, u64, u32, u64, vp, vp, vp, vp, vp]
    L.cryo_codec_last_verify_failure.argtypes = [vp, C.POINTER(u64), C.POINTER(u32)]
    L.cryo_multi_last_verify_failure.argtypes = [vp, C.POINTER(u64), C.POINTER(u32)]
    L.cryo_codec_check_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, vp]
    L.cryo_codec_check_blocks.argtypes = [vp, i32, vp, vp, sz, sz, vp]
    L.cryo_multi_check_blocks.argtypes = [vp, i32, vp, vp, sz, sz, vp]
    L.cryo_codec_recode_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, i32, i32, vp, u64, vp, vp]
    L.cryo_codec_recode_blocks.argtypes = [vp, i32, vp, vp, sz, sz, i32, i32, vp, sz, vp, vp, vp]
    L.cryo_multi_recode_blocks.argtypes = [vp, i32, vp, vp, sz, sz, i32, i32, vp, sz, vp, vp, vp]
    L.cryo_codec_fetch_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, vp, vp, u64, vp, u64, vp, vp]
    L.cryo_codec_fetch_blocks.argtypes = [vp, i32, vp, vp, sz, sz, vp, vp, vp, sz, vp, C.POINTER(u64)]
    L.cryo_multi_fetch_blocks.argtypes = [vp, i32, vp, vp, sz, sz, vp, vp, vp, sz, vp, C.POINTER(u64)]
    fp = C.POINTER(CryoFilter)
    L.cryo_codec_filter_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, fp, vp, u64, vp, u64, vp, vp]
    L.cryo_codec_filter_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, vp, sz, vp, sz, vp, vp]
    L.cryo_multi_filter_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, vp, sz, vp, sz, vp, vp]
    ap = C.POINTER(CryoAgg)
    L.cryo_codec_agg_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, fp, ap, vp, vp]
    L.cryo_codec_agg_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, ap, vp, vp]
    L.cryo_multi_agg_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, ap, vp, vp]
    gp = C.POINTER(CryoGroup)
    L.cryo_codec_group_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, fp, gp, ap, vp, vp, u64, vp, vp]
    L.cryo_codec_group_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, gp, ap, vp, vp, sz, vp, C.POINTER(u64)]
    L.cryo_multi_group_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, gp, ap, vp, vp, sz, vp, C.POINTER(u64)]
    pp = C.POINTER(CryoProject)
    L.cryo_codec_project_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, fp, pp, vp, u64, vp, u64, vp, vp]
    L.cryo_codec_project_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, pp, vp, sz, vp, sz, vp, vp]
    L.cryo_multi_project_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, pp, vp, sz, vp, sz, vp, vp]
    op = C.POINTER(CryoOrder)
    L.cryo_codec_topn_batch.argtypes = [vp, i32, vp, vp, vp, u32, u64, fp, op, pp, vp, vp, u64, vp, vp]
    L.cryo_codec_topn_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, op, pp, vp, vp, sz, vp, vp]
    L.cryo_multi_topn_blocks.argtypes = [vp, i32, vp, vp, sz, sz, fp, op, pp, vp, vp, sz, vp, vp]
    L.cryo_codec_lz4_index_cap.argtypes = [u32]
    L.cryo_codec_lz4_index_cap.restype = u32
    L.cryo_codec_lz4_index_rows.argtypes = [vp, vp, vp, vp, u32, u64, i32, vp, vp]
    L.cryo_codec_debug_fill.argtypes = [vp, i32, C.POINTER(FillReport)]
    _bound = True
    return L


def version():
    return lib().cryo_codec_version().decode()


def device_count():
    return lib().cryo_codec_device_count()


def bound(method, block_size):
    return lib().cryo_codec_bound(method, block_size)


def checksum64(data):
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
    return lib().cryo_checksum64(a.ctypes.data, a.nbytes)


def recode_blocks_call(fn, handle, chk, src_method, comps, block_size, dst_method, dst_param, dst=None):
    """cryo_codec_recode_blocks / cryo_multi_recode_blocks (fn) on a list of host streams"""
    n = len(comps)
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    if dst is None:
        dst = np.zeros(max(n, 1) * ((bound(dst_method, block_size) + 15) & ~15), np.uint8)
    off, osz, st = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.int32)
    chk(fn(handle, src_method, src, szs, n, block_size, dst_method, dst_param, dst.ctypes.data, dst.nbytes,
           off.ctypes.data, osz.ctypes.data, st.ctypes.data), "recode_blocks")
    off, osz, st = off[:n], osz[:n], st[:n]
    outs = [dst[int(off[i]):int(off[i]) + int(osz[i])] if st[i] == 0 else None for i in range(n)]
    return outs, st, off, osz, dst


def request_table(requests):
    """the CSR request table of a fetch call from one list of 1-based item positions per block: (req_first u64[n + 1],
    pos u16[n_req])"""
    first = np.zeros(len(requests) + 1, np.uint64)
    first[1:] = np.cumsum([len(r) for r in requests], dtype=np.uint64)
    pos = np.array([p for r in requests for p in r], np.uint16)
    return first, pos


def fetch_blocks_call(fn, handle, chk, method, comps, block_size, requests, dst=None):
    """cryo_codec_fetch_blocks / cryo_multi_fetch_blocks (fn) on a list of host streams and one list of positions per block;
    returns (records: FETCH_RESULT array in call order, dst, total).  dst: the caller's buffer (its capacity is len(dst)), else a
    fresh one of n * block_size bytes"""
    n = len(comps)
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    first, pos = request_table(requests)
    n_req = int(first[-1])
    if dst is None:
        dst = np.zeros(max(n, 1) * block_size, np.uint8)
    res = np.zeros(max(n_req, 1), FETCH_RESULT)
    total = C.c_uint64()
    chk(fn(handle, method, src, szs, n, block_size, first.ctypes.data, pos.ctypes.data if n_req else None, dst.ctypes.data,
           dst.nbytes, res.ctypes.data, C.byref(total)), "fetch_blocks")
    return res[:n_req], dst, total.value


def truth_dnf(terms, nkeys):
    """the truth table (CRYO_FILTER_TRUTH) of a disjunctive normal form over nkeys keys: each term a mask of the keys that are
    ANDed (bit k: keys[k]), the terms ORed.  Bit m of the result is set when some term lies within m, so the table is monotone.
    0 -- no valid table -- for no term, an empty term, a term beyond nkeys, or nkeys outside 1 .. 4 (cryo_filter_truth_dnf,
    host/filter.h)"""
    terms = [int(t) for t in terms]
    if not 1 <= nkeys <= FILTER_MAX_KEYS or not terms or any(t <= 0 or t >> nkeys for t in terms):
        return 0
    return sum(1 << m for m in range(1 << nkeys) if any(t & m == t for t in terms))


def truth_flags(flags=0, truth=None):
    """(flags, rsv) of a descriptor: with a truth table FILTER_TRUTH is set and rsv is the table; without one rsv is 0"""
    return (flags, 0) if truth is None else (flags | FILTER_TRUTH, int(truth))


def filter_desc(atts, keys=(), flags=0, truth=None):
    """the descriptor of a filter call as host arrays: atts a list of (attlen, attalign), keys a list of (att, type, op, value)
    (att 1-based; type KEY_*, op OP_*; the value of a KEY_BYTES comparison is a bytes object, that of an OP_IN / OP_NOT_IN key
    a sequence of ints, that of a KEY_FLOAT4 / KEY_FLOAT8 comparison a Python float or, as an int, the 64 bits of a double, that of an
    OP_LIKE / OP_NOT_LIKE key -- its type is KEY_BYTES -- a like(pattern, utf8) object).  Returns (CryoFilter, atts array,
    keys array); the struct points into the two arrays, which the caller keeps alive.  The constants of KEY_BYTES keys live in
    one uint8 array the struct holds (f.consts), so they live as long as it does.  truth: a truth table over the keys (truth_dnf):
    FILTER_TRUTH is set in flags and the table goes into rsv"""
    a = np.zeros(max(len(atts), 1), FILTER_ATT)
    for i, (attlen, attalign) in enumerate(atts):
        a[i] = (attlen, attalign, 0)
    k, consts = _filter_keys(keys)
    _rebase_keys(k, keys, consts.ctypes.data)
    flags, rsv = truth_flags(flags, truth)
    f = CryoFilter(len(atts), len(keys), flags, rsv, a.ctypes.data, k.ctypes.data if len(keys) else None)
    f.consts = consts
    return f, a, k


class like:
    """the value of an OP_LIKE / OP_NOT_LIKE key, so that the key stays (att, KEY_BYTES, op, value): the pattern's bytes ('%',
    '_' and '\\' as in SQL with ESCAPE '\\'; a str is encoded as UTF-8) and whether a character is a UTF-8 character (utf8) or a
    byte.  pattern None: no bytes and a null address.  rsv: the key's rsv word as given, for descriptors the library must
    refuse; otherwise it is the pattern's length with LIKE_UTF8 under utf8"""

    def __init__(self, pattern, utf8=True, rsv=None):
        self.pattern = None if pattern is None else pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
        self.utf8 = bool(utf8)
        self.rsv = (len(self.pattern or b"") | (LIKE_UTF8 if self.utf8 else 0)) if rsv is None else int(rsv)

    def __len__(self):
        return len(self.pattern or b"")

    def __repr__(self):
        return "like(%r, utf8=%r, rsv=0x%x)" % (self.pattern, self.utf8, self.rsv)


def _is_like_key(key):
    """a key whose value is a pattern"""
    return isinstance(key[3], like)


def _is_bytes_key(key):
    """a key whose value is a byte string (None: no bytes and a null address)"""
    return key[1] == KEY_BYTES and isinstance(key[3], (bytes, bytearray, memoryview, type(None)))


def _is_set_key(key):
    """a key whose value is a list of integers (None under OP_IN / OP_NOT_IN: no members and a null address)"""
    return isinstance(key[3], (list, tuple, range, np.ndarray)) or (key[3] is None and key[2] in (OP_IN, OP_NOT_IN))


def float_key_bits(value):
    """the value field of a float key: the 64 bits of the double `value` (a Python float), or of the bits given as an int, as
    the signed integer the field is"""
    bits = struct.unpack("<Q", struct.pack("<d", value))[0] if isinstance(value, float) else int(value) & (1 << 64) - 1
    return bits - (1 << 64) if bits >> 63 else bits


def _filter_keys(keys):
    """(keys array with rsv = the length and value = the offset of each KEY_BYTES constant, rsv = the number of members and
    value = the offset of each set key's list -- little-endian int64 --, rsv = like.rsv and value = the offset of each pattern
    key's pattern, constants, lists and patterns packed back to back)"""
    k = np.zeros(max(len(keys), 1), FILTER_KEY)
    parts, at = [], 0
    for i, key in enumerate(keys):
        att, typ, op, value = key
        if _is_bytes_key(key):
            value = bytes(value or b"")
            k[i] = (att, typ, op, len(value), at)
            parts.append(value)
            at += len(value)
        elif _is_like_key(key):
            k[i] = (att, typ, op, value.rsv, at)
            parts.append(value.pattern or b"")
            at += len(value)
        elif _is_set_key(key):
            value = () if value is None else value
            members = b"".join(int(m).to_bytes(8, "little", signed=True) for m in value)
            k[i] = (att, typ, op, len(value), at)
            parts.append(members)
            at += len(members)
        elif typ in (KEY_FLOAT4, KEY_FLOAT8) and OP_LT <= op <= OP_NE:
            k[i] = (att, typ, op, 0, float_key_bits(value))
        else:
            k[i] = (att, typ, op, 0, value)
    consts = np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy()        # never empty: it has an address
    return k, consts


def _rebase_keys(k, keys, base):
    """offsets into the packed constants -> addresses from `base` on; an empty constant keeps a null address"""
    for i, key in enumerate(keys):
        if _is_bytes_key(key) or _is_set_key(key) or _is_like_key(key):
            k[i]["value"] = base + int(k[i]["value"]) if (key[3] is not None and len(key[3])) else 0


def filter_desc_device(atts, keys=(), flags=0, truth=None):
    """the device form of a descriptor with KEY_BYTES keys or set keys: returns (atts array, keys array, consts array, rebase).  The caller
    uploads consts to device memory at some address d and calls rebase(d), which sets every KEY_BYTES key's and set key's value to the
    device address of its constant or list (they lie back to back in consts, at any alignment); then it uploads the keys.
    rebase.flags and rebase.rsv are the struct's two words (truth_flags of flags and truth), which the *_batch calls take as
    flags and truth"""
    a = np.zeros(max(len(atts), 1), FILTER_ATT)
    for i, (attlen, attalign) in enumerate(atts):
        a[i] = (attlen, attalign, 0)
    k, consts = _filter_keys(keys)
    offs = k["value"].copy()

    def rebase(d_consts):
        k["value"] = offs
        _rebase_keys(k, keys, int(d_consts))
        return k
    rebase.flags, rebase.rsv = truth_flags(flags, truth)
    return a, k, consts, rebase


def filter_blocks_call(fn, handle, chk, method, comps, block_size, desc, dst=None, rec=None):
    """cryo_codec_filter_blocks / cryo_multi_filter_blocks (fn) on a list of host streams with the descriptor filter_desc made;
    returns (table: FILTER_BLOCK array in call order, records: the FILTER_REC buffer, dst, (total bytes, total records)).
    dst / rec: the caller's buffers (their capacities are their lengths), else fresh ones of the worst-case size"""
    n = len(comps)
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    if dst is None:
        dst = np.zeros(max(n, 1) * block_size, np.uint8)
    if rec is None:
        rec = np.zeros(max(n, 1) * 290, FILTER_REC)
    table = np.zeros(max(n, 1), FILTER_BLOCK)
    total = (C.c_uint64 * 2)()
    chk(fn(handle, method, src, szs, n, block_size, C.byref(desc[0]), dst.ctypes.data if dst.size else None, dst.nbytes,
           rec.ctypes.data if rec.size else None, rec.size, table.ctypes.data, total), "filter_blocks")
    return table[:n], rec, dst, (total[0], total[1])


def agg_desc(cols):
    """the aggregate descriptor of an agg call as a host array: cols a list of (att, type) (att 1-based; type KEY_*).  Returns
    (CryoAgg, cols array); the struct points into the array, which the caller keeps alive"""
    a = np.zeros(max(len(cols), 1), AGG_COL)
    for j, (att, typ) in enumerate(cols):
        a[j] = (att, typ, 0, 0)
    return CryoAgg(len(cols), 0, a.ctypes.data), a


def agg_blocks_call(fn, handle, chk, method, comps, block_size, desc, adesc):
    """cryo_codec_agg_blocks / cryo_multi_agg_blocks (fn) on a list of host streams with the descriptors filter_desc and agg_desc
    made; returns (rows: AGG_BLOCK array in call order, cells: AGG_CELL array of shape (n, ncols))"""
    n, ncols = len(comps), adesc[0].ncols
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    rows = np.zeros(max(n, 1), AGG_BLOCK)
    cells = np.zeros((max(n, 1), max(ncols, 1)), AGG_CELL)
    chk(fn(handle, method, src, szs, n, block_size, C.byref(desc[0]), C.byref(adesc[0]), rows.ctypes.data, cells.ctypes.data),
        "agg_blocks")
    return rows[:n], cells[:n]


def bucket_array(buckets):
    """buckets, a list of (kind, flags, origin, value) with one entry per group column (value: a WIDTH bucket's width, a
    BOUNDS bucket's sequence of boundaries, in any order), as (BUCKET array, lists array, rebase): the lists lie back to back in
    the uint8 array `lists` as little-endian int64 (behind one pad byte: at no alignment); once the caller knows where they lie --
    host memory, or device memory after an upload -- rebase(address) sets every BOUNDS bucket's value and returns the array"""
    b = np.zeros(max(len(buckets), 1), BUCKET)
    parts, at, offs = [b"\0"], 1, {}
    for j, (kind, flags, origin, value) in enumerate(buckets):
        if kind == BUCKET_BOUNDS and value is not None and not isinstance(value, int):
            members = b"".join(int(m).to_bytes(8, "little", signed=True) for m in value)
            b[j] = (kind, flags, 0, len(value), origin, 0)
            if len(value):
                offs[j] = at
            parts.append(members)
            at += len(members)
        else:
            b[j] = (kind, flags, 0, 0, origin, value or 0)
    lists = np.frombuffer(b"".join(parts), np.uint8).copy()

    def rebase(base):
        for j, off in offs.items():
            b[j]["value"] = int(base) + off
        return b
    return b, lists, rebase


def group_desc(by, buckets=None, text=False):
    """the group descriptor of a group call as a host array: by a list of (att, type) (att 1-based; type KEY_*).  Returns
    (CryoGroup, by array); the struct points into the array, which the caller keeps alive.  buckets: one (kind, flags, origin,
    value) per group column (bucket_array) -- the struct is then a CryoGroupB, which holds the buckets array and the lists of
    boundaries it points into (g.bucket_arr, g.bucket_lists).  text: the struct's rsv is GROUP_TEXT and a column's type may be
    KEY_BYTES; with buckets as well the library refuses the descriptor"""
    a = np.zeros(max(len(by), 1), AGG_COL)
    for j, (att, typ) in enumerate(by):
        a[j] = (att, typ, 0, 0)
    if buckets is None:
        return CryoGroup(len(by), GROUP_TEXT if text else 0, a.ctypes.data), a
    b, lists, rebase = bucket_array(buckets)
    rebase(lists.ctypes.data)
    g = CryoGroupB(len(by), GROUP_BUCKETS | (GROUP_TEXT if text else 0), a.ctypes.data, b.ctypes.data)
    g.bucket_arr, g.bucket_lists = b, lists
    return g, a


def group_blocks_call(fn, handle, chk, method, comps, block_size, desc, gdesc, adesc=None, group_cap=None):
    """cryo_codec_group_blocks / cryo_multi_group_blocks (fn) on a list of host streams with the descriptors filter_desc,
    group_desc and agg_desc made (adesc None: no aggregate column, a null agg and null cells); returns (rows: GROUP_BLOCK array
    in call order, records: GROUP_REC array of the call's groups, cells: AGG_CELL array of shape (groups, ncols), total).
    group_cap: the room in records (default: the worst case, 290 per block).  A GROUP_TEXT descriptor (group_desc(text=True))
    returns a fifth item: the key cells, a GROUP_KEY array of shape (groups, ntext), one column per KEY_BYTES group column"""
    n, ncols = len(comps), adesc[0].ncols if adesc else 0
    if gdesc[0].rsv == GROUP_TEXT:
        return _group_text_blocks_call(fn, handle, chk, method, comps, block_size, desc, gdesc, adesc, group_cap)
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    cap = 290 * n if group_cap is None else group_cap
    rows = np.zeros(max(n, 1), GROUP_BLOCK)
    recs = np.zeros(max(cap, 1), GROUP_REC)
    cells = np.zeros((max(cap, 1), max(ncols, 1)), AGG_CELL)
    total = C.c_uint64()
    chk(fn(handle, method, src, szs, n, block_size, C.byref(desc[0]), C.byref(gdesc[0]), C.byref(adesc[0]) if adesc else None,
           rows.ctypes.data, recs.ctypes.data, cap, cells.ctypes.data if ncols else None, C.byref(total)), "group_blocks")
    return rows[:n], recs[:total.value], cells[:total.value, :ncols], total.value


def group_text_count(gdesc):
    """how many of a group descriptor's columns are KEY_BYTES"""
    return sum(1 for c in gdesc[1][:gdesc[0].nby] if int(c["type"]) == KEY_BYTES)


def group_cells_split(cells, ncols, ntext):
    """the cells of a GROUP_TEXT call, shape (groups, ncols + ntext) of 40 bytes each, as (AGG_CELL (groups, ncols), GROUP_KEY
    (groups, ntext)): copies"""
    raw = np.ascontiguousarray(cells).view(np.uint8).reshape(len(cells), (ncols + ntext) * 40)
    agg = np.frombuffer(raw[:, :ncols * 40].tobytes(), AGG_CELL).reshape(len(cells), ncols).copy()
    key = np.frombuffer(raw[:, ncols * 40:].tobytes(), GROUP_KEY).reshape(len(cells), ntext).copy()
    return agg, key


def _group_text_blocks_call(fn, handle, chk, method, comps, block_size, desc, gdesc, adesc, group_cap):
    """group_blocks_call for a GROUP_TEXT descriptor: a group has ncols + ntext cells"""
    n, ncols, ntext = len(comps), adesc[0].ncols if adesc else 0, group_text_count(gdesc)
    cpg = ncols + ntext
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    cap = 290 * n if group_cap is None else group_cap
    rows = np.zeros(max(n, 1), GROUP_BLOCK)
    recs = np.zeros(max(cap, 1), GROUP_REC)
    cells = np.zeros((max(cap, 1), max(cpg, 1), 40), np.uint8)
    total = C.c_uint64()
    chk(fn(handle, method, src, szs, n, block_size, C.byref(desc[0]), C.byref(gdesc[0]), C.byref(adesc[0]) if adesc else None,
           rows.ctypes.data, recs.ctypes.data, cap, cells.ctypes.data if cpg else None, C.byref(total)), "group_blocks")
    agg, key = group_cells_split(cells[:total.value, :cpg].reshape(total.value, cpg * 40), ncols, ntext)
    return rows[:n], recs[:total.value], agg, total.value, key


def project_desc(cols):
    """the projection of a project call as a host array: cols a list of column numbers (1-based).  Returns (CryoProject, cols
    array); the struct points into the array, which the caller keeps alive"""
    a = np.zeros(max(len(cols), 1), PROJECT_COL)
    for j, att in enumerate(cols):
        a[j] = (att, 0, 0)
    return CryoProject(len(cols), 0, a.ctypes.data), a


def project_row_layout(atts, cols):
    """the row layout rule of include/cryo_codec.h: atts a list of (attlen, attalign), cols a list of column numbers (1-based)
    of width 1, 2, 4 or 8.  Returns (offsets, row_bytes): o_0 = 0, o_j = align(o_(j-1) + w_(j-1), w_j), row_bytes =
    MAXALIGN(o_last + w_last)"""
    offsets, end = [], 0
    for att in cols:
        w = atts[att - 1][0]
        o = (end + w - 1) & ~(w - 1)
        offsets.append(o)
        end = o + w
    return offsets, (end + 7) & ~7


def project_blocks_call(fn, handle, chk, method, comps, block_size, desc, pdesc, row_bytes, rows=None, rec=None):
    """cryo_codec_project_blocks / cryo_multi_project_blocks (fn) on a list of host streams with the descriptors filter_desc and
    project_desc made; row_bytes: what project_row_layout says.  Returns (table: PROJECT_BLOCK array in call order, records: the
    PROJECT_REC buffer, rows: a uint8 buffer of shape (row_cap, row_bytes), (total rows, total records)).  rows / rec: the
    caller's buffers (their capacities are their lengths), else fresh ones of the worst-case size, 290 per block"""
    n = len(comps)
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    if rows is None:
        rows = np.zeros((max(n, 1) * 290, row_bytes), np.uint8)
    if rec is None:
        rec = np.zeros(max(n, 1) * 290, PROJECT_REC)
    table = np.zeros(max(n, 1), PROJECT_BLOCK)
    total = (C.c_uint64 * 2)()
    chk(fn(handle, method, src, szs, n, block_size, C.byref(desc[0]), C.byref(pdesc[0]), rows.ctypes.data if rows.size else None,
           rows.shape[0], rec.ctypes.data if rec.size else None, rec.size, table.ctypes.data, total), "project_blocks")
    return table[:n], rec, rows, (total[0], total[1])


def order_desc(by, limit):
    """the order of a topn call as a host array: by a list of (att, type, flags) (att 1-based; type KEY_INT2 .. KEY_INT8,
    KEY_FLOAT4, KEY_FLOAT8; flags ORDER_DESC | ORDER_NULLS_FIRST).  Returns (CryoOrder, by array); the struct points into the
    array, which the caller keeps alive"""
    a = np.zeros(max(len(by), 1), ORDER_COL)
    for j, (att, typ, flags) in enumerate(by):
        a[j] = (att, typ, flags, 0)
    return CryoOrder(len(by), limit, a.ctypes.data), a


def topn_blocks_call(fn, handle, chk, method, comps, block_size, desc, odesc, pdesc, row_bytes, rows=None, rec=None):
    """cryo_codec_topn_blocks / cryo_multi_topn_blocks (fn) on a list of host streams with the descriptors filter_desc,
    order_desc and project_desc made; row_bytes: what project_row_layout says.  Returns (table: TOPN_BLOCK array in call order,
    records: the TOPN_REC buffer, rows: a uint8 buffer of shape (row_cap, row_bytes), total kept rows).  rows / rec: the caller's
    buffers (the capacity is the shorter one's length), else fresh ones of the worst-case size, min(limit, 290) per block"""
    n = len(comps)
    arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
    src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
    szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
    per = min(int(odesc[0].limit), 290)
    if rows is None:
        rows = np.zeros((max(n, 1) * max(per, 1), row_bytes), np.uint8)
    if rec is None:
        rec = np.zeros(max(n, 1) * max(per, 1), TOPN_REC)
    cap = min(rows.shape[0], rec.size)
    table = np.zeros(max(n, 1), TOPN_BLOCK)
    total = C.c_uint64(0)
    chk(fn(handle, method, src, szs, n, block_size, C.byref(desc[0]), C.byref(odesc[0]), C.byref(pdesc[0]),
           rows.ctypes.data if cap else None, rec.ctypes.data if cap else None, cap, table.ctypes.data, C.byref(total)), "topn_blocks")
    return table[:n], rec, rows, total.value


def topn_sort_key(by, rec):
    """what the order of the descriptor (by: a list of (att, type, flags)) compares of a TOPN_REC: per order column (class, key
    under the direction); Python tuples of these sort as the contract's order does"""
    out = []
    for j, (_, _, flags) in enumerate(by):
        if (int(rec["key_nulls"]) >> j) & 1:
            out.append((0 if flags & ORDER_NULLS_FIRST else 2, 0))
        else:
            k = int(rec["key"][j])
            out.append((1, ~k if flags & ORDER_DESC else k))
    return tuple(out)


def topn_merge(by, limit, blocks):
    """the merge of a call's blocks: by as for order_desc, blocks a sequence of (records, rows) -- one block's TOPN_REC array and
    its rows, in the block's order -- of the blocks the caller's snapshot sees, in the order they are added.  Returns (records,
    rows) of the first `limit` rows of the whole: ordered by the descriptor over key / key_nulls, ties to the block added earlier,
    then to the block's own order"""
    entries = []
    for b, (recs, rows) in enumerate(blocks):
        for r in range(len(recs)):
            entries.append((topn_sort_key(by, recs[r]), b, r))
    entries.sort()
    entries = entries[:limit]
    row_bytes = next((rows.shape[1] for _, rows in blocks if len(rows)), 0)
    out_rec = np.zeros(len(entries), TOPN_REC)
    out_rows = np.zeros((len(entries), row_bytes), np.uint8)
    for i, (_, b, r) in enumerate(entries):
        out_rec[i] = blocks[b][0][r]
        out_rows[i] = blocks[b][1][r]
    return out_rec, out_rows


def cell_sum(cell):
    """the exact sum of an AGG_CELL as a Python integer"""
    return (int(cell["sum_hi"]) << 64) + int(cell["sum_lo"])


FLOAT_NAN_BITS = 0x7FF8000000000000            # the canonical NaN of a float cell


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def cell_float(cell):
    """(n, min, max, sum, err) of an AGG_CELL that holds a float column's cell (cryo_agg_cell_f): Python floats, bit for bit"""
    c = np.frombuffer(np.asarray(cell).tobytes(), AGG_CELL_F)[0]
    return int(c["n"]), float(c["min"]), float(c["max"]), float(c["sum"]), float(c["err"])


def float_order(x):
    """the signed integer whose order is the float keys' order of the double x: a NaN INT64_MAX, a zero 0"""
    b = _bits(x)
    if b & 0x7FFFFFFFFFFFFFFF > 0x7FF0000000000000:
        return (1 << 63) - 1
    if b & 0x7FFFFFFFFFFFFFFF == 0:
        return 0
    return -(b & 0x7FFFFFFFFFFFFFFF) - 1 if b >> 63 else b


def float_pair_add(x, y):
    """x (+) y of include/cryo_codec.h ("The reduction") on pairs (hi, lo) of Python floats, which are IEEE doubles"""
    s = x[0] + y[0]
    bb = s - x[0]
    e = (x[0] - (s - bb)) + (y[0] - bb)
    t = e + (x[1] + y[1])
    h = s + t
    return h, t - (h - s)


def cell_float_combine(a, b):
    """the float cell of two blocks' (or groups') float cells, a before b, as cryo_agg_cell_f_combine (host/aggregate.h): each
    and the result (n, min, max, sum, err) as cell_float gives them.  n adds; min / max in the float keys' order, canonical;
    NaN, or both infinities, give (NaN, +0), one infinity (that, +0); otherwise (sum, err) is a (+) b, and a pair that left the
    double range (NaN, NaN)"""
    if a[0] == 0 or b[0] == 0:
        return tuple(b if a[0] == 0 else a)
    nan = _f64(FLOAT_NAN_BITS)
    lo = min(a[1], b[1], key=float_order)
    hi = max(a[2], b[2], key=float_order)
    lo, hi = (nan if x != x else x + 0.0 if x == 0 else x for x in (lo, hi))
    inf = float("inf")

    def kind(c):
        # (P, M, Q, overflow) of a cell's (sum, err)
        s, e = c[3], c[4]
        if e != e:
            return False, False, False, True
        return s == inf, s == -inf, s != s, False
    ka, kb = kind(a), kind(b)
    P, M, Q, V = (ka[i] or kb[i] for i in range(4))
    if Q or (P and M):
        s, e = nan, 0.0
    elif P or M:
        s, e = (inf if P else -inf), 0.0
    elif V:
        s, e = nan, nan
    else:
        s, e = float_pair_add((a[3], a[4]), (b[3], b[4]))
        if s != s or e != e or abs(s) == inf or abs(e) == inf:
            s, e = nan, nan
    return a[0] + b[0], lo, hi, s, e


class DeviceBuffer:
    """A hipMalloc'ed region owned by a Codec handle."""

    def __init__(self, codec, nbytes):
        self.codec = codec
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        codec._chk(codec.L.cryo_dev_alloc(codec.h, self.nbytes, C.byref(p)), "cryo_dev_alloc")
        self.ptr = p.value

    def free(self):
        if self.ptr:
            self.codec.L.cryo_dev_free(self.codec.h, self.ptr)
            self.ptr = None

    def upload(self, arr, offset=0):
        a = np.ascontiguousarray(arr)
        assert offset + a.nbytes <= self.nbytes
        self.codec._chk(self.codec.L.cryo_dev_upload(self.codec.h, self.ptr + offset, a.ctypes.data, a.nbytes),
                        "cryo_dev_upload")

    def download(self, nbytes=None, offset=0, dtype=np.uint8):
        nbytes = self.nbytes - offset if nbytes is None else int(nbytes)
        out = np.empty(nbytes, dtype=np.uint8)
        self.codec._chk(self.codec.L.cryo_dev_download(self.codec.h, out.ctypes.data, self.ptr + offset, nbytes),
                        "cryo_dev_download")
        return out.view(dtype)

    def memset(self, value=0):
        self.codec._chk(self.codec.L.cryo_dev_memset(self.codec.h, self.ptr, value, self.nbytes), "cryo_dev_memset")


class Codec:
    """One handle = one GPU + one HIP stream (include/cryo_codec.h)."""

    def __init__(self, device=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.cryo_codec_open(device, C.byref(h))
        if rc != OK:
            raise CryoError(rc, "cryo_codec_open(%d)" % device,
                            "no CPU fallback exists; a gfx950 GPU and the HIP runtime are required")
        self.h = h.value
        self.device = device

    def close(self):
        if self.h:
            self.L.cryo_codec_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != OK:
            raise CryoError(rc, what, (self.L.cryo_codec_last_error(self.h) or b"").decode())

    # -- plumbing --
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def sync(self):
        self._chk(self.L.cryo_codec_sync(self.h), "cryo_codec_sync")

    def set_option(self, option, value):
        self._chk(self.L.cryo_codec_set_option(self.h, option, int(value)), "cryo_codec_set_option")

    def get_option(self, option):
        v = C.c_int64()
        self._chk(self.L.cryo_codec_get_option(self.h, option, C.byref(v)), "cryo_codec_get_option")
        return v.value

    def timer_start(self):
        self._chk(self.L.cryo_codec_timer_start(self.h), "timer_start")

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.L.cryo_codec_timer_stop(self.h, C.byref(ms)), "timer_stop")
        return ms.value

    def transfer_counters(self):
        t = TransferCounters()
        self._chk(self.L.cryo_codec_get_transfer_counters(self.h, C.byref(t)), "get_transfer_counters")
        return {f: getattr(t, f) for f, _ in TransferCounters._fields_}

    def trim(self):
        self._chk(self.L.cryo_codec_trim(self.h), "cryo_codec_trim")

    def debug_fill(self, value):
        """test aid: wait for the handle's streams and fill every handle-owned buffer (not the keyed pool) with the byte `value`
        over its whole capacity; returns the bytes filled per buffer as a dict (pipe_pin0 .. pipe_pin3 for the four pipeline
        staging buffers), 0 for a buffer that is not allocated"""
        r = FillReport()
        self._chk(self.L.cryo_codec_debug_fill(self.h, value, C.byref(r)), "cryo_codec_debug_fill")
        out = {f: int(getattr(r, f)) for f, _ in FillReport._fields_ if f != "pipe_pin"}
        out.update(("pipe_pin%d" % i, int(r.pipe_pin[i])) for i in range(4))
        return out

    def pool_invalidate(self, key_hi=0, everything=False):
        self._chk(self.L.cryo_codec_pool_invalidate(self.h, key_hi, 1 if everything else 0), "pool_invalidate")

    def decompress_blocks_keyed(self, method, keys, comps, block_size):
        """host buffers in, host buffers out, through the device-resident pool; returns (list of arrays|None, statuses)"""
        n = len(comps)
        arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
        src = (C.c_void_p * n)(*[a.ctypes.data if a.nbytes else None for a in arrs])
        szs = (C.c_uint32 * n)(*[a.nbytes for a in arrs])
        outs = [np.full(block_size, 0xA5, np.uint8) for _ in range(n)]
        dst = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        st = (C.c_int32 * n)()
        ks = (C.c_uint64 * n)(*[int(k) for k in keys])
        self._chk(self.L.cryo_codec_decompress_blocks_keyed(self.h, method, ks, src, szs, n, dst, block_size, st),
                  "decompress_blocks_keyed")
        st = np.array(list(st), np.int32)
        return [outs[i] if st[i] == 0 else None for i in range(n)], st

    def counters(self):
        c = Counters()
        self._chk(self.L.cryo_codec_get_counters(self.h, C.byref(c)), "get_counters")
        return {f: getattr(c, f) for f, _ in Counters._fields_}

    # -- device-resident batches (async on the handle's stream) --
    def synth_batch(self, seed, first_block, n, block_size, dist, d_dst, stride=None, block_step=1):
        stride = block_size if stride is None else stride
        self._chk(self.L.cryo_codec_synth_batch(self.h, seed, first_block, block_step, n, block_size, dist,
                                                d_dst.ptr, stride),
                  "synth_batch")

    def compress_batch(self, method, param, d_src, src_stride, block_size, n, d_dst, dst_stride, d_sizes, d_status):
        self._chk(self.L.cryo_codec_compress_batch(self.h, method, param, d_src.ptr, src_stride, block_size, n,
                                                   d_dst.ptr, dst_stride, d_sizes.ptr, d_status.ptr),
                  "compress_batch")

    def decompress_batch(self, method, d_src, d_off, d_sizes, d_dst, dst_stride, block_size, n, d_status):
        self._chk(self.L.cryo_codec_decompress_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, d_dst.ptr,
                                                     dst_stride, block_size, n, d_status.ptr),
                  "decompress_batch")

    def lz4_index_cap(self, block_size):
        """16-bit entries per row of the one-walker LZ4 sequence index of a block size"""
        return int(self.L.cryo_codec_lz4_index_cap(block_size))

    def lz4_index_rows(self, d_src, d_off, d_sizes, block_size, n, form, d_entries, d_counts):
        """build the one-walker LZ4 sequence index of the batch with `form` (LZ4_INDEX_*) into d_entries (n x lz4_index_cap
        uint16) and d_counts (n uint32).  Asynchronous."""
        self._chk(self.L.cryo_codec_lz4_index_rows(self.h, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, form,
                                                   d_entries.ptr, d_counts.ptr),
                  "lz4_index_rows")

    def verify_batch(self, method, d_raw, raw_stride, block_size, n, d_comp, d_off, d_sizes, d_status, d_first=None):
        """decode the n streams (d_comp + d_off[i], d_sizes[i] bytes) and compare them with the raw blocks: d_status[i] = OK /
        E_VERIFY, d_first[i] = first differing byte (VERIFY_NONE: none, or the stream does not decode).  Asynchronous."""
        self._chk(self.L.cryo_codec_verify_batch(self.h, method, d_raw.ptr, raw_stride, block_size, n, d_comp.ptr, d_off.ptr,
                                                 d_sizes.ptr, d_status.ptr, d_first.ptr if d_first else None),
                  "verify_batch")

    def check_batch(self, method, d_src, d_off, d_sizes, block_size, n, d_result):
        """check the n stored blocks (d_src + d_off[i], d_sizes[i] bytes): d_result[i] = {reason, offset} (CHECK_*), 8 bytes per
        block.  Asynchronous."""
        self._chk(self.L.cryo_codec_check_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, d_result.ptr),
                  "check_batch")

    def check_blocks(self, method, comps, block_size):
        """check host compressed blocks; returns an (n, 2) uint32 array of {reason, offset}"""
        n = len(comps)
        arrs = [np.ascontiguousarray(np.asarray(c, dtype=np.uint8)) for c in comps]
        src = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.nbytes else None for a in arrs])
        szs = (C.c_uint32 * max(n, 1))(*[a.nbytes for a in arrs])
        out = np.zeros((n, 2), np.uint32)
        self._chk(self.L.cryo_codec_check_blocks(self.h, method, src, szs, n, block_size, out.ctypes.data), "check_blocks")
        return out

    def recode_batch(self, src_method, d_src, d_off, d_sizes, block_size, n, dst_method, dst_param, d_dst, dst_stride,
                     d_out_sizes, d_status):
        """decode the n streams (d_src + d_off[i], d_sizes[i] bytes) into handle workspace and encode them again into
        d_dst + i * dst_stride: d_out_sizes[i], d_status[i] (OK / E_CORRUPT / E_VERIFY).  Asynchronous."""
        self._chk(self.L.cryo_codec_recode_batch(self.h, src_method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n,
                                                 dst_method, dst_param, d_dst.ptr, dst_stride, d_out_sizes.ptr, d_status.ptr),
                  "recode_batch")

    def recode_blocks(self, src_method, comps, block_size, dst_method, dst_param, dst=None):
        """recompress host streams; returns (streams, statuses, offsets, sizes, dst): streams[i] is a view of dst (None for a
        block whose status is not OK), dst the packed buffer (a fresh one of the worst-case size unless the caller brings
        one: its capacity is len(dst))"""
        return recode_blocks_call(self.L.cryo_codec_recode_blocks, self.h, self._chk, src_method, comps, block_size,
                                  dst_method, dst_param, dst)

    def fetch_batch(self, method, d_src, d_off, d_sizes, block_size, n, d_req_first, d_pos, n_req, d_dst, dst_cap, d_result,
                    d_total):
        """gather the requested tuples of the n stored blocks (d_src + d_off[i], d_sizes[i] bytes): block i owns requests
        d_req_first[i] .. d_req_first[i + 1] - 1 of d_pos (1-based item positions); d_result[r] = {status, len, off} (FETCH_*,
        16 bytes per request), the tuples packed into d_dst, the packed total in d_total (u64).  Asynchronous."""
        self._chk(self.L.cryo_codec_fetch_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, d_req_first.ptr,
                                                d_pos.ptr if d_pos else None, n_req, d_dst.ptr if d_dst else None, dst_cap,
                                                d_result.ptr if d_result else None, d_total.ptr), "fetch_batch")

    def fetch_blocks(self, method, comps, block_size, requests, dst=None):
        """fetch tuples of host streams by position (requests[i]: the 1-based item positions wanted of block i, ascending);
        returns (records, dst, total): records a FETCH_RESULT array in call order, tuple r the records[r]["len"] bytes at
        dst[records[r]["off"]:] when its status is FETCH_OK"""
        return fetch_blocks_call(self.L.cryo_codec_fetch_blocks, self.h, self._chk, method, comps, block_size, requests, dst)

    def filter_batch(self, method, d_src, d_off, d_sizes, block_size, n, natts, d_atts, nkeys, d_keys, flags, d_dst, dst_cap,
                     d_rec, rec_cap, d_blocks, d_total, truth=None):
        """test the keys (d_keys: FILTER_KEY, d_atts: FILTER_ATT, device arrays) on every tuple of the n stored blocks: one
        FILTER_BLOCK row per block in d_blocks, one FILTER_REC per match and per bad item in d_rec, the matches packed into
        d_dst, the two totals {bytes, records} in d_total (2 x u64).  truth: a truth table over the keys (truth_dnf; FILTER_TRUTH
        is set for it).  Asynchronous once the descriptor is read back."""
        flags, rsv = truth_flags(flags, truth)
        f = CryoFilter(natts, nkeys, flags, rsv, d_atts.ptr if d_atts else None, d_keys.ptr if d_keys else None)
        self._chk(self.L.cryo_codec_filter_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, C.byref(f),
                                                 d_dst.ptr if d_dst else None, dst_cap, d_rec.ptr if d_rec else None, rec_cap,
                                                 d_blocks.ptr if d_blocks else None, d_total.ptr if d_total else None),
                  "filter_batch")

    def filter_blocks(self, method, comps, block_size, desc, dst=None, rec=None):
        """filter host streams (desc: what filter_desc returns); returns (table, records, dst, (bytes, records)): block i's
        records are records[table[i]["rec_first"]:][:n_match + n_bad], its tuples lie MAXALIGN-packed from dst[table[i]["off"]:]"""
        return filter_blocks_call(self.L.cryo_codec_filter_blocks, self.h, self._chk, method, comps, block_size, desc, dst, rec)

    def agg_batch(self, method, d_src, d_off, d_sizes, block_size, n, natts, d_atts, nkeys, d_keys, ncols, d_cols, d_blocks,
                  d_cells, truth=None):
        """test the keys on every tuple of the n stored blocks and reduce the ncols columns d_cols names (AGG_COL; d_keys:
        FILTER_KEY, d_atts: FILTER_ATT, device arrays) over each block's matches: one AGG_BLOCK row per block in d_blocks, ncols
        AGG_CELL cells per block in d_cells.  truth: as for filter_batch.  Asynchronous once the descriptors are read back."""
        f = CryoFilter(natts, nkeys, *truth_flags(0, truth), d_atts.ptr if d_atts else None, d_keys.ptr if d_keys else None)
        a = CryoAgg(ncols, 0, d_cols.ptr if d_cols else None)
        self._chk(self.L.cryo_codec_agg_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, C.byref(f),
                                              C.byref(a), d_blocks.ptr if d_blocks else None, d_cells.ptr if d_cells else None),
                  "agg_batch")

    def agg_blocks(self, method, comps, block_size, desc, adesc):
        """aggregate host streams (desc: what filter_desc returns, adesc: what agg_desc returns); returns (rows, cells): rows an
        AGG_BLOCK array in call order, cells an AGG_CELL array of shape (n, ncols); cell_sum gives a cell's 128-bit sum"""
        return agg_blocks_call(self.L.cryo_codec_agg_blocks, self.h, self._chk, method, comps, block_size, desc, adesc)

    def group_batch(self, method, d_src, d_off, d_sizes, block_size, n, natts, d_atts, nkeys, d_keys, nby, d_by, ncols, d_cols,
                    d_blocks, d_groups, group_cap, d_cells, d_total, truth=None, buckets=None, text=False):
        """test the keys on every tuple of the n stored blocks, partition each block's matches by the nby columns d_by names and
        reduce the ncols columns d_cols names per group (both AGG_COL; d_keys: FILTER_KEY, d_atts: FILTER_ATT, device arrays):
        one GROUP_BLOCK row per block in d_blocks, one GROUP_REC per group in d_groups and ncols AGG_CELL per group in d_cells (at
        most group_cap groups are written), the call's number of groups in d_total (u64).  ncols 0: d_cols and d_cells may be
        None.  truth: as for filter_batch.  buckets: a device array of nby BUCKET entries whose lists of boundaries lie in device
        memory (bucket_array).  text: the descriptor's rsv is GROUP_TEXT: d_by may name KEY_BYTES columns, and a group then has
        ncols + ntext cells of 40 bytes in d_cells, a GROUP_KEY per such column behind its AGG_CELLs.  Asynchronous once the
        descriptors are read back."""
        f = CryoFilter(natts, nkeys, *truth_flags(0, truth), d_atts.ptr if d_atts else None, d_keys.ptr if d_keys else None)
        g = CryoGroup(nby, GROUP_TEXT if text else 0, d_by.ptr if d_by else None)
        if buckets is not None:
            g = CryoGroupB(nby, GROUP_BUCKETS | (GROUP_TEXT if text else 0), d_by.ptr if d_by else None, buckets.ptr)
        a = CryoAgg(ncols, 0, d_cols.ptr if d_cols else None)
        self._chk(self.L.cryo_codec_group_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, C.byref(f),
                                                C.byref(g), C.byref(a), d_blocks.ptr if d_blocks else None,
                                                d_groups.ptr if d_groups else None, group_cap, d_cells.ptr if d_cells else None,
                                                d_total.ptr if d_total else None), "group_batch")

    def group_blocks(self, method, comps, block_size, desc, gdesc, adesc=None, group_cap=None, buckets=None):
        """group host streams (desc: what filter_desc returns, gdesc: group_desc, adesc: agg_desc or None); returns (rows,
        records, cells, total): block i's groups are records[rows[i]["first_group"]:][:rows[i]["n_groups"]], cells has one row
        per group and one column per aggregate column; cell_sum gives a cell's 128-bit sum.  buckets: as for group_desc, for
        gdesc's columns.  A gdesc made with text=True returns the key cells as a fifth item (group_blocks_call)"""
        if buckets is not None:
            gdesc = group_desc([(int(c["att"]), int(c["type"])) for c in gdesc[1][:gdesc[0].nby]], buckets)
        return group_blocks_call(self.L.cryo_codec_group_blocks, self.h, self._chk, method, comps, block_size, desc, gdesc, adesc,
                                 group_cap)

    def project_batch(self, method, d_src, d_off, d_sizes, block_size, n, natts, d_atts, nkeys, d_keys, ncols, d_cols, d_rows,
                      row_cap, d_rec, rec_cap, d_blocks, d_total, truth=None):
        """test the keys on every tuple of the n stored blocks and copy the ncols fixed-width columns d_cols names (PROJECT_COL;
        d_keys: FILTER_KEY, d_atts: FILTER_ATT, device arrays) of every match into a row: one PROJECT_BLOCK row per block in
        d_blocks, one PROJECT_REC per match and per bad item in d_rec, one row of row_bytes per match in d_rows (at most row_cap
        rows and rec_cap records are written), the two totals {rows, records} in d_total (2 x u64).  truth: as for filter_batch.  Asynchronous once the
        descriptors are read back and the column table is in place."""
        f = CryoFilter(natts, nkeys, *truth_flags(0, truth), d_atts.ptr if d_atts else None, d_keys.ptr if d_keys else None)
        p = CryoProject(ncols, 0, d_cols.ptr if d_cols else None)
        self._chk(self.L.cryo_codec_project_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, C.byref(f),
                                                  C.byref(p), d_rows.ptr if d_rows else None, row_cap,
                                                  d_rec.ptr if d_rec else None, rec_cap, d_blocks.ptr if d_blocks else None,
                                                  d_total.ptr if d_total else None), "project_batch")

    def project_blocks(self, method, comps, block_size, desc, pdesc, row_bytes, rows=None, rec=None):
        """project host streams (desc: what filter_desc returns, pdesc: project_desc, row_bytes: project_row_layout's); returns
        (table, records, rows, (total rows, total records)): block i's records are records[table[i]["rec_first"]:][:n_match +
        n_bad], the row of its k-th match is rows[table[i]["row_first"] + k]"""
        return project_blocks_call(self.L.cryo_codec_project_blocks, self.h, self._chk, method, comps, block_size, desc, pdesc,
                                   row_bytes, rows, rec)

    def topn_batch(self, method, d_src, d_off, d_sizes, block_size, n, natts, d_atts, nkeys, d_keys, nby, limit, d_by, ncols, d_cols,
                   d_rows, d_rec, row_cap, d_blocks, d_total, truth=None):
        """test the keys on every tuple of the n stored blocks, rank each block's matches by the nby order columns d_by names
        (ORDER_COL) and keep the first `limit` of each block: one TOPN_BLOCK row per block in d_blocks, one TOPN_REC in d_rec and
        one row of row_bytes in d_rows per kept row (at most row_cap of each are written), in rank order, the total of kept rows
        in d_total (1 x u64).  d_atts, d_keys, d_cols, truth: as for project_batch.  Asynchronous once the descriptors are read
        back and the kernel's table is in place."""
        f = CryoFilter(natts, nkeys, *truth_flags(0, truth), d_atts.ptr if d_atts else None, d_keys.ptr if d_keys else None)
        o = CryoOrder(nby, limit, d_by.ptr if d_by else None)
        p = CryoProject(ncols, 0, d_cols.ptr if d_cols else None)
        self._chk(self.L.cryo_codec_topn_batch(self.h, method, d_src.ptr, d_off.ptr, d_sizes.ptr, block_size, n, C.byref(f), C.byref(o),
                                               C.byref(p), d_rows.ptr if d_rows else None, d_rec.ptr if d_rec else None, row_cap,
                                               d_blocks.ptr if d_blocks else None, d_total.ptr if d_total else None), "topn_batch")

    def topn_blocks(self, method, comps, block_size, desc, odesc, pdesc, row_bytes, rows=None, rec=None):
        """ordered scan of host streams (desc: what filter_desc returns, odesc: order_desc, pdesc: project_desc, row_bytes:
        project_row_layout's); returns (table, records, rows, total): block i's kept rows are records / rows
        [table[i]["row_first"]:][:table[i]["n_rows"]], in rank order"""
        return topn_blocks_call(self.L.cryo_codec_topn_blocks, self.h, self._chk, method, comps, block_size, desc, odesc, pdesc,
                                row_bytes, rows, rec)

    def last_verify_failure(self):
        """(block, first mismatch) that made the last host-buffer compress call fail verification, or None"""
        b, o = C.c_uint64(), C.c_uint32()
        r = self.L.cryo_codec_last_verify_failure(self.h, C.byref(b), C.byref(o))
        if r < 0:
            self._chk(r, "last_verify_failure")
        return (b.value, o.value) if r == 1 else None

    def checksum_batch(self, d_src, stride, n, d_sums, d_sizes=None, fixed_size=0):
        self._chk(self.L.cryo_codec_checksum_batch(self.h, d_src.ptr, stride, d_sizes.ptr if d_sizes else None,
                                                   fixed_size, n, d_sums.ptr), "checksum_batch")

    def compare_batch(self, d_a, a_stride, d_b, b_stride, block_size, n, d_mismatch):
        self._chk(self.L.cryo_codec_compare_batch(self.h, d_a.ptr, a_stride, d_b.ptr, b_stride, block_size, n,
                                                  d_mismatch.ptr), "compare_batch")

    # -- host convenience over batches: lists of numpy blocks in, lists out --
    def compress_blocks(self, method, param, blocks):
        """Compress equally sized host blocks as one device batch; returns list of uint8 arrays."""
        n = len(blocks)
        if n == 0:
            return []
        B = len(blocks[0])
        cap = bound(method, B)
        d_src, d_dst = self.alloc(n * B), self.alloc(n * cap)
        d_sizes, d_status = self.alloc(4 * n), self.alloc(4 * n)
        try:
            d_src.upload(np.concatenate([np.asarray(b, dtype=np.uint8) for b in blocks]))
            self.compress_batch(method, param, d_src, B, B, n, d_dst, cap, d_sizes, d_status)
            self.sync()
            st = d_status.download(dtype=np.int32)
            if (st != 0).any():
                raise CryoError(int(st[st != 0][0]), "compress_batch status")
            sizes = d_sizes.download(dtype=np.uint32)
            raw = d_dst.download()
            return [raw[i * cap:i * cap + int(sizes[i])].copy() for i in range(n)]
        finally:
            for b in (d_src, d_dst, d_sizes, d_status):
                b.free()

    def decompress_blocks(self, method, comps, block_size):
        """Decode host compressed blocks as one device batch; returns (list of arrays|None, statuses)."""
        n = len(comps)
        if n == 0:
            return [], np.zeros(0, np.int32)
        sizes = np.array([len(c) for c in comps], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        pos = 0
        for i, c in enumerate(comps):
            offs[i] = pos
            pos += (len(c) + 15) & ~15
        packed = np.zeros(max(pos, 16), dtype=np.uint8)
        for i, c in enumerate(comps):
            packed[int(offs[i]):int(offs[i]) + len(c)] = np.asarray(c, dtype=np.uint8)
        d_src, d_off, d_sizes = self.alloc(packed.nbytes), self.alloc(8 * n), self.alloc(4 * n)
        d_dst, d_status = self.alloc(n * block_size), self.alloc(4 * n)
        try:
            d_src.upload(packed)
            d_off.upload(offs)
            d_sizes.upload(sizes)
            d_dst.memset(0xA5)
            self.decompress_batch(method, d_src, d_off, d_sizes, d_dst, block_size, block_size, n, d_status)
            self.sync()
            st = d_status.download(dtype=np.int32)
            raw = d_dst.download()
            outs = [raw[i * block_size:(i + 1) * block_size].copy() if st[i] == 0 else None for i in range(n)]
            return outs, st
        finally:
            for b in (d_src, d_off, d_sizes, d_dst, d_status):
                b.free()

    # -- single block through the host-buffer entry points (what the PG shim calls) --
    def compress_block(self, method, param, block):
        a = np.ascontiguousarray(np.asarray(block, dtype=np.uint8))
        cap = bound(method, a.nbytes)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_size_t()
        self._chk(self.L.cryo_codec_compress_block(self.h, method, param, a.ctypes.data, a.nbytes,
                                                   out.ctypes.data, cap, C.byref(n)), "compress_block")
        return out[:n.value].copy()

    def decompress_block(self, method, comp, block_size):
        a = np.ascontiguousarray(np.asarray(comp, dtype=np.uint8))
        out = np.empty(block_size, dtype=np.uint8)
        rc = self.L.cryo_codec_decompress_block(self.h, method, a.ctypes.data, a.nbytes, out.ctypes.data, block_size)
        if rc == E_CORRUPT:
            return None
        self._chk(rc, "decompress_block")
        return out
