"""A codec double for the three host walks (host/filter.c, host/aggregate.c, host/group.c) that knows byte-string keys: the oracle
double of tests/codec_double.py plus a filter, an aggregate and a group table that decode with the oracle and answer from
tests/bytes_key_ref.py.  A CRYO_KEY_BYTES key arrives as the C ABI carries it -- rsv the length, value a host address -- and its
constant is read from that address.  Test infrastructure only."""
import ctypes as C

import numpy as np

import bytes_key_ref as br
from pg_cryogen_amd import codec, host

E_ARG, E_DSTSIZE = -1, -5


def _arr(p, count, dtype):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (dtype.itemsize * count,)).view(dtype) if count else []


def descriptor(filt):
    """(atts, keys with bytes for the constants, the keys' rsv fields, the struct) of a cryo_filter in host memory"""
    f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
    atts = [(int(a["attlen"]), int(a["attalign"])) for a in _arr(f.atts, f.natts, codec.FILTER_ATT)]
    keys, rsv = [], []
    for k in _arr(f.keys, f.nkeys, codec.FILTER_KEY):
        key = (int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"]))
        rsv.append(int(k["rsv"]))
        if br.is_bytes_key(key):
            n, at = int(k["rsv"]), int(k["value"])
            key = key[:3] + (None if n and not at else C.string_at(at, n) if n <= br.BYTES_MAX and n else b"",)
        keys.append(key)
    return atts, keys, rsv, f


def _cols(p, count):
    return [(int(c["att"]), int(c["type"])) for c in _arr(p, count, codec.AGG_COL)]


def _cols_ok(atts, cols):
    return all(1 <= a <= len(atts) and t in br.KEY_SIZE and atts[a - 1][0] == br.KEY_SIZE[t] and atts[a - 1][1] >= br.KEY_SIZE[t]
               for a, t in cols)


class BytesKeyDouble:
    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self._filter = host.FILTER_BLOCKS_FN(self.filter_blocks)
        self.filter_ops = host.CryoCodecFilterOps(self._filter)
        self._agg = host.AGG_BLOCKS_FN(self.agg_blocks)
        self.agg_ops = host.CryoCodecAggOps(self._agg)
        self._group = host.GROUP_BLOCKS_FN(self.group_blocks)
        self.group_ops = host.CryoCodecGroupOps(self._group)

    def _decode(self, what, method, srcs, sizes, n, bs):
        self.calls.append((what, method, n))
        return [br.decode(self.base.ora, method, np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy(), bs)
                for i in range(n)]

    def filter_blocks(self, ctx, method, srcs, sizes, n, bs, filt, dst, dst_cap, rec, rec_cap, rows, total):
        atts, keys, rsv, f = descriptor(filt)
        if not br.desc_ok(atts, keys, f.flags, f.rsv, rsv):
            return E_ARG
        table, recs, packed, (tb, tr) = br.filter_call(self._decode("filter", method, srcs, sizes, n, bs), atts, keys, f.flags)
        if tb > dst_cap or tr > rec_cap:
            return E_DSTSIZE
        if tb:
            C.memmove(dst, packed.ctypes.data, tb)
        if tr:
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
        C.memmove(rows, table.ctypes.data, table.nbytes)
        total[0], total[1] = tb, tr
        return 0

    def agg_blocks(self, ctx, method, srcs, sizes, n, bs, filt, agg, rows, cells):
        atts, keys, rsv, f = descriptor(filt)
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents
        cols = _cols(g.cols, g.ncols)
        if not br.desc_ok(atts, keys, f.flags, f.rsv, rsv) or f.flags or g.rsv or not 1 <= len(cols) <= 4 or not _cols_ok(atts, cols):
            return E_ARG
        ro, ce = br.agg_call(self._decode("agg", method, srcs, sizes, n, bs), atts, keys, cols)
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0

    def group_blocks(self, ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total):
        atts, keys, rsv, f = descriptor(filt)
        r = C.cast(group, C.POINTER(codec.CryoGroup)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents if agg else None
        by, cols = _cols(r.by, r.nby), _cols(g.cols, g.ncols) if g else []
        if (not br.desc_ok(atts, keys, f.flags, f.rsv, rsv) or f.flags or r.rsv or (g and g.rsv) or not 1 <= len(by) <= 2 or
                len(cols) > 4 or not _cols_ok(atts, by + cols)):
            return E_ARG
        ro, re, ce, tot = br.group_call(self._decode("group", method, srcs, sizes, n, bs), atts, keys, by, cols)
        total[0] = tot
        if tot > cap:
            return E_DSTSIZE
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        if tot:
            C.memmove(recs, re.ctypes.data, re.nbytes)
            if cols:
                C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0
