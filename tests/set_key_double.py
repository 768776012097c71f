"""A codec double for the four host walks (host/filter.c, host/aggregate.c, host/group.c, host/project.c) that knows set keys: the
oracle double of tests/codec_double.py plus a filter, an aggregate, a group and a project table that decode with the oracle and
answer from tests/set_key_ref.py.  A set key arrives as the C ABI carries it -- rsv the number of members, value a host address
of that many int64 -- and its list is read from that address; a byte-string constant likewise.  Test infrastructure only."""
import ctypes as C

import numpy as np

import set_key_ref as sr
from bytes_key_double import _arr, _cols, _cols_ok
from pg_cryogen_amd import codec, host

E_ARG, E_DSTSIZE = -1, -5


def descriptor(filt):
    """(atts, keys with lists and bytes for their values, the keys' rsv fields, the struct) of a cryo_filter in host memory"""
    f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
    atts = [(int(a["attlen"]), int(a["attalign"])) for a in _arr(f.atts, f.natts, codec.FILTER_ATT)]
    keys, rsv = [], []
    for k in _arr(f.keys, f.nkeys, codec.FILTER_KEY):
        key = (int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"]))
        n, at = int(k["rsv"]), int(k["value"])
        rsv.append(n)
        if sr.is_set_key(key):
            readable = at and 1 <= n <= sr.SET_MAX
            key = key[:3] + (np.frombuffer(C.string_at(at, 8 * n), "<i8").tolist() if readable else [] if at else None,)
        elif sr.br.is_bytes_key(key):
            key = key[:3] + (None if n and not at else C.string_at(at, n) if n <= sr.BYTES_MAX and n else b"",)
        keys.append(key)
    return atts, keys, rsv, f


class SetKeyDouble:
    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self.keys_seen = []                                            # the keys of every call, as read from the ABI
        self._filter = host.FILTER_BLOCKS_FN(self.filter_blocks)
        self.filter_ops = host.CryoCodecFilterOps(self._filter)
        self._agg = host.AGG_BLOCKS_FN(self.agg_blocks)
        self.agg_ops = host.CryoCodecAggOps(self._agg)
        self._group = host.GROUP_BLOCKS_FN(self.group_blocks)
        self.group_ops = host.CryoCodecGroupOps(self._group)
        self._project = host.PROJECT_BLOCKS_FN(self.project_blocks)
        self.project_ops = host.CryoCodecProjectOps(self._project)

    def _decode(self, what, method, srcs, sizes, n, bs, keys):
        self.calls.append((what, method, n))
        self.keys_seen.append(keys)
        return [sr.decode(self.base.ora, method, np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy(), bs)
                for i in range(n)]

    def filter_blocks(self, ctx, method, srcs, sizes, n, bs, filt, dst, dst_cap, rec, rec_cap, rows, total):
        atts, keys, rsv, f = descriptor(filt)
        if not sr.desc_ok(atts, keys, f.flags, f.rsv, rsv):
            return E_ARG
        table, recs, packed, (tb, tr) = sr.filter_call(self._decode("filter", method, srcs, sizes, n, bs, keys), atts, keys, f.flags)
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
        if not sr.desc_ok(atts, keys, f.flags, f.rsv, rsv) or f.flags or g.rsv or not 1 <= len(cols) <= 4 or not _cols_ok(atts, cols):
            return E_ARG
        ro, ce = sr.agg_call(self._decode("agg", method, srcs, sizes, n, bs, keys), atts, keys, cols)
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0

    def group_blocks(self, ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total):
        atts, keys, rsv, f = descriptor(filt)
        r = C.cast(group, C.POINTER(codec.CryoGroup)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents if agg else None
        by, cols = _cols(r.by, r.nby), _cols(g.cols, g.ncols) if g else []
        if (not sr.desc_ok(atts, keys, f.flags, f.rsv, rsv) or f.flags or r.rsv or (g and g.rsv) or not 1 <= len(by) <= 2 or
                len(cols) > 4 or not _cols_ok(atts, by + cols)):
            return E_ARG
        ro, re, ce, tot = sr.group_call(self._decode("group", method, srcs, sizes, n, bs, keys), atts, keys, by, cols)
        total[0] = tot
        if tot > cap:
            return E_DSTSIZE
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        if tot:
            C.memmove(recs, re.ctypes.data, re.nbytes)
            if cols:
                C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0

    def project_blocks(self, ctx, method, srcs, sizes, n, bs, filt, project, rows, row_cap, rec, rec_cap, table, total):
        atts, keys, rsv, f = descriptor(filt)
        p = C.cast(project, C.POINTER(codec.CryoProject)).contents
        pc = _arr(p.cols, p.ncols, codec.PROJECT_COL)
        cols = [int(c["att"]) for c in pc]
        plain = [(1, 0, sr.NOTNULL, 0)] * len(keys)                    # the projection's own rules, the keys' checked apart
        if (not sr.desc_ok(atts, keys, f.flags, f.rsv, rsv) or
                not sr.pr.desc_ok(atts, plain, cols, f.flags, f.rsv, p.rsv, [int(c["rsv"]) for c in pc], [int(c["rsv2"]) for c in pc])):
            return E_ARG
        t, recs, rws, (tw, tr) = sr.project_call(self._decode("project", method, srcs, sizes, n, bs, keys), atts, keys, cols)
        total[0], total[1] = tw, tr
        if tw > row_cap or tr > rec_cap:
            return E_DSTSIZE
        C.memmove(table, t.ctypes.data, t.nbytes)
        if tr:
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
        if tw:
            rws = np.ascontiguousarray(rws)
            C.memmove(rows, rws.ctypes.data, rws.nbytes)
        return 0
