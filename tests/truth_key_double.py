"""A codec double for the four host walks (host/filter.c, host/aggregate.c, host/group.c, host/project.c) that knows the truth
table: tests/set_key_double.py's double, answering from tests/truth_key_ref.py.  The descriptor arrives as the C ABI carries it;
flags and rsv of every call are kept as read from the struct, so that a test can hold them against what the caller set.  Test
infrastructure only."""
import ctypes as C

import numpy as np

import truth_key_ref as tr
from bytes_key_double import _arr, _cols, _cols_ok
from pg_cryogen_amd import codec
from set_key_double import E_ARG, E_DSTSIZE, SetKeyDouble, descriptor


class TruthKeyDouble(SetKeyDouble):
    def __init__(self):
        super().__init__()
        self.words_seen = []                                           # (what, flags, rsv) of every call, as read from the ABI

    def _desc(self, what, filt):
        atts, keys, rsv, f = descriptor(filt)
        self.words_seen.append((what, int(f.flags), int(f.rsv)))
        ok = tr.desc_ok(atts, keys, f.flags, f.rsv, rsv) and (what == "filter" or tr.reduce_flags_ok(f.flags))
        return ok, atts, keys, f.flags, f.rsv if f.flags & tr.TRUTH else None

    def filter_blocks(self, ctx, method, srcs, sizes, n, bs, filt, dst, dst_cap, rec, rec_cap, rows, total):
        ok, atts, keys, flags, truth = self._desc("filter", filt)
        if not ok:
            return E_ARG
        table, recs, packed, (tb, tr_) = tr.filter_call(self._decode("filter", method, srcs, sizes, n, bs, keys), atts, keys, flags, truth)
        if tb > dst_cap or tr_ > rec_cap:
            return E_DSTSIZE
        if tb:
            C.memmove(dst, packed.ctypes.data, tb)
        if tr_:
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
        C.memmove(rows, table.ctypes.data, table.nbytes)
        total[0], total[1] = tb, tr_
        return 0

    def agg_blocks(self, ctx, method, srcs, sizes, n, bs, filt, agg, rows, cells):
        ok, atts, keys, flags, truth = self._desc("agg", filt)
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents
        cols = _cols(g.cols, g.ncols)
        if not ok or g.rsv or not 1 <= len(cols) <= 4 or not _cols_ok(atts, cols):
            return E_ARG
        ro, ce = tr.agg_call(self._decode("agg", method, srcs, sizes, n, bs, keys), atts, keys, cols, truth)
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0

    def group_blocks(self, ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total):
        ok, atts, keys, flags, truth = self._desc("group", filt)
        r = C.cast(group, C.POINTER(codec.CryoGroup)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents if agg else None
        by, cols = _cols(r.by, r.nby), _cols(g.cols, g.ncols) if g else []
        if not ok or r.rsv or (g and g.rsv) or not 1 <= len(by) <= 2 or len(cols) > 4 or not _cols_ok(atts, by + cols):
            return E_ARG
        ro, re, ce, tot = tr.group_call(self._decode("group", method, srcs, sizes, n, bs, keys), atts, keys, by, cols, truth)
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
        ok, atts, keys, flags, truth = self._desc("project", filt)
        p = C.cast(project, C.POINTER(codec.CryoProject)).contents
        pc = _arr(p.cols, p.ncols, codec.PROJECT_COL)
        cols = [int(c["att"]) for c in pc]
        plain = [(1, 0, tr.NOTNULL, 0)] * len(keys)                    # the projection's own rules, the keys' checked apart
        if not ok or not tr.sr.pr.desc_ok(atts, plain, cols, 0, 0, p.rsv, [int(c["rsv"]) for c in pc], [int(c["rsv2"]) for c in pc]):
            return E_ARG
        t, recs, rws, (tw, tr_) = tr.project_call(self._decode("project", method, srcs, sizes, n, bs, keys), atts, keys, cols, truth)
        total[0], total[1] = tw, tr_
        if tw > row_cap or tr_ > rec_cap:
            return E_DSTSIZE
        C.memmove(table, t.ctypes.data, t.nbytes)
        if tr_:
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
        if tw:
            rws = np.ascontiguousarray(rws)
            C.memmove(rows, rws.ctypes.data, rws.nbytes)
        return 0
