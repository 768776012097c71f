"""A codec double for the four host walks (host/filter.c, host/aggregate.c, host/group.c, host/project.c) that knows float keys and
float aggregate columns: tests/set_key_double.py's double, answering from tests/float_ref.py.  A float key arrives as the C ABI
carries it -- value the 64 bits of a double -- and a truth table in the descriptor's rsv.  Test infrastructure only."""
import ctypes as C

import numpy as np

import float_ref as fl
from bytes_key_double import _arr, _cols
from pg_cryogen_amd import codec
from set_key_double import E_ARG, E_DSTSIZE, SetKeyDouble, descriptor


def _truth(f):
    return f.rsv if f.flags & fl.tr.TRUTH else None


class FloatDouble(SetKeyDouble):
    def filter_blocks(self, ctx, method, srcs, sizes, n, bs, filt, dst, dst_cap, rec, rec_cap, rows, total):
        atts, keys, rsv, f = descriptor(filt)
        if not fl.desc_ok(atts, keys, f.flags, f.rsv, rsv):
            return E_ARG
        table, recs, packed, (tb, tr) = fl.filter_call(self._decode("filter", method, srcs, sizes, n, bs, keys), atts, keys, f.flags, _truth(f))
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
        if (not fl.desc_ok(atts, keys, f.flags, f.rsv, rsv) or f.flags & ~fl.tr.TRUTH or g.rsv or not 1 <= len(cols) <= 4 or
                not all(fl.col_ok(atts, c) for c in cols)):
            return E_ARG
        ro, ce = fl.agg_call(self._decode("agg", method, srcs, sizes, n, bs, keys), atts, keys, cols, _truth(f))
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0

    def group_blocks(self, ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total):
        atts, keys, rsv, f = descriptor(filt)
        r = C.cast(group, C.POINTER(codec.CryoGroup)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents if agg else None
        by, cols = _cols(r.by, r.nby), _cols(g.cols, g.ncols) if g else []
        if (not fl.desc_ok(atts, keys, f.flags, f.rsv, rsv) or f.flags & ~fl.tr.TRUTH or r.rsv or (g and g.rsv) or not 1 <= len(by) <= 2 or
                len(cols) > 4 or not all(fl.col_ok(atts, c, True) for c in by) or not all(fl.col_ok(atts, c) for c in cols)):
            return E_ARG
        ro, re, ce, tot = fl.group_call(self._decode("group", method, srcs, sizes, n, bs, keys), atts, keys, by, cols, _truth(f))
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
        plain = [(1, 0, fl.NOTNULL, 0)] * len(keys)                    # the projection's own rules, the keys' checked apart
        if (not fl.desc_ok(atts, keys, f.flags, f.rsv, rsv) or
                not fl.sr.pr.desc_ok(atts, plain, cols, 0, 0, p.rsv, [int(c["rsv"]) for c in pc], [int(c["rsv2"]) for c in pc])):
            return E_ARG
        t, recs, rws, (tw, tr) = fl.project_call(self._decode("project", method, srcs, sizes, n, bs, keys), atts, keys, cols, _truth(f))
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
