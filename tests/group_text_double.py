"""A codec double for the grouped scan's host walk (host/group.c) under CRYO_GROUP_TEXT: tests/group_double.py's, whose
group_blocks answers a descriptor that carries the flag from tests/group_text_ref.py -- records, then per group the aggregate
cells and the key cells, ncols + ntext cells of 40 bytes -- and every other descriptor as group_double does.  Test infrastructure
only."""
import ctypes as C

import numpy as np

import agg_ref as ar
import group_double
import group_text_ref as gt
from pg_cryogen_amd import codec

E_ARG, E_DSTSIZE = group_double.E_ARG, group_double.E_DSTSIZE


class TextGroupingDouble(group_double.GroupingDouble):
    def group_blocks(self, ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total):
        r = C.cast(group, C.POINTER(codec.CryoGroup)).contents
        if r.rsv != codec.GROUP_TEXT:
            return super().group_blocks(ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total)
        f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents if agg else None

        def arr(p, count, dtype):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (dtype.itemsize * count,)).view(dtype) if count else []

        atts = [(int(a["attlen"]), int(a["attalign"])) for a in arr(f.atts, f.natts, codec.FILTER_ATT)]
        keys = [(int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"])) for k in arr(f.keys, f.nkeys, codec.FILTER_KEY)]
        by = [(int(c["att"]), int(c["type"])) for c in arr(r.by, r.nby, codec.AGG_COL)]
        cols = None if g is None else [(int(c["att"]), int(c["type"])) for c in arr(g.cols, g.ncols, codec.AGG_COL)]
        if f.flags or f.rsv or (g and g.rsv) or not gt.desc_ok(atts, keys, by, cols, r.rsv):
            return E_ARG
        blocks = []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(ar.decode(self.base.ora, method, comp, bs))
        self.calls.append((method, n))
        ro, re, ce, tot, kc = gt.group_call(blocks, atts, keys, by, cols or [])
        total[0] = tot
        if tot > cap:
            return E_DSTSIZE
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        if tot:
            C.memmove(recs, re.ctypes.data, re.nbytes)
            parts = [np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).reshape(tot, 40 * x.shape[1]) for x in (ce, kc)]
            both = np.concatenate(parts, axis=1)                          # per group: the aggregate cells, then the key cells
            if both.shape[1]:
                if not cells:
                    return E_ARG
                both = np.ascontiguousarray(both)
                C.memmove(cells, both.ctypes.data, both.nbytes)
        return 0
