"""A codec double for the grouped scan's host walk (host/group.c): the oracle double of tests/codec_double.py plus a group table
whose group_blocks decodes with the oracle and answers from tests/group_ref.py.  Test infrastructure only."""
import ctypes as C

import numpy as np

import agg_ref as ar
import group_ref as gr
from pg_cryogen_amd import codec, host

E_ARG, E_DSTSIZE = -1, -5


class GroupingDouble:
    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self._group = host.GROUP_BLOCKS_FN(self.group_blocks)
        self.group_ops = host.CryoCodecGroupOps(self._group)

    def group_blocks(self, ctx, method, srcs, sizes, n, bs, filt, group, agg, rows, recs, cap, cells, total):
        f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
        r = C.cast(group, C.POINTER(codec.CryoGroup)).contents
        g = C.cast(agg, C.POINTER(codec.CryoAgg)).contents if agg else None

        def arr(p, count, dtype):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (dtype.itemsize * count,)).view(dtype) if count else []

        atts = [(int(a["attlen"]), int(a["attalign"])) for a in arr(f.atts, f.natts, codec.FILTER_ATT)]
        keys = [(int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"])) for k in arr(f.keys, f.nkeys, codec.FILTER_KEY)]
        by = [(int(c["att"]), int(c["type"])) for c in arr(r.by, r.nby, codec.AGG_COL)]
        cols = None if g is None else [(int(c["att"]), int(c["type"])) for c in arr(g.cols, g.ncols, codec.AGG_COL)]
        if not gr.desc_ok(atts, keys, by, cols, f.flags, f.rsv, r.rsv, None, g.rsv if g else 0):
            return E_ARG
        blocks = []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(ar.decode(self.base.ora, method, comp, bs))
        self.calls.append((method, n))
        ro, re, ce, tot = gr.group_call(blocks, atts, keys, by, cols or [])
        total[0] = tot
        if tot > cap:
            return E_DSTSIZE
        C.memmove(rows, ro.ctypes.data, ro.nbytes)
        if tot:
            C.memmove(recs, re.ctypes.data, re.nbytes)
            if cols:
                C.memmove(cells, np.ascontiguousarray(ce).ctypes.data, ce.nbytes)
        return 0
