"""A codec double for the ordered scan's host walk (host/topn.c): the oracle double of tests/codec_double.py plus a topn table whose
topn_blocks decodes with the oracle and answers from tests/topn_ref.py.  Test infrastructure only."""
import ctypes as C

import numpy as np

import agg_ref as ar
import topn_ref as tr
from pg_cryogen_amd import codec, host

E_ARG, E_DSTSIZE = -1, -5


class OrderingDouble:
    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self.row_cap_limit = None      # a call that needs more rows than this answers CRYO_E_DSTSIZE (None: the caller's cap)
        self._topn = host.TOPN_BLOCKS_FN(self.topn_blocks)
        self.topn_ops = host.CryoCodecTopnOps(self._topn)

    def topn_blocks(self, ctx, method, srcs, sizes, n, bs, filt, order, project, rows, rec, row_cap, table, total):
        f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
        o = C.cast(order, C.POINTER(codec.CryoOrder)).contents
        p = C.cast(project, C.POINTER(codec.CryoProject)).contents

        def arr(ptr, count, dtype):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (dtype.itemsize * count,)).view(dtype) if count and ptr else []

        atts = [(int(a["attlen"]), int(a["attalign"])) for a in arr(f.atts, f.natts, codec.FILTER_ATT)]
        keys = [(int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"])) for k in arr(f.keys, f.nkeys, codec.FILTER_KEY)]
        oc = arr(o.by, o.nby, codec.ORDER_COL)
        by = [(int(c["att"]), int(c["type"]), int(c["flags"])) for c in oc]
        pc = arr(p.cols, p.ncols, codec.PROJECT_COL)
        cols = [int(c["att"]) for c in pc]
        if not tr.desc_ok(atts, keys, by, o.limit, cols, f.flags, f.rsv, p.rsv, [int(c["rsv"]) for c in pc], [int(c["rsv2"]) for c in pc],
                          by_rsv=[int(c["rsv"]) for c in oc]):
            return E_ARG
        blocks = []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(ar.decode(self.base.ora, method, comp, bs))
        self.calls.append((method, n, row_cap))
        t, recs, rws, tot = tr.topn_call(blocks, atts, keys, by, o.limit, cols)
        total[0] = tot
        cap = row_cap if self.row_cap_limit is None else min(row_cap, self.row_cap_limit)
        if tot > cap:
            return E_DSTSIZE
        C.memmove(table, t.ctypes.data, t.nbytes)
        if tot:
            rws = np.ascontiguousarray(rws)
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
            C.memmove(rows, rws.ctypes.data, rws.nbytes)
        return 0
