"""A codec double for the projecting scan's host walk (host/project.c): the oracle double of tests/codec_double.py plus a project
table whose project_blocks decodes with the oracle and answers from tests/project_ref.py.  Test infrastructure only."""
import ctypes as C

import numpy as np

import agg_ref as ar
import project_ref as pr
from pg_cryogen_amd import codec, host

E_ARG, E_DSTSIZE = -1, -5


class ProjectingDouble:
    def __init__(self):
        import codec_double
        self.base = codec_double.OracleCodecOps()
        self.calls = []
        self.row_cap_limit = None      # a call that needs more rows than this answers CRYO_E_DSTSIZE (None: the caller's cap)
        self._project = host.PROJECT_BLOCKS_FN(self.project_blocks)
        self.project_ops = host.CryoCodecProjectOps(self._project)

    def project_blocks(self, ctx, method, srcs, sizes, n, bs, filt, project, rows, row_cap, rec, rec_cap, table, total):
        f = C.cast(filt, C.POINTER(codec.CryoFilter)).contents
        p = C.cast(project, C.POINTER(codec.CryoProject)).contents

        def arr(ptr, count, dtype):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (dtype.itemsize * count,)).view(dtype) if count else []

        atts = [(int(a["attlen"]), int(a["attalign"])) for a in arr(f.atts, f.natts, codec.FILTER_ATT)]
        keys = [(int(k["att"]), int(k["type"]), int(k["op"]), int(k["value"])) for k in arr(f.keys, f.nkeys, codec.FILTER_KEY)]
        pc = arr(p.cols, p.ncols, codec.PROJECT_COL)
        cols = [int(c["att"]) for c in pc]
        if not pr.desc_ok(atts, keys, cols, f.flags, f.rsv, p.rsv, [int(c["rsv"]) for c in pc], [int(c["rsv2"]) for c in pc]):
            return E_ARG
        blocks = []
        for i in range(n):
            comp = np.ctypeslib.as_array(C.cast(srcs[i], C.POINTER(C.c_uint8)), (sizes[i],)).copy()
            blocks.append(ar.decode(self.base.ora, method, comp, bs))
        self.calls.append((method, n))
        t, recs, rws, (tw, tr) = pr.project_call(blocks, atts, keys, cols)
        total[0], total[1] = tw, tr
        cap = row_cap if self.row_cap_limit is None else min(row_cap, self.row_cap_limit)
        if tw > cap or tr > rec_cap:
            return E_DSTSIZE
        C.memmove(table, t.ctypes.data, t.nbytes)
        if tr:
            C.memmove(rec, recs.ctypes.data, recs.nbytes)
        if tw:
            rws = np.ascontiguousarray(rws)
            C.memmove(rows, rws.ctypes.data, rws.nbytes)
        return 0
