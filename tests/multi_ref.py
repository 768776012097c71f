"""The deal and the region bookkeeping of the cryo_multi_* calls (include/cryo_codec.h; pg_cryogen_amd/csrc/multi_share.h in the
library), stated once for the references: block i -> handle i mod G; a handle's region starts (blocks of the handles before it) x
(units per block) in; a total is the end of the last unit any handle used.  Each *_multi takes the single-handle reference of the
module that calls it.  Test infrastructure only."""
import numpy as np

MAX_ITEMS = 290


def shares(n, G):
    """[(g, block indices of handle g, blocks of the handles before g)] for every handle with a share"""
    out, before = [], 0
    for g in range(min(G, n)):
        idx = list(range(g, n, G))
        out.append((g, idx, before))
        before += len(idx)
    return out


def share_regions(n, G, units, single):
    """the per-handle loop: single(idx, bases) -> (what the share gave, its totals), bases[j] = before x units[j] the start of the
    share's j-th region and totals[j] what it used of it.  Returns ([(idx, bases, what the share gave)] per handle with a share,
    [the end of the last unit used of the j-th regions, 0: none])"""
    out, ends = [], [0] * len(units)
    for _, idx, before in shares(n, G):
        bases = [before * u for u in units]
        result, totals = single(idx, bases)
        out.append((idx, bases, result))
        ends = [max(e, b + t) if t else e for e, b, t in zip(ends, bases, totals)]
    return out, ends


def _scan_multi(single, table_dtype, blocks, G, units):
    """single(share's blocks, base a, base b) -> (table, records, packed, (total a, total b)): (table in call order, [((base a,
    base b), records, packed)] per handle with a share, (end a, end b))"""
    table = np.zeros(len(blocks), table_dtype)

    def one(idx, bases):
        t, recs, packed, totals = single([blocks[i] for i in idx], *bases)
        table[idx] = t
        return (recs, packed), totals
    out, ends = share_regions(len(blocks), G, units, one)
    return table, [(bases, recs, packed) for _, bases, (recs, packed) in out], tuple(ends)


def filter_multi(filter_call, table_dtype, blocks, atts, keys, G, B, flags=0):
    """what cryo_multi_filter_blocks with G handles gives: handle g has a tuple region of B x (its blocks) bytes and a record
    region of 290 x (its blocks) records, in handle order.  Returns (table in call order, [(byte start, packed bytes, record
    start, records)] per handle with a share, (end of the last byte, of the last record used))"""
    table, regions, ends = _scan_multi(lambda bl, b0, r0: filter_call(bl, atts, keys, flags, b0, r0), table_dtype, blocks, G,
                                       (B, MAX_ITEMS))
    return table, [(b0, packed, r0, recs) for (b0, r0), recs, packed in regions], ends


def project_multi(project_call, table_dtype, blocks, atts, keys, cols, G):
    """what cryo_multi_project_blocks with G handles gives: handle g has a row region and a record region of 290 x (its blocks)
    entries each, in handle order.  Returns (table in call order, [(first entry of both regions, rows, records)] per handle with
    a share, (end of the last row, of the last record used))"""
    table, regions, ends = _scan_multi(lambda bl, w0, r0: project_call(bl, atts, keys, cols, w0, r0), table_dtype, blocks, G,
                                       (MAX_ITEMS, MAX_ITEMS))
    return table, [(w0, rows, recs) for (w0, _), recs, rows in regions], ends


def fetch_multi(fetch_call, result_dtype, blocks, requests, G, B):
    """what cryo_multi_fetch_blocks with G handles gives: handle g packs its share into a region of B x (its blocks) bytes, the
    regions in handle order.  Returns (records in call order, [(region start, packed bytes)] per handle with a share, total: the
    end of the last byte used)"""
    first = np.concatenate([[0], np.cumsum([len(r) for r in requests])]).astype(int)
    records = np.zeros(int(first[-1]), result_dtype)

    def one(idx, bases):
        recs, packed, tot = fetch_call([blocks[i] for i in idx], [requests[i] for i in idx], base=bases[0])
        at = 0
        for i in idx:
            k = len(requests[i])
            records[first[i]:first[i] + k] = recs[at:at + k]
            at += k
        return packed, [tot]
    out, ends = share_regions(len(blocks), G, (B,), one)
    return records, [(bases[0], packed) for _, bases, packed in out], ends[0]


def offsets_multi(pack_offsets, sizes, statuses, G, dst_cap):
    """what cryo_multi_recode_blocks with G handles gives: handle g packs its share, in block order, from g x region on, region =
    dst_cap // G rounded down to 16 bytes.  Returns (sizes, offsets, region)"""
    region = (int(dst_cap) // G) & ~15
    out_s, out_o = [0] * len(sizes), [0] * len(sizes)
    for g, idx, _ in shares(len(sizes), G):
        s, o, _ = pack_offsets([sizes[i] for i in idx], [statuses[i] for i in idx], g * region)
        for k, i in enumerate(idx):
            out_s[i], out_o[i] = s[k], o[k]
    return out_s, out_o, region
