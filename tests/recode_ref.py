"""The packing rules of recompression (include/cryo_codec.h, cryo_codec_recode_blocks / cryo_multi_recode_blocks) restated in
Python, for the CPU and GPU tests and the codec double.  Test infrastructure only."""
import numpy as np

import multi_ref


def align16(x):
    return (int(x) + 15) & ~15


def pack_offsets(sizes, statuses, base=0):
    """(sizes, offsets, total): a block whose status is not 0 has size 0 and takes no room; offsets[0] = base,
    offsets[i + 1] = offsets[i] + align16(sizes[i])"""
    sizes = [int(s) if int(st) == 0 else 0 for s, st in zip(sizes, statuses)]
    offs, pos = [], int(base)
    for s in sizes:
        offs.append(pos)
        pos += align16(s)
    return sizes, offs, pos - int(base)


def multi_offsets(sizes, statuses, G, dst_cap):
    """block i -> handle i mod G; handle g packs its share, in block order, from g * region on, region = dst_cap // G
    rounded down to 16 bytes"""
    return multi_ref.offsets_multi(pack_offsets, sizes, statuses, G, dst_cap)


def pack_buffer(streams, statuses, dst, base=0):
    """write streams by the rule into dst (a uint8 array); pad bytes zero; returns (sizes, offsets, total)"""
    sizes, offs, total = pack_offsets([0 if s is None else len(s) for s in streams], statuses, base)
    for s, sz, o in zip(streams, sizes, offs):
        if sz:
            dst[o:o + sz] = np.asarray(s, np.uint8)
            dst[o + sz:o + align16(sz)] = 0
    return sizes, offs, total
