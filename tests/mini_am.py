"""Mini-AM helpers of the stored-block check tests: rows packed into cryo blocks by the host library's own
cryo_init_page / cryo_storage_insert, and a small relation written through its page-chain staging.  Test infrastructure
only."""
import ctypes as C
import struct

from pg_cryogen_amd import host


def heap_tuple(payload, natts):
    """23-byte HeapTupleHeader (t_hoff = 24) + user data"""
    hdr = bytearray(24)
    struct.pack_into("<H", hdr, 18, natts)
    struct.pack_into("<H", hdr, 20, 0x0800)
    hdr[22] = 24
    return bytes(hdr) + payload


def pack_rows(L, rows, natts, bs):
    """the multi_insert loop of reference pg_cryogen.c:633-662: insert until the block is full, then start a new one"""
    blocks = []
    buf = (C.c_uint8 * bs)()
    L.cryo_init_page(buf)
    for payload in rows:
        t = heap_tuple(payload, natts)
        tb = C.create_string_buffer(t, len(t))
        ht = host.HeapTupleData(len(t), C.cast(tb, C.c_void_p))
        if L.cryo_storage_insert(buf, C.byref(ht)) == -1:
            blocks.append(bytes(buf))
            L.cryo_init_page(buf)
            assert L.cryo_storage_insert(buf, C.byref(ht)) == 1
    blocks.append(bytes(buf))
    return blocks


def load_relation(L, rows, natts, method, relid=4242, batch=8, xid=777):
    """an in-memory relation holding `rows`: blocks of host.get_block_size() bytes written by the write-behind staging
    (cryo_stage_write_batch, the bound codec compresses); returns (memrel, CryoRel, blocks, first pages)"""
    mem = L.cryo_memrel_create()
    rel = host.CryoRel()
    L.cryo_memrel_bind(mem, relid, C.byref(rel))
    blocks = pack_rows(L, rows, natts, host.get_block_size())
    firsts = []
    for i in range(0, len(blocks), batch):
        chunk = blocks[i:i + batch]
        fb = (C.c_uint32 * len(chunk))(*[L.cryo_memrel_reserve(mem) for _ in chunk])
        assert L.cryo_stage_write_batch(C.byref(rel), b"".join(chunk), len(chunk), method, xid, fb) == 0
        firsts += list(fb)
    return mem, rel, blocks, firsts
