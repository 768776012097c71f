"""Hand-built Zstandard frames for format corners libzstd's own encoder never emits (test infrastructure).

huf12_frame(): one compressed block whose literals use a Huffman table of log 12 (RFC 8878 4.2.1 allows
up to 12; libzstd's encoder stops at 11), direct 4-bit weights, 1 or 4 streams, no sequences.  The
decoders take a different path for such tables (two-level lookup in the batch pipeline).

walk(): the structure of a frame (header flags, window, blocks, literal section types, sequence-table modes).
zstd_corpus(): frames libzstd writes only with non-default parameters (ZSTD_compress2): content checksums and broken
copies of them, small windows, no content size, forced literal modes, minMatch 3, long-distance matching,
targetCBlockSize, blocks of few sequences, and mutations of them.

tests/zstd_asm.py assembles whole frames from a description (sequences, table modes, headers) and shares huf_codes()."""
import numpy as np

# 13 listed weights + 1 implied: 3 x 2^10 + 2^9 + ... + 2^0 + 2^0 = 4096 -> table log 12, code lengths 2..12
WEIGHTS = [11, 11, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]  # symbol 13's weight is implied by the others
LOG = 12


def huf_codes(weights):
    """canonical codes as the decoder assigns them (RFC 8878 4.2.1): weights ascending, symbols ascending inside a weight.
    weights holds every symbol's, the implied last one included.  -> ({symbol: (value, nbits)}, table log)"""
    total = sum((1 << w) >> 1 for w in weights)
    log = total.bit_length() - 1
    assert total == 1 << log, weights
    codes, nxt = {}, 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                span = 1 << (w - 1)
                codes[s] = (nxt // span, log + 1 - w)
                nxt += span
    assert nxt == 1 << log
    return codes, log


def _codes():
    codes, log = huf_codes(WEIGHTS)
    assert log == LOG
    return codes


def _stream(symbols, codes):
    acc, n = 0, 0
    for s in reversed(symbols):          # the decoder reads backwards: the first symbol sits on top
        v, nb = codes[int(s)]
        acc |= v << n
        n += nb
    acc |= 1 << n                        # end mark
    return acc.to_bytes((n + 8) // 8, "little")


def huf12_frame(n=700, streams=4, seed=1):
    rng = np.random.default_rng(seed)
    p = np.array([2.0 ** -(LOG + 1 - w) for w in WEIGHTS])
    lits = rng.choice(len(WEIGHTS), size=n, p=p / p.sum()).astype(np.uint8)
    lits[:14] = np.arange(14)            # every code, incl. both 12-bit ones, at least once
    codes = _codes()
    nw = len(WEIGHTS) - 1
    tree = bytes([127 + nw]) + bytes(((WEIGHTS[i] << 4) | (WEIGHTS[i + 1] if i + 1 < nw else 0)) for i in range(0, nw, 2))
    if streams == 1:
        body, fmt = _stream(lits, codes), 0
    else:
        seg = (n + 3) // 4
        parts = [_stream(lits[i * seg:(i + 1) * seg], codes) for i in range(4)]
        jump = b"".join(len(q).to_bytes(2, "little") for q in parts[:3])
        body, fmt = jump + b"".join(parts), 1
    csize = len(tree) + len(body)
    assert n < 1024 and csize < 1024
    lit_hdr = (2 | (fmt << 2) | (n << 4) | (csize << 14)).to_bytes(3, "little")
    block = lit_hdr + tree + body + b"\x00"          # literals, then "0 sequences"
    bh = ((len(block) << 3) | (2 << 1) | 1).to_bytes(3, "little")
    assert n >= 256
    frame = (0xFD2FB528).to_bytes(4, "little") + bytes([0x60]) + (n - 256).to_bytes(2, "little") + bh + block
    return np.frombuffer(frame, np.uint8).copy(), lits


# ---------------- a structural walker and a corpus of non-default frames (libzstd 1.4.8 through ZSTD_compress2) ----------------
MODES = ("predefined", "rle", "fse", "repeat")
LIT_TYPES = ("raw", "rle", "compressed", "treeless")


def walk(frame):
    """frame header, block headers, literal section type and the three sequence-table modes of one frame (RFC 8878 3.1.1,
    no entropy decoding: a literal section states its own size).  Returns a dict, or None where the structure is broken."""
    b = bytes(frame)
    if len(b) < 6 or int.from_bytes(b[:4], "little") != 0xFD2FB528:
        return None
    fhd = b[4]
    fcs_flag, single, checksum, did = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    info = {"checksum": bool(checksum), "content_size": bool(fcs_flag or single),
            "window_log": None if single or p > len(b) else 10 + (b[5] >> 3), "blocks": []}
    while True:
        if p + 3 > len(b):
            return None
        h = int.from_bytes(b[p:p + 3], "little")
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        p += 3
        blk = {"type": ("raw", "rle", "compressed", "reserved")[btype], "size": bsize}
        if btype == 2:
            blk.update(_walk_block(b[p:p + bsize]) or {"broken": True})
        p += 1 if btype == 1 else bsize
        info["blocks"].append(blk)
        if last:
            break
    info["end"] = p + 4 * checksum
    return info if info["end"] <= len(b) else None


def _walk_block(b):
    if not b:
        return None
    b0 = b[0]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt < 2:
        hl = (1, 2, 1, 3)[sf]
        size = b0 >> 3 if hl == 1 else (int.from_bytes(b[:hl], "little") >> 4)
        p = hl + (size if lt == 0 else 1)
    else:
        hl, bits = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
        h = int.from_bytes(b[:hl], "little")
        p = hl + ((h >> (4 + bits)) & ((1 << bits) - 1))
    if p >= len(b):
        return None
    s0 = b[p]
    nseq, q = (s0, p + 1) if s0 < 128 else ((((s0 - 128) << 8) + b[p + 1], p + 2) if s0 < 255 else
                                            (b[p + 1] + (b[p + 2] << 8) + 0x7F00, p + 3))
    out = {"lit": LIT_TYPES[lt], "nseq": nseq, "modes": None}
    if nseq:
        if q >= len(b):
            return None
        m = b[q]
        out["modes"] = (MODES[m >> 6], MODES[(m >> 4) & 3], MODES[(m >> 2) & 3])   # LL, OF, ML
    return out


def walk_entropy(frame):
    """walk() with the entropy stage's header fields on every compressed block (header reading, no entropy decoding):
        lit          raw | rle | compressed | treeless
        lit_format   the 2-bit size format of the literals section header
        lit_header   bytes of that header (1, 2, 3 | 3, 4, 5)
        regen        regenerated size: the number of literals
        lit_csize    compressed size (Huffman literals), else None
        streams      1 or 4 (Huffman literals), else None
        tree         the tree description's first byte (compressed literals): < 128 FSE-compressed weights of that many
                     bytes, >= 128 direct 4-bit weights of (byte - 127) symbols; else None
        nseq, nseq_bytes   the sequence count and the bytes it takes (1, 2 or 3)
        modes        (LL, OF, ML) table modes, None without sequences
    Raises AssertionError where walk() finds the structure broken."""
    info = walk(frame)
    assert info is not None, "broken frame"
    b = bytes(frame)
    fhd = b[4]
    fcs_flag, single, did = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs_flag]
    for blk in info["blocks"]:
        body = b[p + 3:p + 3 + blk["size"]]
        p += 3 + (1 if blk["type"] == "rle" else blk["size"])
        if blk["type"] != "compressed":
            continue
        assert not blk.get("broken"), blk
        b0 = body[0]
        lt, sf = b0 & 3, (b0 >> 2) & 3
        blk["lit_format"] = sf
        if lt < 2:
            hl = (1, 2, 1, 3)[sf]
            blk["regen"] = b0 >> 3 if hl == 1 else int.from_bytes(body[:hl], "little") >> 4
            blk["lit_csize"] = blk["streams"] = blk["tree"] = None
            q = hl + (blk["regen"] if lt == 0 else 1)
        else:
            hl, bits = (3, 3, 4, 5)[sf], (10, 10, 14, 18)[sf]
            h = int.from_bytes(body[:hl], "little")
            blk["regen"] = (h >> 4) & ((1 << bits) - 1)
            blk["lit_csize"] = (h >> (4 + bits)) & ((1 << bits) - 1)
            blk["streams"] = 1 if sf == 0 else 4
            blk["tree"] = body[hl] if lt == 2 else None
            q = hl + blk["lit_csize"]
        blk["lit_header"] = hl
        s0 = body[q]
        blk["nseq_bytes"] = 1 if s0 < 128 else (2 if s0 < 255 else 3)
    return info


def zstd_nbmax(B):
    """blocks per frame the batch planner takes (zstd_pipe.hip make_layout: B / 128 KiB + 2); more go to the fused kernel"""
    return min(B // 131072 + 2, 254)


def few_sequence_block(rng, n):
    """periodic with a few disturbed bytes: one to five sequences (test_oracle_golden.few_sequence_blocks at a fixed size)"""
    per = int(rng.choice([1, 2, 3, 4, 8, 13, 64]))
    blk = np.tile(rng.integers(0, 256, per, dtype=np.uint8), (n + per - 1) // per)[:n].copy()
    for _ in range(int(rng.integers(0, 5))):
        blk[int(rng.integers(0, n))] ^= int(rng.integers(1, 256))
    return blk


def zstd_corpus(stock, oracle, seed):
    """non-default frames: [(name, B, frame)].  Checksummed ones with broken copies, small windows (at the planner's nbmax
    and one past it), no content size, forced literal modes, minMatch 3, long-distance matching, targetCBlockSize, blocks of
    few sequences, and mutations of a sample of all of them."""
    import oracle_lib as ol
    import stress_gpu
    stock.zstd_check_param_bounds()
    rng = np.random.default_rng(seed)
    out = []

    def data(B, k):
        k %= 7
        return oracle.synth(seed, k, B, k) if k < 5 else stress_gpu.make_block(rng, B)

    def add(name, B, raw, **p):
        params = {ol.ZSTD_C_COMPRESSION_LEVEL: p.pop("level", 3)}
        for key, num in (("wlog", ol.ZSTD_C_WINDOWLOG), ("minmatch", ol.ZSTD_C_MINMATCH), ("ldm", ol.ZSTD_C_ENABLE_LDM),
                         ("csize", ol.ZSTD_C_CONTENTSIZE_FLAG), ("checksum", ol.ZSTD_C_CHECKSUM_FLAG),
                         ("litmode", ol.ZSTD_C_LITERAL_COMPRESSION_MODE), ("target", ol.ZSTD_C_TARGET_CBLOCK_SIZE)):
            if key in p:
                params[num] = p.pop(key)
        assert not p, p
        f = stock.zstd_compress2(raw, params)
        assert f is not None, (name, B)
        out.append((name, B, f))
        return f

    # checksum on; copies with a flipped checksum bit, and with a valid structure over one changed byte (old checksum)
    for B in (4096, 131072, 1 << 20):
        for i, lvl in enumerate((1, 3, 9) if B < (1 << 20) else (1, 3)):
            raw = data(B, i + B)
            f = add("checksum/l%d" % lvl, B, raw, level=lvl, checksum=1)
            g = f.copy()
            g[len(g) - 1 - int(rng.integers(0, 4))] ^= 1 << int(rng.integers(0, 8))
            out.append(("checksum_bitflip/l%d" % lvl, B, g))
            raw2 = raw.copy()
            raw2[int(rng.integers(0, B))] ^= 0x5A
            h = stock.zstd_compress2(raw2, {ol.ZSTD_C_COMPRESSION_LEVEL: lvl, ol.ZSTD_C_CHECKSUM_FLAG: 1})
            h[-4:] = f[-4:]
            out.append(("checksum_of_other_data/l%d" % lvl, B, h))
    # small windows; blocks per frame at the planner's nbmax and one past it
    for B, wl in ((131072, 10), (131072, 12), (131072, 15), (131072, 16), (131072, 17), (4096, 10),
                  (262144, 16), (262145, 16), (1 << 20, 17), (1 << 20, 16)):
        for k in range(2):
            add("wlog%d" % wl, B, data(B, k + wl), level=(1, 5)[k], wlog=wl, checksum=k)
    # no content size, with and without a checksum
    for B in (4096, 131072, 300001):
        for ck in (0, 1):
            add("no_content_size/ck%d" % ck, B, data(B, B + ck), level=3, csize=0, checksum=ck)
    # forced literal modes: 1 = Huffman at the fast levels, 2 = raw at the others
    for B in (4096, 131072):
        for k, (lvl, lm) in enumerate(((-5, 1), (-1, 1), (3, 2), (9, 2), (19, 2))):
            if B > 4096 and lvl == 19:
                continue
            add("litmode%d/l%d" % (lm, lvl), B, data(B, k), level=lvl, litmode=lm)
    # minMatch 3, long-distance matching
    for B in (4096, 131072):
        for lvl in range(3, 10):
            add("minmatch3/l%d" % lvl, B, data(B, lvl), level=lvl, minmatch=3)
    for B in (131072, 1 << 20):
        add("ldm/wlog20", B, data(B, 5), level=3, ldm=1, wlog=20)
    # targetCBlockSize: splits blocks into small ones with treeless literals and Repeat-mode tables (some of its frames are
    # undecodable by the library itself: verdict cases)
    for B in (4096, 131072):
        for dist in range(5):
            for tgt in (64, 1340, 4096):
                for lvl in (1, 3, 9):
                    if B > 4096 and (dist + tgt + lvl) % 3:
                        continue
                    add("target%d/l%d/d%d" % (tgt, lvl, dist), B, oracle.synth(seed, 40 + dist, B, dist), level=lvl, target=tgt)
    # blocks of few sequences: predefined / RLE / new tables on very few symbols
    for B in (4096, 32768, 131072):
        for k in range(12):
            blk = few_sequence_block(rng, B)
            for lvl in (1, 3, 5, 9, 19):
                if B > 32768 and lvl == 19:
                    continue
                add("few_sequences/l%d" % lvl, B, blk, level=lvl)
    # mutations of a sample of everything above
    base = list(out)
    for j in rng.choice(len(base), size=len(base) // 3, replace=False):
        name, B, f = base[int(j)]
        out.append(("mutated/" + name, B, stress_gpu.mutate(rng, f)))
    return out
