"""A Zstandard frame assembler and a plain model of the frames it writes (test infrastructure, RFC 8878).

libzstd's encoder writes a narrow part of what its decoder takes.  This module writes a frame from a description instead:
frame header fields of every size, raw / RLE / compressed / reserved blocks, raw / RLE / Huffman / treeless literals in every
header format (weights direct or FSE-compressed, 1 or 4 streams), a sequence section with any of the three count forms and
predefined / RLE / described / Repeat tables, and a backwards sequence bitstream written from a list of
(literal length, offset value, match length) -- offset value 1..3 for the repeat codes, else offset + 3.

Frame is both the writer and the model: every add_* call appends the bytes and executes the same description (literals,
repeat-offset history with the "rep0 - 1 = 0 is forced to 1" floor and the ll = 0 shift, copies), so .content holds the
bytes a decoder must produce while the description is valid and .valid turns False where the model itself sees a rule broken
(an offset beyond the output, literals that run out).  It keeps the bookkeeping the coverage tests count: count forms, table
modes, how often the floor was met.

Every bit writer is linear in the stream length (64-bit flushes, no growing integers).
crafted_corpus() is the corpus built on it; see there.  Measured build time of the whole corpus (245 frames, 1.8 MB): 4.4 s on
one CPU core, most of it the two full-size blocks of 43 690 sequences."""
import numpy as np

import zstd_craft

MAGIC = (0xFD2FB528).to_bytes(4, "little")
BLOCK_MAX = 131072

LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 0x80, 0x100, 0x200,
           0x400, 0x800, 0x1000, 0x2000, 0x4000, 0x8000, 0x10000]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 0x83, 0x103, 0x203, 0x403, 0x803, 0x1003, 0x2003,
                                0x4003, 0x8003, 0x10003]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
ML_DEF = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_DEF = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
DEFAULTS = ((LL_DEF, 6), (OF_DEF, 5), (ML_DEF, 6))
MAX_LOG = (9, 8, 9)           # LL, OF, ML
MAX_SYM = (35, 31, 52)
_PREDEFINED = {}


# ---------------------------------------------------------------- bit writers
def pack_bits(fields):
    """[(value, nbits)] -> (bytes, bit count); the first field lands in the lowest bits of byte 0.  Linear."""
    out = bytearray()
    acc = n = total = 0
    for v, nb in fields:
        acc |= (v & ((1 << nb) - 1)) << n
        n += nb
        total += nb
        if n >= 64:
            out += (acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            acc >>= 64
            n -= 64
    out += acc.to_bytes((n + 7) // 8, "little")
    return bytes(out), total


def backward_stream(read_order, trailing=0, missing=0):
    """fields in the order a backwards reader takes them -> stream with its end mark.  `trailing` bits nobody reads are put
    below the first-written bit; `missing` drops that many of the bits read last."""
    fields = list(reversed(read_order))
    if trailing:
        fields.insert(0, ((1 << trailing) - 1, trailing))
    while missing and fields:
        v, nb = fields[0]
        d = min(nb, missing)
        fields[0] = (v >> d, nb - d)
        missing -= d
        if fields[0][1] == 0:
            fields.pop(0)
    fields.append((1, 1))
    return pack_bits(fields)[0]


# ---------------------------------------------------------------- FSE
class FseTable:
    """decode table of RFC 8878 4.1.1 from a normalised distribution (-1: "less than 1"), and for every symbol the map
    "state after the update" -> "state before" that an encoder needs"""

    def __init__(self, norm, log):
        size = 1 << log
        self.log, self.norm = log, list(norm)
        cell, high = [0] * size, size - 1
        for s, c in enumerate(norm):
            if c == -1:
                cell[high] = s
                high -= 1
        pos, step = 0, (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                cell[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        assert pos == 0 and sum(abs(c) for c in norm) == size, (norm, log)
        nxt = [1 if c == -1 else c for c in norm]
        self.sym, self.nb, self.base = cell, [0] * size, [0] * size
        self.back = {s: [None] * size for s, c in enumerate(norm) if c}
        self.first = {}
        for i in range(size):
            s = cell[i]
            ns = nxt[s]
            nxt[s] += 1
            nb = log - (ns.bit_length() - 1)
            self.nb[i], self.base[i] = nb, (ns << nb) - size
            self.first.setdefault(s, i)
            bk = self.back[s]
            for t in range(self.base[i], self.base[i] + (1 << nb)):
                bk[t] = i

    @classmethod
    def rle(cls, sym):
        t = cls.__new__(cls)
        t.log, t.norm, t.sym, t.nb, t.base = 0, None, [sym], [0], [0]
        t.back, t.first = {sym: [0]}, {sym: 0}
        return t

    def states(self, syms):
        """the states a decoder passes through while it emits syms, chosen from the last symbol to the first"""
        n = len(syms)
        st = [0] * n
        if self.log == 0:                    # an RLE table has one state, whatever the sequences would like
            return st
        st[-1] = self.first[syms[-1]]
        for i in range(n - 2, -1, -1):
            st[i] = self.back[syms[i]][st[i + 1]]
        return st


def write_ncount(norm, log, lax=False):
    """the table description of RFC 8878 4.1.1: accuracy log, then the probabilities in variable widths, zero runs as 2-bit
    repeat flags.  lax: write a distribution whose counts overshoot the table size as far as it goes."""
    f = [(log - 5, 4)]
    remaining, threshold, nb = (1 << log) + 1, 1 << log, log + 1
    s, prev0, n = 0, False, len(norm)
    while s < n and remaining > 1:
        if prev0:
            start = s
            while s < n and norm[s] == 0:
                s += 1
            assert s < n
            while s >= start + 3:
                start += 3
                f.append((3, 2))
            f.append((s - start, 2))
        c = norm[s]
        s += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        c += 1
        if c >= threshold:
            c += mx
        f.append((c, nb - (c < mx)))
        prev0 = c == 1
        assert lax or remaining >= 1
        while remaining < threshold and threshold > 1:
            nb -= 1
            threshold >>= 1
    assert lax or (remaining == 1 and all(c == 0 for c in norm[s:])), norm
    return pack_bits(f)[0]


def zero_run_flags(norm):
    """how many 2-bit repeat flags each zero run of a distribution takes in write_ncount"""
    runs, i = [], 0
    while i < len(norm):
        j = i + 1
        if norm[i] == 0:
            while j < len(norm) and norm[j] == 0:
                j += 1
            runs.append((j - i - 1) // 3 + 1)
        i = j
    return runs


def spread_norm(used, log, alphabet, low=()):
    """a distribution over `alphabet` symbols: every symbol of `used` gets a share of 2^log, those in `low` "less than 1"."""
    used = sorted(set(used) - set(low))
    norm = [0] * alphabet
    for s in low:
        norm[s] = -1
    left = (1 << log) - len(low)
    assert used and left >= len(used)
    for i, s in enumerate(used):
        norm[s] = left // len(used) + (1 if i < left % len(used) else 0)
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


# ---------------------------------------------------------------- Huffman
huf_codes = zstd_craft.huf_codes       # canonical codes from a weight list, shared with huf12_frame


def huf_stream(symbols, codes, trailing=0, zero_last=False):
    s = backward_stream([codes[int(x)] for x in symbols], trailing=trailing)
    return s + b"\x00" if zero_last else s


def huf_tree_direct(weights):
    nw = len(weights) - 1
    assert 1 <= nw <= 128
    return bytes([127 + nw]) + bytes((weights[i] << 4) | (weights[i + 1] if i + 1 < nw else 0) for i in range(0, nw, 2))


def huf_tree_fse(weights):
    """the weights (all but the implied last) through a two-state FSE stream, as RFC 8878 4.2.1.2 reads it: the states take
    turns, and the stream ends when an update runs dry -- so the state under the last but one weight must need bits"""
    w = list(weights[:-1])
    n = len(w)
    assert n >= 2
    cnt = [w.count(v) for v in range(max(w) + 1)]
    log = 6 if n >= 32 else 5
    norm = [0] * len(cnt)
    share = (1 << log) - sum(1 for c in cnt if c)
    tot = sum(cnt)
    for v, c in enumerate(cnt):
        if c:
            norm[v] = 1 + c * share // tot
    norm[max(range(len(cnt)), key=lambda v: cnt[v])] += (1 << log) - sum(norm)
    t = FseTable(norm, log)
    chains = [w[0::2], w[1::2]]
    sts = []
    for k, ch in enumerate(chains):
        st = [0] * len(ch)
        runs_dry = (n - 2) % 2 == k          # this chain holds the last but one weight
        cand = [i for i in range(1 << log) if t.sym[i] == ch[-1] and (t.nb[i] > 0 or not runs_dry)]
        st[-1] = cand[0]
        for i in range(len(ch) - 2, -1, -1):
            st[i] = t.back[ch[i]][st[i + 1]]
        sts.append(st)
    order = [(sts[0][0], log), (sts[1][0], log)]
    for j in range(n - 2):                    # the update behind weight j, by the chain that emitted it
        st, i = sts[j % 2], j // 2
        order.append((st[i + 1] - t.base[st[i]], t.nb[st[i]]))
    body = write_ncount(norm, log) + backward_stream(order)
    assert len(body) < 128
    return bytes([len(body)]) + body


# ---------------------------------------------------------------- sequences
def _code(base, v):
    c = len(base) - 1
    while base[c] > v:
        c -= 1
    return c


def seq_codes(ll, ofv, ml):
    """(LL code, extra), (OF code, extra), (ML code, extra) of one sequence"""
    lc, mc = _code(LL_BASE, ll), _code(ML_BASE, ml)
    oc = ofv.bit_length() - 1
    assert ll - LL_BASE[lc] < (1 << LL_BITS[lc]) and ml - ML_BASE[mc] < (1 << ML_BITS[mc]) and ofv >= 1
    return (lc, ll - LL_BASE[lc]), (oc, ofv - (1 << oc)), (mc, ml - ML_BASE[mc])


def seq_count(n, form=None):
    """the 1-, 2- or 3-byte sequence count; form picks a longer one than n needs"""
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert 0x7F00 <= n <= 0x7F00 + 0xFFFF
    return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")


class Frame:
    """writer and model of one frame.  Table arguments (ll=, of=, ml=): "predefined", "repeat", ("rle", symbol),
    ("fse", norm, log) or ("fse", norm, log, "lax")."""

    def __init__(self, floor=True, shift=True):
        self.blocks = bytearray()
        self.out = bytearray()
        self.valid = True
        self.rep = [1, 4, 8]
        self.tables = [None, None, None]
        self.huf = None
        self.floor, self.shift = floor, shift
        self.stats = {"floor": 0, "count_forms": set(), "modes": [set(), set(), set()], "nblocks": 0, "lat_total": 0,
                      "max_seq_bits": 0}
        self._open = True
        self.script = []                     # what the model executed: ("bytes", data) | ("block", literals, sequences)

    # ---- blocks
    def _block(self, btype, size, payload, last):
        assert self._open
        self.blocks += ((size << 3) | (btype << 1) | int(last)).to_bytes(3, "little") + payload
        self.stats["nblocks"] += 1
        self._open = not last

    def add_raw(self, data, last=False):
        data = bytes(data)
        self._block(0, len(data), data, last)
        self.out += data
        self.script.append(("bytes", data))
        self.stats["lat_total"] += 1

    def add_rle(self, byte, n, last=False):
        self._block(1, n, bytes([byte]), last)
        self.out += bytes([byte]) * n
        self.script.append(("bytes", bytes([byte]) * n))
        self.stats["lat_total"] += 1

    def add_reserved(self, payload=b"", last=True):
        self._block(3, len(payload), bytes(payload), last)
        self.valid = False

    def add_compressed(self, literals, seqs=(), last=False, ll="predefined", of="predefined", ml="predefined", count_form=None,
                       trailing=0, missing=0, size=None):
        """literals: (section bytes, literal bytes) from one of the lit_* methods; seqs: [(ll, offset value, ml)].
        size: the block size to state, when not the payload's"""
        lit_bytes, lits = literals
        seqs = list(seqs)
        body = lit_bytes + self._sequences(seqs, (ll, of, ml), count_form, trailing, missing)
        self._block(2, len(body) if size is None else size, body, last)
        self._execute(lits, seqs)
        self.script.append(("block", lits, seqs))
        self.stats["lat_total"] += len(seqs) + 1
        return len(body)

    # ---- literal sections
    @staticmethod
    def lit_raw(data, fmt=None, rle=False):
        """raw literals, or RLE ones (data: one repeated byte); fmt 0 / 2: 1-byte header, 1: 2 bytes, 3: 3 bytes"""
        data = bytes(data)
        n = len(data)
        if fmt is None:
            fmt = 0 if n < 32 else 1 if n < 4096 else 3
        t = 1 if rle else 0
        if fmt in (0, 2):
            assert n < 32
            h = bytes([t | (fmt << 2) | (n << 3)])
        elif fmt == 1:
            assert n < 4096
            h = (t | (1 << 2) | (n << 4)).to_bytes(2, "little")
        else:
            assert n < (1 << 20)
            h = (t | (3 << 2) | (n << 4)).to_bytes(3, "little")
        if rle:
            assert n >= 1 and data == data[:1] * n
            return h + data[:1], data
        return h + data, data

    def lit_huf(self, data, weights=None, streams=4, fmt=None, fse=False, tree=None, jump=None, trailing=0, zero_last=False, bad=1):
        """Huffman literals from a weight list (all symbols, the implied last included), or treeless (weights None: the
        frame's last table).  fmt: 0 (1 stream) / 1 / 2 / 3 as in the section header, default the smallest that fits.
        trailing (unread bits) and zero_last (a last byte of 0) break stream `bad` of four; jump: the jump table to write."""
        data = bytes(data)
        n = len(data)
        if weights is not None:
            self.huf = huf_codes(weights)[0]
            tree = tree if tree is not None else (huf_tree_fse(weights) if fse else huf_tree_direct(weights))
        else:
            tree = b""
        codes = self.huf if self.huf is not None else {b: (0, 1) for b in set(data)}   # treeless with no table: any bits
        if self.huf is None:
            self.valid = False
        if trailing or zero_last or jump is not None:
            self.valid = False
        if streams == 1:
            body = huf_stream(data, codes, trailing, zero_last)
        else:
            seg = (n + 3) // 4
            parts = [huf_stream(data[i * seg:(i + 1) * seg], codes, trailing if i == bad else 0, zero_last and i == bad)
                     for i in range(4)]
            jt = jump if jump is not None else [len(q) for q in parts[:3]]
            body = b"".join(int(j).to_bytes(2, "little") for j in jt) + b"".join(parts)
            if 3 * seg > n:
                self.valid = False           # the fourth stream would hold a negative count (libzstd: corruption)
        csize = len(tree) + len(body)
        if fmt is None:
            fmt = (0 if streams == 1 else 1) if max(n, csize) < 1024 else 2 if max(n, csize) < 16384 else 3
        assert (fmt == 0) == (streams == 1)
        bits = (10, 10, 14, 18)[fmt]
        assert max(n, csize) < (1 << bits)
        t = 2 if weights is not None else 3
        h = (t | (fmt << 2) | (n << 4) | (csize << (4 + bits))).to_bytes((3, 3, 4, 5)[fmt], "little")
        return h + tree + body, data

    # ---- sequence section
    def _table(self, k, spec, used):
        if spec == "predefined":
            if k not in _PREDEFINED:
                _PREDEFINED[k] = FseTable(*DEFAULTS[k])
            return 0, b"", _PREDEFINED[k]
        if spec == "repeat":
            if self.tables[k] is None:
                self.valid = False
                return 3, b"", FseTable(spread_norm(used, MAX_LOG[k] - 2, MAX_SYM[k] + 1), MAX_LOG[k] - 2)
            return 3, b"", self.tables[k]
        if spec[0] == "rle":
            if spec[1] > MAX_SYM[k]:
                self.valid = False
            return 1, bytes([spec[1]]), FseTable.rle(spec[1])
        norm, log = spec[1], spec[2]
        lax = len(spec) > 3
        if lax or log > MAX_LOG[k]:
            self.valid = False
        good = list(norm)
        if lax:                              # the states come from the distribution before it was broken
            good[max(range(len(good)), key=lambda s: good[s])] -= sum(abs(c) for c in good) - (1 << log)
        return 2, write_ncount(norm, log, lax), FseTable(good, log)

    def _sequences(self, seqs, specs, count_form, trailing, missing):
        n = len(seqs)
        if n == 0:
            return seq_count(0, count_form)
        form = count_form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
        codes = [seq_codes(*s) for s in seqs]
        cols = [[c[k][0] for c in codes] for k in (0, 1, 2)]
        modes, desc, tabs = [], b"", []
        for k in range(3):
            m, d, t = self._table(k, specs[k], cols[k])
            modes.append(m)
            desc += d
            tabs.append(t)
        for k in range(3):                   # a block's tables are the next block's Repeat tables, also when rejected later
            self.tables[k] = tabs[k]
        tl, to, tm = tabs
        sl, so, sm = tl.states(cols[0]), to.states(cols[1]), tm.states(cols[2])
        order = [(sl[0], tl.log), (so[0], to.log), (sm[0], tm.log)]
        widest = 0
        for i, ((lc, lx), (oc, ox), (mc, mx)) in enumerate(codes):
            order += [(ox, oc), (mx, ML_BITS[mc]), (lx, LL_BITS[lc])]
            bits = oc + ML_BITS[mc] + LL_BITS[lc]
            if i + 1 < n:
                order += [(sl[i + 1] - tl.base[sl[i]], tl.nb[sl[i]]), (sm[i + 1] - tm.base[sm[i]], tm.nb[sm[i]]),
                          (so[i + 1] - to.base[so[i]], to.nb[so[i]])]
                bits += tl.nb[sl[i]] + tm.nb[sm[i]] + to.nb[so[i]]
            widest = max(widest, bits)
        if trailing or missing:
            self.valid = False
        if self.valid:
            self.stats["count_forms"].add(form)
            for k in range(3):
                self.stats["modes"][k].add(zstd_craft.MODES[modes[k]])
        self.stats["max_seq_bits"] = max(self.stats["max_seq_bits"], widest)
        return (seq_count(n, count_form) + bytes([(modes[0] << 6) | (modes[1] << 4) | (modes[2] << 2)]) + desc +
                backward_stream(order, trailing, missing))

    # ---- the model
    def _execute(self, lits, seqs):
        out, rep, lp = self.out, self.rep, 0
        start = len(out)
        for ll, ofv, ml in seqs:
            if ofv > 3:
                off = ofv - 3
                rep[:] = [off, rep[0], rep[1]]
            else:
                idx = ofv - 1 + (1 if ll == 0 and self.shift else 0)
                if idx == 0:
                    off = rep[0]
                elif idx == 3:
                    off = rep[0] - 1
                    if off == 0 and self.floor:
                        off = 1
                        self.stats["floor"] += 1
                    rep[:] = [off, rep[0], rep[1]]
                elif idx == 1:
                    off = rep[1]
                    rep[:] = [off, rep[0], rep[2]]
                else:
                    off = rep[2]
                    rep[:] = [off, rep[0], rep[1]]
            if ll > len(lits) - lp:
                self.valid = False
                return
            out += lits[lp:lp + ll]
            lp += ll
            if off > len(out) or off == 0:
                self.valid = False
                return
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                out += (out[len(out) - off:] * (ml // off + 1))[:ml]
        out += lits[lp:]
        if len(out) - start > BLOCK_MAX:
            self.valid = False

    def model(self, floor=True, shift=True):
        """the described content executed again, with or without the floor rule and the ll = 0 shift; None where it breaks"""
        m = Frame(floor, shift)
        for step in self.script:
            if step[0] == "bytes":
                m.out += step[1]
            else:
                m._execute(step[1], step[2])
        return m.content if m.valid else None

    # ---- the frame
    def frame(self, single=True, fcs_bytes=None, fcs=None, window=None, did_bytes=0, did=0, checksum=None, reserved=0, unused=0):
        """header + blocks (+ checksum).  fcs_bytes 0 / 1 / 2 / 4 / 8 (1 needs single); window: (exponent, mantissa) byte when not
        single; checksum: True for the right one, an int for a given one."""
        assert not self._open, "no last block"
        n = len(self.out) if fcs is None else fcs
        if fcs_bytes is None:
            fcs_bytes = 1 if single and n < 256 else 2 if 256 <= n < 65792 else 4
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
        assert (fcs_bytes == 1) <= single and not (single and fcs_bytes == 0)
        fhd = (flag << 6) | (int(single) << 5) | (unused << 4) | (reserved << 3) | ((checksum is not None) << 2) | \
            {0: 0, 1: 1, 2: 2, 4: 3}[did_bytes]
        h = MAGIC + bytes([fhd])
        if not single:
            h += bytes([(window[0] << 3) | window[1]])
        h += did.to_bytes(did_bytes, "little")
        h += (n - 256 if fcs_bytes == 2 else n if fcs_bytes else 0).to_bytes(fcs_bytes, "little")
        f = h + bytes(self.blocks)
        if checksum is not None:
            if checksum is True:
                from test_gpu_zstd_checksum import xxh64_py
                checksum = xxh64_py(self.out) & 0xFFFFFFFF
            f += int(checksum).to_bytes(4, "little")
        return np.frombuffer(f, np.uint8).copy()

    @property
    def content(self):
        return np.frombuffer(bytes(self.out), np.uint8)


def skippable(payload, nibble=0):
    return (0x184D2A50 + nibble).to_bytes(4, "little") + len(payload).to_bytes(4, "little") + bytes(payload)


# ---------------------------------------------------------------- the corpus
def lat_nmax(B):
    """sequences per frame the few-frames execution takes (zstd_pipe.hip make_layout)"""
    return (B // 4 + 2 * zstd_craft.zstd_nbmax(B) + 255) & ~255


CHAIN_K = (1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513)
W_LOG = {1: [1, 1], 2: [2, 1, 1], 6: [6, 5, 4, 3, 2, 1, 1], 11: [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1],
         12: list(zstd_craft.WEIGHTS)}
# rejected cases: each is one of the named edges, by name prefix
REJECT_EDGES = ("A/initial_history_early", "B/ll_code_too_long", "B/ml_code_too_long", "B/full_block_131072",
                "C/rle_symbol_36", "C/rle_symbol_32", "C/rle_symbol_53", "C/described_log_over", "C/described_bad_sum",
                "C/repeat_first_block", "C/treeless_first_block", "D/four_streams_5", "D/stream_last_byte_0",
                "D/stream_unread_bits", "D/jump_table_long", "E/fcs_wrong", "E/window_exp22", "E/dict_id_1",
                "E/reserved_bit", "E/block_type_3", "E/trailing_bytes", "E/checksum_wrong")


# every one of these holds at least one accepted case, by name prefix
FAMILIES = ("A/chain/", "A/walk700/", "A/walk5000/", "A/initial_history_used_late/", "A/history_across/raw",
            "A/history_across/rle", "A/history_across/empty", "B/count/127", "B/count/128", "B/count/32511", "B/count/32512",
            "B/count/32513", "B/lat_total/511", "B/lat_total/512", "B/lat_total/%d" % lat_nmax(32768),
            "B/lat_total/%d" % (lat_nmax(32768) + 1), "B/third_of_B/", "B/ll_codes/", "B/ll_codes_big/", "B/ml_codes/",
            "B/ml_codes_big/", "B/wide_sequences/", "B/full_block_131071", "C/rle_ll", "C/rle_of", "C/rle_ml",
            "C/described_log_5", "C/described_log_max", "C/described_less_than_1", "C/described_zero_runs",
            "C/repeat_after_predefined/next", "C/repeat_after_rle/next", "C/repeat_after_described/next",
            "C/repeat_after_predefined/empty", "C/repeat_after_rle/raw", "C/repeat_after_described/empty",
            "C/treeless_after_huffman/next", "C/treeless_after_huffman/raw_literals", "D/raw_literals/fmt1",
            "D/raw_literals/fmt2", "D/raw_literals/fmt3", "D/rle_literals/fmt1", "D/rle_literals/fmt2", "D/rle_literals/fmt3",
            "D/rle_literals/with_sequences", "D/zero_literals", "D/huffman/log1/", "D/huffman/log2/", "D/huffman/log6/",
            "D/huffman/log11/", "D/huffman/log12/", "D/huffman/log6/fse/", "D/huffman/log11/direct/1", "D/huffman/header_fmt2",
            "D/huffman/header_fmt3", "D/four_streams_4", "D/four_streams_6", "D/four_streams_9", "D/unequal_streams/4095",
            "D/unequal_streams/4096", "D/unequal_streams/4097", "E/fcs_0_bytes", "E/fcs_1_bytes", "E/fcs_2_bytes/256",
            "E/fcs_2_bytes/65791", "E/fcs_4_bytes", "E/fcs_8_bytes", "E/window_larger", "E/window_equal", "E/window_smaller",
            "E/window_exp21", "E/dict_id_0/1", "E/dict_id_0/2", "E/dict_id_0/4", "E/unused_bit", "E/order2/", "E/order3/",
            "E/last_raw_block_of_0", "E/rle_block_of_B", "E/behind_skippable", "E/two_frames", "E/checksum_right")


def crafted_cases(seed):
    """[(name, B, frame, declared, Frame or None)]: crafted_corpus with the writer/model objects (None where a case is made
    of several frames or of bytes around one)"""
    rng = np.random.default_rng(seed)
    out = []

    def rnd(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def emit(name, B, fr, declared, frame=None, **hdr):
        f = fr.frame(**hdr) if frame is None else frame
        if declared and frame is None:
            assert fr.valid and len(fr.out) == B, (name, fr.valid, len(fr.out), B)
        out.append((name, B, f, declared, fr if frame is None else None))

    def block(fr, B, seqs, last=True, lit_fmt=None, lit_rle=False, **kw):
        """a compressed block of raw literals that brings the frame's output to B bytes: the sequences' literals, then as
        many trailing literals as are missing"""
        need = B - len(fr.out) - sum(s[0] + s[2] for s in seqs)
        assert need >= 0, need
        nl = sum(s[0] for s in seqs) + need
        fr.add_compressed(Frame.lit_raw(b"\x6c" * nl if lit_rle else rnd(nl), lit_fmt, lit_rle), seqs, last=last, **kw)

    def one(name, B, seqs, declared=True, hdr=None, **kw):
        fr = Frame()
        block(fr, B, seqs, **kw)
        emit(name, B, fr, declared, **(hdr or {}))
        return fr

    # ---------------- A. repeat-offset history
    B = 4096
    for k in CHAIN_K:
        for r in sorted({1, 2, 3, k + 2}):
            # rep0 = r after the first sequence, then k times "rep0 - 1": the floor at once, after one or two steps, never
            one("A/chain/k%d/r%d" % (k, r), B, [(k + 2, r + 3, 3)] + [(0, 3, 3)] * k)
    for n, Bw in ((700, 4096), (5000, 32768)):
        for j in range(3 if n == 700 else 2):
            seqs = [(16, 4 + int(rng.integers(0, 11)), 3)]
            for _ in range(n - 1):
                ofv = int(rng.integers(1, 4)) if rng.random() < 0.75 else 4 + int(rng.integers(0, 11))
                seqs.append((int(rng.integers(0, 3)), ofv, 3 if rng.random() < 0.8 else 4))
            one("A/walk%d/%d" % (n, j), Bw, seqs)
    one("A/initial_history_used_late/0", B, [(8, 1, 4), (1, 2, 3), (2, 3, 5), (0, 1, 3), (0, 2, 3), (0, 3, 3)])
    one("A/initial_history_used_late/1", B, [(9, 3, 4), (0, 3, 3)])
    fr = Frame()
    fr.add_raw(rnd(8))
    block(fr, B, [(0, 2, 3), (0, 1, 3), (1, 3, 3)])          # rep2 = 8 straight after a raw block of 8 bytes
    emit("A/initial_history_used_late/2", B, fr, True)
    one("A/initial_history_early/ll0_rep", B, [(0, 1, 3)], declared=False)
    one("A/initial_history_early/rep1_at_3", B, [(3, 2, 3)], declared=False)
    one("A/initial_history_early/rep2_at_7", B, [(7, 3, 3)], declared=False)
    fr = Frame()
    fr.add_raw(rnd(3))
    block(fr, B, [(0, 1, 3)])                                # rep1 = 4 behind a raw block of 3 bytes
    emit("A/initial_history_early/after_raw_block", B, fr, False)
    for mid in ("raw", "rle", "empty"):
        fr = Frame()
        block(fr, 64, [(20, 5 + 3, 3), (1, 6 + 3, 3), (1, 7 + 3, 3)], last=False)
        if mid == "raw":
            fr.add_raw(rnd(33))
        elif mid == "rle":
            fr.add_rle(0x41, 33)
        else:
            fr.add_compressed(Frame.lit_raw(rnd(33)), [])
        block(fr, B, [(1, 3, 3), (0, 3, 3), (0, 1, 4), (2, 2, 3), (0, 2, 3)])
        emit("A/history_across/" + mid, B, fr, True)

    # ---------------- B. counts and field widths
    for n in (127, 128):
        one("B/count/%d" % n, B, [(1, 4, 3)] * n)
    one("B/count/long_form_of_100", B, [(1, 4, 3)] * 100, count_form=2)
    for n in (0x7EFF, 0x7F00, 0x7F01):
        one("B/count/%d" % n, 131072, [(1, 4, 3)] * n)
    BL = 32768
    for n in (510, 511, lat_nmax(BL) - 1, lat_nmax(BL)):     # k_zlat_count's total is nseq + 1
        one("B/lat_total/%d" % (n + 1), BL, [(1, 4, 3)] + [(0, 4 + int(rng.integers(0, 2)), 3)] * (n - 1))
    for j in range(3):
        one("B/third_of_B/%d" % j, B, [(1, 4, 3)] + [(0, 4, 3)] * (B // 3 - 1))

    def pack(name, lens, mk, Bp, **kw):
        group, room, j = [], Bp - 64, 0
        for v in lens + [None]:
            if v is None or v + 4 > room:
                one("%s/%d" % (name, j), Bp, [(8, 4, 3)] + [mk(x) for x in group], **kw)
                group, room, j = [], Bp - 64, j + 1
            if v is not None:
                group.append(v)
                room -= v + 4
    ll_all = [(c, LL_BASE[c] + x) for c in range(16, 36) for x in (0, (1 << LL_BITS[c]) - 1)]
    ml_all = [(c, ML_BASE[c] + x) for c in range(32, 53) for x in (0, (1 << ML_BITS[c]) - 1)]
    pack("B/ll_codes", [v for c, v in ll_all if v < 2048], lambda v: (v, 4, 3), B)
    pack("B/ml_codes", [v for c, v in ml_all if v < 2048], lambda v: (1, 4, v), B)
    pack("B/ll_codes_big", [v for c, v in ll_all if 2048 <= v < 131071], lambda v: (v, 4, 3), 131072,
         lit_rle=True)                                       # so many raw literals would not fit a block
    pack("B/ml_codes_big", [v for c, v in ml_all if 2048 <= v < 131072], lambda v: (1, 4, v), 131072)
    fr = Frame()                                             # LL code 35, all ones: 131 071 literals and a match
    fr.add_compressed(Frame.lit_raw(b"\x6c" * 131071, None, True), [(131071, 4, 3)], last=True)
    emit("B/ll_code_too_long/code35", 131072, fr, False, fcs=131072)
    fr = Frame()                                             # LL code 31 at its base: one match more than B = 4096 holds
    fr.add_compressed(Frame.lit_raw(b"\x6c" * 4096, None, True), [(4096, 4, 3)], last=True)
    emit("B/ll_code_too_long/code31", B, fr, False, fcs=B)
    fr = Frame()                                             # ML code 52, all ones: 131 074 bytes
    fr.add_compressed(Frame.lit_raw(rnd(1)), [(1, 4, 131074)], last=True)
    emit("B/ml_code_too_long/code52", 131072, fr, False, fcs=131072)
    fr = Frame()                                             # ML code 47, all ones: 4 098 bytes behind one literal
    fr.add_compressed(Frame.lit_raw(rnd(1)), [(1, 4, ML_BASE[47] + 2047)], last=True)
    emit("B/ml_code_too_long/code47", B, fr, False, fcs=B)
    # more than 57 bits in one sequence: every used symbol holds one cell of a table at the maximum log
    for j in range(2):
        seqs = [(70000, 4, 3)]
        for _ in range(3):
            seqs.append((LL_BASE[32] + int(rng.integers(0, 1 << 10)), (1 << 16) + int(rng.integers(0, 4000)),
                         ML_BASE[48] + int(rng.integers(0, 1 << 10))))
        seqs += [(0, 3, 3), (1, 4, 3)] * 3
        cols = [set(seq_codes(*q)[k][0] for q in seqs) for k in range(3)]
        specs = []
        for k in range(3):
            norm = [0] * (MAX_SYM[k] + 1)
            for s in cols[k]:
                norm[s] = 1
            fill = min(set(range(8)) - cols[k])
            norm[fill] = (1 << MAX_LOG[k]) - len(cols[k])
            while norm[-1] == 0:
                norm.pop()
            specs.append(("fse", norm, MAX_LOG[k]))
        fr = one("B/wide_sequences/%d" % j, 131072, seqs, ll=specs[0], of=specs[1], ml=specs[2])
        assert fr.stats["max_seq_bits"] > 57, fr.stats
    # a compressed block of 131 071 / 131 072 bytes behind an RLE block: every sequence costs 24 bits (offset codes 16 and
    # 17 with 8 and 7 state bits), a few cheaper ones (codes 8 and 9) trim the section to the byte
    of_norm = [251] + [0] * 7 + [1, 1] + [0] * 6 + [1, 2]
    for size in (131071, 131072):
        n = 131072 // 3
        L = 131072 - 3 * n                                   # trailing literals
        want = (size - 1 - L - 3 - 1 - 1 - 1 - len(write_ncount(of_norm, 8))) * 8 - 1   # stream bits before the end mark
        a = b9 = 0
        while (8 + 24 * n - 8 * a - 7 * b9 - 8) > want:      # code 8: 16 bits, code 9: 17 bits; the last one updates nothing
            if (8 + 24 * n - 8 * a - 7 * b9 - 8) - want >= 8:
                a += 1
            else:
                b9 += 1
        assert 0 <= want - (8 + 24 * n - 8 * a - 7 * b9 - 8) < 8
        seqs = [(0, (1 << 8) + int(rng.integers(0, 256)), 3)] * a + [(0, (1 << 9) + int(rng.integers(0, 512)), 3)] * b9
        while len(seqs) < n - 1:
            c = 16 + (len(seqs) & 1)
            room = (1 << 16) - 8 if c == 16 else min(1 << 16, 3 * len(seqs)) + 1   # code 17 reaches back 131 069 and more
            seqs.append((0, (1 << c) + int(rng.integers(0, room)), 3))
        seqs.append((0, (1 << 16) + 5, 3))                   # the last one: code 16, 8 state bits not written
        fr = Frame()
        fr.add_rle(0x5A, 131072)
        got = fr.add_compressed(Frame.lit_raw(rnd(L), 0), seqs, last=True, ll=("rle", 0), of=("fse", of_norm, 8), ml=("rle", 0))
        assert got == size, (got, size)
        emit("B/full_block_%d" % size, 262144, fr, size == 131071)

    # ---------------- C. table modes
    one("C/rle_ll", B, [(16 + (i & 1), 4 + i % 5, 3 + i % 4) for i in range(40)], ll=("rle", 16))
    one("C/rle_of", B, [(13, 8, 3)] + [(i % 3 + 1, 8 + i % 8, 3 + i % 4) for i in range(40)], of=("rle", 3))
    one("C/rle_ml", B, [(i % 3 + 1, 4 + i % 5, 35 + (i & 1)) for i in range(40)], ml=("rle", 32))
    one("C/rle_all", B, [(17, 9, 4)] * 30, ll=("rle", 16), of=("rle", 3), ml=("rle", 1))
    one("C/rle_symbol_36", B, [(1, 4, 3)] * 5, declared=False, ll=("rle", 36))
    one("C/rle_symbol_32", B, [(1, 4, 3)] * 5, declared=False, of=("rle", 32))
    one("C/rle_symbol_53", B, [(1, 4, 3)] * 5, declared=False, ml=("rle", 53))
    mix = [(16, 4, 3)] + [(int(rng.integers(0, 6)), int(rng.integers(1, 20)), int(rng.integers(3, 9))) for _ in range(150)]
    mixc = [seq_codes(*s) for s in mix]
    used = [sorted(set(c[k][0] for c in mixc)) for k in range(3)]

    def fse(k, log, **kw):
        return ("fse", spread_norm(used[k], log, MAX_SYM[k] + 1, **kw), log)
    one("C/described_log_5", B, mix, ll=fse(0, 5), of=fse(1, 5), ml=fse(2, 5))
    one("C/described_log_max", B, mix, ll=fse(0, 9), of=fse(1, 8), ml=fse(2, 9))
    one("C/described_log_over/ll", B, mix, declared=False, ll=fse(0, 10))
    one("C/described_log_over/of", B, mix, declared=False, of=fse(1, 9))
    one("C/described_log_over/ml", B, mix, declared=False, ml=fse(2, 10))
    one("C/described_less_than_1", B, mix, ll=fse(0, 6, low=used[0][-2:]), of=fse(1, 6, low=used[1][:1]), ml=fse(2, 7, low=used[2][1:3]))
    # zero runs of one repeat flag (ML 0 -> 2, OF 0 -> 2), two (LL 0 -> 5), four (ML 2 -> 13, OF 2 -> 11)
    zr = [(5, 4, 3), (5, 4, 5), (0, 2048 + 77, 16), (5, 5, 3)] * 20
    zn = ([40, 0, 0, 0, 0, 24], [0, 0, 12] + [0] * 8 + [20], [30, 0, 20] + [0] * 10 + [14])
    assert [zero_run_flags(x) for x in zn] == [[2], [1, 3], [1, 4]]
    fr = Frame()
    fr.add_raw(rnd(B - 64 - sum(s[0] + s[2] for s in zr)))
    block(fr, B, zr, ll=("fse", zn[0], 6), of=("fse", zn[1], 5), ml=("fse", zn[2], 6))
    emit("C/described_zero_runs", B, fr, True)
    bad = fse(0, 6)
    bad[1][used[0][0]] += 1
    one("C/described_bad_sum/ll", B, mix, declared=False, ll=bad + ("lax",))
    bad = fse(1, 5)
    bad[1][used[1][-1]] += 1
    one("C/described_bad_sum/of", B, mix, declared=False, of=bad + ("lax",))
    bad = fse(2, 7)
    bad[1][used[2][1]] += 2
    one("C/described_bad_sum/ml", B, mix, declared=False, ml=bad + ("lax",))
    firsts = {"predefined": {}, "rle": dict(ll=("rle", 2), of=("rle", 2), ml=("rle", 1)),
              "described": dict(ll=("fse", [20, 20, 24], 6), of=("fse", [10, 6, 10, 6], 5), ml=("fse", [30, 20, 14], 6))}
    rseq = [(2, 4, 4), (2, 1, 4), (2, 3, 4)] * 8               # LL code 2, OF codes 0..2, ML code 1: in each of the tables
    rep3 = dict(ll="repeat", of="repeat", ml="repeat")
    for first, spec in firsts.items():
        for between in ("next", "empty", "raw"):
            fr = Frame()
            rs = [(2, 4, 4), (2, 5, 4), (2, 7, 4)] * 8 if first == "rle" else rseq     # one code per table
            block(fr, 400, rs, last=False, **spec)
            if between == "empty":
                fr.add_compressed(Frame.lit_raw(rnd(20)), [])
            elif between == "raw":
                fr.add_raw(rnd(20))
            block(fr, B, rs[::-1] + rs, **rep3)
            emit("C/repeat_after_%s/%s" % (first, between), B, fr, True)
    for key in ("ll", "of", "ml"):
        one("C/repeat_first_block/" + key, B, rseq, declared=False, **{key: "repeat"})
    fr = Frame()
    fr.add_raw(rnd(100))
    block(fr, B, rseq, **rep3)
    emit("C/repeat_first_block/after_raw", B, fr, False)
    hw = W_LOG[6]

    def hlits(n, w=hw):
        """n literals over the symbols of a weight list, short codes often, every code at least once"""
        p = np.array([2.0 ** w_ for w_ in w])
        a = rng.choice(len(w), size=n, p=p / p.sum()).astype(np.uint8)
        a[:len(w)] = np.arange(len(w))
        return a.tobytes()

    for between in ("next", "raw_literals"):
        fr = Frame()
        fr.add_compressed(fr.lit_huf(hlits(300), hw, streams=1), [])
        if between == "raw_literals":
            fr.add_compressed(Frame.lit_raw(rnd(40)), [(3, 4, 5)])
        fr.add_compressed(fr.lit_huf(hlits(500), None, streams=4), [(500, 4, B - len(fr.out) - 500)], last=True)
        emit("C/treeless_after_huffman/" + between, B, fr, True)
    fr = Frame()
    fr.add_compressed(fr.lit_huf(hlits(500), None, streams=4), [(500, 4, B - 500)], last=True)
    emit("C/treeless_first_block/0", B, fr, False)
    fr = Frame()
    fr.add_compressed(Frame.lit_raw(rnd(40)), [(3, 4, 5)])
    fr.add_compressed(fr.lit_huf(hlits(500), None, streams=1), [(500, 4, B - len(fr.out) - 500)], last=True)
    emit("C/treeless_first_block/after_raw_literals", B, fr, False)
    fr = Frame()
    fr.add_raw(rnd(40))
    fr.add_compressed(fr.lit_huf(hlits(500), None, streams=4), [(500, 4, B - len(fr.out) - 500)], last=True)
    emit("C/treeless_first_block/after_raw_block", B, fr, False)

    # ---------------- D. literals
    for t, rle in (("raw", False), ("rle", True)):
        for fmt in (0, 1, 2, 3):
            n = 5 + fmt
            data = bytes([0x61 + fmt]) * n if rle else rnd(n)
            fr = Frame()
            fr.add_compressed(Frame.lit_raw(data, fmt, rle), [(n - 1, 4, B - n)], last=True)
            emit("D/%s_literals/fmt%d" % (t, fmt), B, fr, True)
    fr = Frame()
    fr.add_compressed(Frame.lit_raw(b"\x33" * 3000, None, True), [(7, 4, 3), (100, 5, 9), (1000, 1, 3), (0, 2, B - 3015)], last=True)
    emit("D/rle_literals/with_sequences", B, fr, True)
    fr = Frame()
    fr.add_raw(rnd(96))
    fr.add_compressed(Frame.lit_raw(b""), [(0, 4 + i % 60, 4) for i in range(1000)], last=True)
    emit("D/zero_literals", B, fr, True)
    for log, w in W_LOG.items():
        for fse_w in (False, True):
            if fse_w and len(w) < 3:
                continue
            for streams in (1, 4):
                n = 1023 if streams == 1 and log >= 11 else 600 + 37 * log
                fr = Frame()
                fr.add_compressed(fr.lit_huf(hlits(n, w), w, streams=streams, fse=fse_w), [(n, 4, B - n)], last=True)
                emit("D/huffman/log%d/%s/%d" % (log, "fse" if fse_w else "direct", streams), B, fr, True)
    for fmt in (2, 3):
        fr = Frame()
        fr.add_compressed(fr.lit_huf(hlits(40), hw, streams=4, fmt=fmt), [(40, 4, B - 40)], last=True)
        emit("D/huffman/header_fmt%d_small" % fmt, B, fr, True)
    for n in (4, 5, 6, 9):
        fr = Frame()
        fr.add_compressed(fr.lit_huf(hlits(16)[:n], hw, streams=4), [(n, 4, B - n)], last=True)
        emit("D/four_streams_%d" % n, B, fr, n != 5, fcs=B)   # 5: seg 2, 3 * seg > 5
    w11 = W_LOG[11]
    for n in (4095, 4096, 4097):
        seg = (n + 3) // 4
        data = bytes([0]) * seg + bytes([10 + (i & 1) for i in range(seg)]) + hlits(n - 2 * seg, w11)
        for j in range(2):
            fr = Frame()
            d = data if j == 0 else data[seg:2 * seg] + data[2 * seg:] + data[:seg]
            fr.add_compressed(fr.lit_huf(d, w11, streams=4), [(n, 4, 8192 - n)], last=True)
            emit("D/unequal_streams/%d/%d" % (n, j), 8192, fr, True)
    for name, kw in (("D/stream_last_byte_0", dict(zero_last=True)), ("D/stream_unread_bits", dict(trailing=3)),
                     ("D/jump_table_long", dict(jump=[300, 300, 300]))):
        for streams in (1, 4):
            if streams == 1 and "jump" in kw:
                continue
            for bad in ((1,) if streams == 1 or "jump" in kw else (0, 1, 3)):
                fr = Frame()
                fr.add_compressed(fr.lit_huf(hlits(600), hw, streams=streams, bad=bad, **kw), [(600, 4, B - 600)], last=True)
                emit("%s/%d/stream%d" % (name, streams, bad if streams == 4 else 0), B, fr, False)
    fr = Frame()
    fr.add_compressed(fr.lit_huf(hlits(600), hw, streams=4, jump=[150, 150, 65535]), [(600, 4, B - 600)], last=True)
    emit("D/jump_table_long/third_entry", B, fr, False)

    # ---------------- E. headers and block order
    few = [(5, 4, 3), (0, 3, 4), (2, 2, 3)]
    for Bh, nb in ((255, 1), (256, 2), (65791, 2), (B, 4), (B, 8), (B, 0)):
        one("E/fcs_%d_bytes/%d" % (nb, Bh), Bh, few, hdr=dict(fcs_bytes=nb, single=nb != 0, window=(2, 0)))
    one("E/fcs_wrong/short", B, few, declared=False, hdr=dict(fcs=B - 1))
    one("E/fcs_wrong/two_byte_form", B, few, declared=False, hdr=dict(fcs=B + 256, fcs_bytes=2))
    one("E/fcs_wrong/long", B, few, declared=False, hdr=dict(fcs=B + 1, fcs_bytes=8))
    for name, win in (("larger", (3, 5)), ("equal", (2, 0)), ("exp21_mantissa7", (21, 7))):
        one("E/window_" + name, B, few, hdr=dict(single=False, window=win, fcs_bytes=4))
    fr = Frame()
    for i in range(3):
        fr.add_raw(rnd(1024))
    block(fr, B, [(4, 4, 3), (0, 1000 + 3, 20)])             # every block and offset within a window of 1 KiB
    emit("E/window_smaller", B, fr, True, single=False, window=(0, 0), fcs_bytes=0)
    for m in (1, 7):
        one("E/window_exp22/mantissa%d" % m, B, few, declared=False, hdr=dict(single=False, window=(22, m), fcs_bytes=4))
    for nb in (1, 2, 4):
        one("E/dict_id_0/%d" % nb, B, few, hdr=dict(did_bytes=nb, did=0))
        one("E/dict_id_1/%d" % nb, B, few, declared=False, hdr=dict(did_bytes=nb, did=1))
    one("E/reserved_bit", B, few, declared=False, hdr=dict(reserved=1))
    one("E/unused_bit", B, few, hdr=dict(unused=1))
    fr = Frame()
    fr.add_raw(rnd(B), last=False)
    fr.add_reserved(b"", last=True)
    emit("E/block_type_3/last", B, fr, False, fcs=B)
    fr = Frame()
    fr.add_reserved(rnd(7), last=False)
    fr.add_raw(rnd(B), last=True)
    emit("E/block_type_3/first", B, fr, False, fcs=B)
    fr = Frame()
    block(fr, 1000, few, last=False)
    fr.add_reserved(b"", last=False)
    fr.add_rle(1, B - 1000, last=True)
    emit("E/block_type_3/middle", B, fr, False, fcs=B)
    kinds = ("raw", "rle", "comp")
    nbm = zstd_craft.zstd_nbmax(B)
    for nblk in (nbm, nbm + 1):
        for code in range(3 ** nblk):
            order = [kinds[(code // 3 ** i) % 3] for i in range(nblk)]
            fr = Frame()
            for i, kind in enumerate(order):
                last = i == nblk - 1
                size = B - len(fr.out) if last else 500 + 111 * i
                if kind == "raw":
                    fr.add_raw(rnd(size), last)
                elif kind == "rle":
                    fr.add_rle(0x20 + i, size, last)
                else:
                    block(fr, len(fr.out) + size, [(6, 4, 5), (1, 2, 3), (0, 3, 4)], last=last)
            emit("E/order%d/%s" % (nblk, "_".join(order)), B, fr, True)
    fr = Frame()
    block(fr, B, few, last=False)
    fr.add_raw(b"", last=True)
    emit("E/last_raw_block_of_0", B, fr, True)
    fr = Frame()
    fr.add_rle(0x77, B, last=True)
    emit("E/rle_block_of_B", B, fr, True)
    fr = Frame()
    block(fr, B, few)
    emit("E/behind_skippable", B, fr, True, frame=np.frombuffer(skippable(rnd(37), 3) + fr.frame().tobytes(), np.uint8).copy())
    f1, f2 = Frame(), Frame()
    block(f1, 1500, few)
    block(f2, B - 1500, few + few)
    emit("E/two_frames", B, f1, True, frame=np.concatenate([f1.frame(), f2.frame()]))
    emit("E/trailing_bytes/1", B, fr, False, frame=np.concatenate([fr.frame(), np.zeros(1, np.uint8)]))
    emit("E/trailing_bytes/4", B, fr, False, frame=np.concatenate([fr.frame(), np.frombuffer(MAGIC, np.uint8)]))
    one("E/checksum_right", B, few, hdr=dict(checksum=True))
    fr = Frame()
    block(fr, B, few)
    good = int.from_bytes(fr.frame(checksum=True)[-4:].tobytes(), "little")
    emit("E/checksum_wrong/bit", B, fr, False, checksum=good ^ (1 << int(rng.integers(0, 32))))
    emit("E/checksum_wrong/high_half", B, fr, False, checksum=(good + 0x10000) & 0xFFFFFFFF)
    return out


def crafted_corpus(seed):
    """[(name, B, frame, declared)]: declared True -- the library must accept the frame and the model's bytes are the block;
    False -- it must reject it.  Families A (repeat-offset history), B (counts and field widths), C (table modes),
    D (literals), E (headers and block order); names start with the family letter."""
    return [c[:4] for c in crafted_cases(seed)]
