"""Crafted LZ4 block streams for decoder conformance tests (test infrastructure).

liblz4's encoder never writes much of what LZ4_decompress_safe accepts or rejects by explicit rule: a last match that
ends 12, 6, 5 or 4 bytes before the block end, offset 0, an offset equal to or one past the bytes written so far,
length-extension bytes next to the input end, literal-only blocks of a few KiB.  This module writes streams at the
sequence level -- a list of (literal length, offset, match length) and a last sequence of literals only -- with every
value drawn from boundary menus (token nibble 15, the edges of the 255-extension runs), ends steered onto the decoder's
rules, and compressed sizes steered onto the routing thresholds of kernels.h (lz4_literal_heavy: B - B/16;
lz4_index_one_walker: 16 384) and onto long runs at index segment cuts.

The truth for a stream is the oracle at capacity B (accepted when it returns B); this module only writes bytes.
Deterministic for a given seed."""
import numpy as np

LIT_MENU = [0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526]
LIT_LONG = [3000, 5000, 9000]                        # several 1 KiB index segments of one literal run
ML_MENU = [4, 5, 18, 19, 20, 273, 274, 275, 528, 529, 530]
ML_LONG = [20000, 40000, 65000]                      # 255-runs of match length
OFF_MENU = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 1023, 1024, 4095, 4096,
            32767, 32768, 65534, 65535]
ENDS = ["tail_exact", "match_end_12", "match_end_6", "match_end_5", "match_end_4", "match_end_0",
        "tail_short", "tail_long"]

_POOL = np.random.default_rng(0x1a4).integers(0, 256, 1 << 21, dtype=np.uint8).tobytes()


def _ext(n):
    """the 255-run that carries n beyond the nibble's 15"""
    return b"\xff" * (n // 255) + bytes([n % 255])


def encode(seqs, last_ll, lit_seed=0):
    """seqs: [(ll, off, ml)] (ml >= 4), then a last sequence of last_ll literals -> bytes.  Literal bytes are slices of a
    fixed random pool; lit_seed picks where."""
    out = bytearray()
    p = (lit_seed * 7919) % (len(_POOL) // 2)
    for ll, off, ml in seqs:
        m = ml - 4
        out.append((min(ll, 15) << 4) | min(m, 15))
        if ll >= 15:
            out += _ext(ll - 15)
        out += _POOL[p:p + ll]
        p = (p + ll) % (len(_POOL) // 2)
        out += bytes([off & 255, (off >> 8) & 255])
        if m >= 15:
            out += _ext(m - 15)
    out.append(min(last_ll, 15) << 4)
    if last_ll >= 15:
        out += _ext(last_ll - 15)
    out += _POOL[p:p + last_ll]
    return out


def csize_of(seqs, last_ll):
    n = 1 + last_ll + ((last_ll - 15) // 255 + 1 if last_ll >= 15 else 0)
    for ll, _, ml in seqs:
        n += 3 + ll + ((ll - 15) // 255 + 1 if ll >= 15 else 0) + ((ml - 19) // 255 + 1 if ml >= 19 else 0)
    return n


class _Gen:
    def __init__(self, rng, B):
        self.rng, self.B = rng, B
        self.p_long = 0.02 if B <= 32768 else (0.08 if B <= 300001 else 0.25)

    def pick(self, menu, long):
        r = self.rng
        if long and r.random() < self.p_long:
            return int(r.choice(long))
        return int(r.choice(menu))

    def offset(self, op):
        """mostly a menu value the output so far can serve; rarely 0, exactly op, op + 1; overlap (off < ml) is common"""
        r = self.rng
        u = r.random()
        if u < 0.02:
            return 0
        if u < 0.04:
            return min(op, 65535)
        if u < 0.06:
            return min(op + 1, 65535)
        ok = [o for o in OFF_MENU if o <= op]
        if not ok or r.random() < 0.03:
            return int(r.choice(OFF_MENU))
        return int(r.choice(ok[-6:] if r.random() < 0.3 else ok))

    def body(self, reserve):
        """sequences until the next one would pass B - reserve; returns (seqs, op)"""
        seqs, op, B = [], 0, self.B
        while True:
            ll = self.pick(LIT_MENU, LIT_LONG)
            if op == 0 and ll == 0:
                ll = 1
            ml = self.pick(ML_MENU, ML_LONG)
            if op + ll + ml > B - reserve:
                return seqs, op
            seqs.append((ll, self.offset(op + ll), ml))
            op += ll + ml

    def end(self, seqs, op, kind):
        """close the block: returns the last literal run (and may append a last match)"""
        B, r = self.B, self.rng
        if kind.startswith("match_end_"):
            t = int(kind[len("match_end_"):])
            rem = B - t - op
            ll = min(int(r.choice([0, 1, 14, 15, 16])), max(rem - 4, 0))
            if op + ll == 0:
                ll = 1
            if rem - ll >= 4:
                seqs.append((ll, self.offset(op + ll), rem - ll))
                return t
            return B - op
        if kind == "tail_short":
            return max(B - op - 1, 0)
        if kind == "tail_long":
            return B - op + 1
        return B - op


def steer(seqs, last_ll, target, rng):
    """move bytes between a sequence's literals and its match (the decoded size stays) until the stream is `target` bytes
    long; offsets that the shorter literal runs no longer cover are clipped.  Returns the new list (maybe not exact)."""
    seqs = [list(s) for s in seqs]
    if not seqs:
        return seqs
    for _ in range(24):
        d = target - csize_of(seqs, last_ll)
        if d == 0:
            break
        order = rng.permutation(len(seqs))
        for j in order:
            ll, off, ml = seqs[j]
            if d > 0 and ml > 4:
                k = min(d, ml - 4)
                seqs[j] = [ll + k, off, ml - k]
                d -= k
            elif d < 0 and ll > 1:
                k = min(-d, ll - 1)
                op = sum(a + c for a, _, c in seqs[:j]) + ll - k
                seqs[j] = [ll - k, min(off, op) if off else 0, ml + k]
                d += k
            if d == 0:
                break
    return [tuple(s) for s in seqs]


def _post(b, rng, kind):
    if kind == "trunc":
        return b[:max(1, len(b) - int(rng.integers(1, 4)))]
    if kind == "trailing":
        return b + bytes([int(rng.integers(0, 256))])
    return b


def stream(rng, B, end=None, target=None, post=None):
    """one crafted stream of a block of B bytes: (name, bytes)"""
    g = _Gen(rng, B)
    end = end or str(rng.choice(ENDS))
    seqs, op = g.body(reserve=int(rng.choice([16, 64, 600])))
    last = g.end(seqs, op, end)
    if target is not None:
        seqs = steer(seqs, last, target, rng)
    post = post or str(rng.choice(["none"] * 8 + ["trunc", "trailing"]))
    b = _post(bytes(encode(seqs, last, lit_seed=int(rng.integers(0, 1 << 30)))), rng, post)
    return "%s/%s%s" % (end, post, "" if target is None else "/csize%d" % target), b


def run_at_cut(rng, B):
    """one literal run, one long match whose 255-run straddles the middle of the stream (where an index walker of two, and
    the walkers around it of more, start on a guess), one literal tail; the stream is >= 16 384 bytes (several walkers)"""
    half = 8000 + int(rng.integers(0, 400))
    t = half + int(rng.integers(-40, 40))
    ml = B - half - t
    seqs = [(half, int(rng.choice([1, 3, 8, 64, 4096])), ml)]
    return "run_at_cut", bytes(encode(seqs, t, lit_seed=int(rng.integers(0, 1 << 30))))


def corpus(B, n, seed):
    """n crafted streams for blocks of B bytes: about a third steered onto the routing thresholds, the rest free"""
    rng = np.random.default_rng([seed, B])
    heavy = B - (B >> 4)
    targets = [heavy - 1, heavy, heavy + 1]
    if B > 16384 + 64:
        targets += [16383, 16384]
    out = []
    for i in range(n):
        u = i % 12
        if u < 3:
            out.append(stream(rng, B, end=str(rng.choice(["tail_exact", "match_end_5", "match_end_12", "match_end_4"])),
                              target=targets[i % len(targets)], post="none"))
        elif u == 3 and B >= 131072:
            out.append(run_at_cut(rng, B))
        else:
            out.append(stream(rng, B))
    return [(name, np.frombuffer(b, np.uint8).copy()) for name, b in out]
