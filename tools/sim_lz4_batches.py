#!/usr/bin/env python3
"""Design aid (CPU only, uses the oracle as a data source): what the batches of the indexed LZ4 decoder look like.

Models the batching of k_lz4_dec_seq (csrc/lz4_dec2.hip: lz4_seq_batch and the loop around it) on oracle-encoded blocks:
a batch is up to 64 consecutive sequences and 1 536 output bytes inside a window of 1 536 compressed bytes, and it ends in
front of a sequence it cannot take.  No timing: only the counts the copy engine's cost depends on (csrc/lz4_copy.h).

Prints, per distribution:
  sequences, literal bytes and match bytes per batch;
  dependent matches (source inside the batch), their bytes, and chunks of 64 bytes of match space per batch;
  the share of batches in which lane_runs takes a second turn of the whole wave, when a run with exactly 16 bytes left
  takes one (rem >= 16) and when it is left to the closing 16-byte copy (rem > 16; far runs keep >= 16);
  the hard stops per block (sequences no batch takes wherever it begins) with their sequence numbers.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from oracle_lib import Oracle  # noqa: E402

R, T_MAX, SEQ_WIN, OVL_MAX = 4096, 1536, 1536, 64
NEAR = R - T_MAX
NAMES = ["wide", "narrow", "int4", "random", "zeros"]


def parse(c):
    """[(pos, ll, off, ml, dlen, ll255, ml255)] of every sequence with a match, then the position of the last token.
    ll255 / ml255: the length's first extension byte is 255 (the batch decoder reads one extension byte)."""
    n, p, out = len(c), 0, []
    while True:
        t = c[p]
        ll, q = t >> 4, p + 1
        ll255 = ll == 15 and c[q] == 255
        if ll == 15:
            while True:
                b = c[q]
                q += 1
                ll += b
                if b != 255:
                    break
        q += ll
        if q >= n:
            return out, p
        off = c[q] | (c[q + 1] << 8)
        q += 2
        ml = (t & 15) + 4
        ml255 = (t & 15) == 15 and c[q] == 255
        if (t & 15) == 15:
            while True:
                b = c[q]
                q += 1
                ml += b
                if b != 255:
                    break
        out.append((p, ll, off, ml, q - p, ll255, ml255))
        p = q


def never(s):
    """a sequence no batch takes, wherever it begins"""
    _, _, off, ml, _, ll255, ml255 = s
    return ll255 or ml255 or (off < ml and ml > OVL_MAX) or (off >= NEAR and ml > 32)


def batch(seqs, i, op, csize, B):
    """sequences the batch that starts at seqs[i] takes (0: none), as lz4_seq_batch validates them"""
    vsafe = csize - 16
    vp = seqs[i][0]
    if vp + 64 > vsafe or op + 64 > B:
        return 0
    oend, n = 0, 0
    while n < 64 and i + n < len(seqs):
        pos, ll, off, ml, dlen, ll255, ml255 = seqs[i + n]
        k = 2 if ll >= 15 else 1
        q = pos + k + ll
        far = off >= NEAR
        ok = (pos + 8 <= vp + SEQ_WIN and q + 8 <= vp + SEQ_WIN and not ll255 and not ml255
              and (off >= ml or (off != 0 and ml <= OVL_MAX)) and off <= op + oend + ll and pos + dlen <= vsafe
              and oend + ll + ml <= T_MAX and op + oend + ll + ml + 16 <= B and not (far and ml > 32))
        if not ok:
            break
        oend += ll + ml
        n += 1
    return n


def second_turn(ll, ml, indep, far, part2):
    """does this lane keep the wave in lane_runs for a second 16-byte turn?"""
    def run(rem, is_far):
        if rem < 16:
            return False
        rem -= 16
        return rem >= 16 if (is_far or not part2) else rem > 16
    return run(ll, False) or (indep and run(ml, far))


def main():
    o = Oracle()
    B, nblk = 131072, 6
    for dist in (0, 1, 2):
        per = {k: [] for k in ("seqs", "lit", "mat", "dep", "depbytes", "chunks", "turn_old", "turn_new", "depth")}
        stops, general, zero_old, zero_new = [], 0, 0, 0
        for blk in range(nblk):
            c = o.lz4_compress(o.synth(0, blk, B, dist), 1).tolist()
            seqs, _ = parse(c)
            i, op, hard_here = 0, 0, []
            while i < len(seqs):
                n = batch(seqs, i, op, len(c), B)
                if n:
                    lit = mat = dep = depb = 0
                    t_old = t_new = False
                    o0, ready = 0, {}
                    depth = 0
                    for pos, ll, off, ml, dlen, _, _ in seqs[i:i + n]:
                        mrel = o0 + ll
                        far = off >= NEAR
                        indep = far or off >= mrel + ml
                        lit += ll
                        mat += ml
                        if not indep:
                            dep += 1
                            depb += ml
                            # dependency level: 1 + the deepest dependent match its source bytes lie in
                            lv = 1 + max([v for (a, b), v in ready.items() if a < mrel - off + min(ml, off) and mrel - off < b] or [0])
                            ready[(mrel, mrel + ml)] = lv
                            depth = max(depth, lv)
                        t_old |= second_turn(ll, ml, indep, far, False)
                        t_new |= second_turn(ll, ml, indep, far, True)
                        o0 += ll + ml
                    for k, v in (("seqs", n), ("lit", lit), ("mat", mat), ("dep", dep), ("depbytes", depb),
                                 ("chunks", (depb + 63) // 64), ("turn_old", t_old), ("turn_new", t_new), ("depth", depth)):
                        per[k].append(v)
                    op += o0
                    i += n
                    if n >= 8 and i < len(seqs):
                        if never(seqs[i]):       # part 3: straight to the general path
                            hard_here.append(i)
                            zero_old += 1
                        else:
                            continue
                else:
                    zero_old += 1
                    zero_new += 1
                    if i < len(seqs) and never(seqs[i]):
                        hard_here.append(i)
                if i < len(seqs):               # one sequence through the general path
                    op += seqs[i][1] + seqs[i][3]
                    i += 1
                    general += 1
            general += 1                        # the block's last sequence (literals only)
            stops.append(hard_here)
        m = {k: float(np.mean(v)) for k, v in per.items()}
        nb = len(per["seqs"])
        print(f"{NAMES[dist]}: {nblk} blocks of {B} bytes, {nb / nblk:.1f} batches per block")
        print(f"   per batch: sequences {m['seqs']:.1f}, literal bytes {m['lit']:.0f}, match bytes {m['mat']:.0f}")
        print(f"   per batch: dependent matches {m['dep']:.1f} ({m['depbytes']:.0f} bytes), chunks of match space {m['chunks']:.2f}, "
              f"dependency depth {m['depth']:.1f}")
        print(f"   batches with a second lane_runs turn: {100 * m['turn_old']:.1f} % at rem >= 16, {100 * m['turn_new']:.1f} % at rem > 16")
        print(f"   per block: general-path sequences {general / nblk:.1f}, empty batches {zero_old / nblk:.1f} -> {zero_new / nblk:.1f} "
              f"with hard stops taken directly")
        print("   hard stops (sequence numbers per block): " + "; ".join(",".join(map(str, s)) or "-" for s in stops))


if __name__ == "__main__":
    main()
