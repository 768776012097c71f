"""CPU: the rule by which the LZ4 / zstd copy engine (csrc/lz4_copy.h, seq_copy) gets the per-chunk bases of match space.

Match space is the bytes of a batch's dependent matches, concatenated in order.  Match r starts at mcum[r] and the engine
sets bit mcum[r] - 1 of a bitmap for every match that starts at a position >= 1, so the number of set bits below a position
is the rank of the match that position belongs to.  The base of chunk c is the number of set bits below byte 64c.  The
engine does not count them: the match that contains byte 64c writes its own rank.  The two must agree for every chunk below
the total, whatever the matches' lengths."""
import numpy as np
import pytest

TMAX = 1536


def _bases_by_popcount(mcum, total):
    bits = np.zeros(TMAX, np.int64)
    for s in mcum:
        if s >= 1:
            assert bits[s - 1] == 0, "two matches start at one position"
            bits[s - 1] = 1
    prefix = np.concatenate([[0], np.cumsum(bits)])      # prefix[p] = set bits below p
    return [int(prefix[64 * c]) for c in range((total + 63) // 64)]


def _bases_by_rank(mcum, ml, total):
    """what the lanes write: rank r for every c with mcum[r] <= 64c < mcum[r] + ml[r], first c = (mcum + 63) >> 6"""
    out = {}
    for r, (s, n) in enumerate(zip(mcum, ml)):
        c = (s + 63) >> 6
        while 64 * c < s + n:
            assert c not in out, "two matches claim one boundary"
            out[c] = r
            c += 1
    nchunks = (total + 63) // 64
    assert sorted(out) == list(range(nchunks)), "every chunk below the total gets a base, and no other"
    return [out[c] for c in range(nchunks)]


def _check(ml):
    ml = [int(x) for x in ml]
    mcum = [int(x) for x in np.concatenate([[0], np.cumsum(ml)[:-1]])] if ml else []
    total = sum(ml)
    assert total <= TMAX
    assert _bases_by_rank(mcum, ml, total) == _bases_by_popcount(mcum, total), (ml,)


def _random_lengths(rng, lo, hi, total_cap=TMAX, nmax=64):
    ml, left = [], total_cap
    while len(ml) < nmax and left >= lo:
        n = int(rng.integers(lo, min(hi, left) + 1))
        ml.append(n)
        left -= n
    return ml


@pytest.mark.parametrize("seed", range(20))
def test_rank_of_the_match_at_a_boundary_is_the_popcount_prefix(seed):
    rng = np.random.default_rng(seed)
    _check(_random_lengths(rng, 3, 12))                      # LZ4's usual matches, zstd's 3-byte ones
    _check(_random_lengths(rng, 4, 64, total_cap=int(rng.integers(4, TMAX + 1))))
    _check(_random_lengths(rng, 3, 300, nmax=int(rng.integers(1, 65))))


def test_a_match_at_position_zero_sets_no_bit_and_has_rank_zero():
    _check([4])
    _check([64])
    _check([65])
    _check([1536])
    _check([200, 4, 4])


@pytest.mark.parametrize("n", [65, 127, 128, 129, 273, 1000])
def test_matches_longer_than_a_chunk_claim_every_boundary_inside_them(n):
    for lead in (0, 1, 4, 63, 64, 65):
        _check(([lead] if lead >= 3 else ([4] if lead else [])) + [n, 5])
        _check([60, n])


@pytest.mark.parametrize("total", [64, 128, 192, 1536])
def test_totals_that_are_multiples_of_a_chunk(total):
    _check([total])
    _check([4] * (total // 4) if total // 4 <= 64 else [24] * (total // 24))
    rng = np.random.default_rng(total)
    for _ in range(20):
        ml = _random_lengths(rng, 3, 40, total_cap=total - 3)
        ml.append(total - sum(ml))
        _check(ml)
    # a match that ends exactly on a boundary, one that starts exactly on it
    _check([60, 4, 8])
    _check([64, 8])
    _check([62, 4, 8])      # the boundary falls inside a 4-byte match
