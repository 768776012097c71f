"""The hand-made blocks of the text group column tests, shared by the CPU test (what tests/group_text_ref.py must say about them)
and the GPU tests (the kernels against group_text_ref on the same blocks).  The tuples are crafted with tests/tuple_craft.py over
the descriptor (id int4, t text, x int8, u text, d int4, f float8).  Test infrastructure only.

cases() yields (name, block, keys, by, cols, groups, n_bad): groups the block's [(key tuple, n_rows)] in the contract's order
-- None a NULL, bytes a text value, an integer an integer column's value --, written out by hand or, for the sweeps, taken
from Python's own ordering of bytes objects, which is the contract's and shares no code with the reference."""
import bytes_key_cases as bkc
import bytes_key_ref as br
import tuple_craft as tc
from filter_ref import EQ, INT4, INT8
from tuple_craft import Long, Toast

B = bkc.B
ATTS = [(4, 4), (-1, 4), (8, 8), (-1, 4), (4, 4), (8, 8)]
T_, X, U, D = (2, br.BYTES), (3, INT8), (4, br.BYTES), (5, INT4)
EDGES = (7, 8, 15, 16, 23, 24, 31)
LENGTHS = (0, 1, 7, 8, 9, 31, 32)


def T(*values):
    return tc.form_tuple(ATTS, list(values))


def block(tuples, size=B):
    return tc.build_block(size, tuples)


def edge_values():
    """32 bytes and, for every edge of a word, the same with that byte one higher: they differ in that byte alone"""
    base = bkc.pattern(32)
    return [base] + [base[:k] + bytes([(base[k] + 1) % 256]) + base[k + 1:] for k in EDGES]


def cases():
    out = []

    def add(name, tuples, keys, by, cols, groups, n_bad=0):
        out.append((name, block(tuples), keys, by, cols, groups, n_bad))

    add("'' is a value, NULL is not", [T(1, b"", 5), T(2, None, 5), T(3, b"", 6), T(4, None, 7), T(5, Long(b""), 8)], [], [T_], [X],
        [((b"",), 3), ((None,), 2)])
    add("a prefix sorts first, a zero byte counts", [T(1, b"abc", 1), T(2, b"ab\0", 1), T(3, b"ab", 1), T(4, Long(b"ab"), 1), T(5, b"a", 1)],
        [], [T_], [], [((b"a",), 1), ((b"ab",), 2), ((b"ab\0",), 1), ((b"abc",), 1)])
    add("bytes are unsigned", [T(1, b"\xff", 1), T(2, b"\x80", 1), T(3, b"\x7f", 1), T(4, b"\x00", 1), T(5, b"\x80", 1)], [], [T_], [X],
        [((b"\x00",), 1), ((b"\x7f",), 1), ((b"\x80",), 2), ((b"\xff",), 1)])
    vals = edge_values()
    assert len(set(vals)) == 8
    add("keys that differ at one byte on a word's edge", [T(i, v, i) for i, v in enumerate(vals + vals[::-1])], [], [T_], [X],
        [((v,), 2) for v in sorted(vals)])
    # every length that is a key under both headers; 33 bytes, a pointer and a compressed value are none
    z = b"z" * 20
    lens = [T(n, b"a" * n, 1) for n in LENGTHS] + [T(n, Long(b"a" * n), 2) for n in LENGTHS]
    lens += [T(33, b"a" * 33, 3), T(34, Toast(), 3), bkc.compressed(T(35, Long(z), 3), z), T(36, Long(b"a" * 33), 3)]
    add("lengths 0 .. 32 are keys, what is longer or away is undecided", lens, [], [T_], [X], [((b"a" * n,), 2) for n in LENGTHS], 4)
    add("an undecided value on a tuple that fails the keys is not bad",
        [T(1, Toast(), 11), T(2, Toast(), 10), T(3, b"a", 10), T(4, b"a" * 40, 12), T(5, b"a" * 40, 10), T(6, None, 10)],
        [(3, INT8, EQ, 10)], [T_], [X], [((b"a",), 1), ((None,), 1)], 2)
    two = [T(1, b"de", 1, b"x", 7), T(2, b"de", 1, b"y", 7), T(3, b"de", 1, b"x", 8), T(4, b"fr", 1, None, 7), T(5, None, 1, b"x", None),
           T(6, b"de", 1, b"x", 7), T(7, None, 1, None, None), T(8, b"fr", 1, Toast(), 7)]
    add("text, then int", two, [], [T_, D], [X], [((b"de", 7), 3), ((b"de", 8), 1), ((b"fr", 7), 2), ((None, None), 2)])
    add("int, then text", two, [], [D, T_], [X], [((7, b"de"), 3), ((7, b"fr"), 2), ((8, b"de"), 1), ((None, None), 2)])
    add("text, then text", two, [], [T_, U], [X],
        [((b"de", b"x"), 3), ((b"de", b"y"), 1), ((b"fr", None), 1), ((None, b"x"), 1), ((None, None), 1)], 1)
    add("a column beyond the tuple's natts is NULL", [T(1, b"a", 10), T(2, b"a", 10, b"u"), T(3, b"b"), T(4)], [], [U, T_], [X],
        [((b"u", b"a"), 1), ((None, b"a"), 1), ((None, b"b"), 1), ((None, None), 1)])
    return out
