"""Reference of the text group columns (include/cryo_codec.h, "Text group columns"), in plain Python: what a grouped call must
report when its descriptor carries CRYO_GROUP_TEXT and a group column is a byte string.  Written from the header's comment, not
from the kernel.  Test infrastructure only.

A group column is (att, type) with type BYTES for a varlena column.  The walk and the payload are bytes_key_ref's (walk,
stored_value: every read of a tuple goes through filter_ref.Tuple, which refuses any index outside the tuple); the keys of every
kind, the truth table and the cells are float_ref's, which is group_ref's on integer columns and plain keys.  A text value's key
is a Python bytes object, whose own ordering is the contract's: unsigned bytes over the shorter length, then the shorter first."""
import numpy as np

import bytes_key_ref as br
import float_ref as flr
import group_ref as gr
from filter_ref import OK, TUPLE

BYTES = br.BYTES
BUCKETS, TEXT = 1, 4                                    # cryo_group.rsv
TEXT_MAX = 32
UNDECIDED = br.UNDECIDED
KEY = np.dtype([("bytes", "u1", (32,)), ("len", "<u4"), ("rsv", "<u4")])     # cryo_group_key
AWAY = "undecided"                                      # a group value that is no key


def by_ok(atts, col, rsv):
    """the rule of one group column under the struct's rsv"""
    att, typ = col
    if typ == BYTES:
        return rsv == TEXT and 1 <= att <= len(atts) and atts[att - 1][0] == -1
    return flr.col_ok(atts, col, group=True)


def desc_ok(atts, keys, by, cols, rsv=TEXT, by_rsv=None):
    """the descriptor rules of a call without buckets: rsv the group struct's; cols None: a null aggregate descriptor; by_rsv:
    the group columns' reserved fields"""
    if rsv not in (0, TEXT) or not flr.desc_ok(atts, keys) or any(by_rsv or ()):
        return False
    if not 1 <= len(by) <= gr.MAX_BY or not all(by_ok(atts, c, rsv) for c in by):
        return False
    return cols is None or (len(cols) <= 4 and all(flr.col_ok(atts, c) for c in cols))      # BYTES is no aggregate column


def text_value(data, at):
    """the key of the non-NULL varlena at `at`: its in-line payload of at most TEXT_MAX bytes, or AWAY"""
    payload = br.stored_value(data, at)
    return AWAY if payload is None or len(payload) > TEXT_MAX else bytes(payload)


def tuple_values(data, atts, keys, cols, truth=None):
    """(TUPLE | NOMATCH | UNDECIDED | OK, [value per column of cols] when OK): a NULL None, an integer or float column its raw
    value, a BYTES column its bytes.  A tuple that passes the keys with a text value that is no key is UNDECIDED; one that
    fails them is NOMATCH whatever its values"""
    last = max([k[0] for k in keys] + [c[0] for c in cols], default=0)
    states = flr.key_states(data, atts, keys, last)
    if states is None:
        return TUPLE, None
    v = flr.tr.verdict_of(states, flr.and_table(len(keys)) if truth is None else truth)
    if v != OK:
        return v, None
    w = br.walk(data, atts, last)
    vals = []
    for att, typ in cols:
        isnull, at, _ = w[att - 1]
        vals.append(None if isnull else text_value(data, at) if typ == BYTES else flr._value(data, at, typ))
    return (UNDECIDED, None) if AWAY in vals else (OK, vals)


def _reduce(block, atts, keys, cols, truth):
    """float_ref._reduce with text values"""
    status, n, items = br._items(block)
    if status != OK:
        return (status, 0, 0, 0), []
    b = np.ascontiguousarray(block, dtype=np.uint8)
    n_bad, rows = 0, []
    for pos, bad, off, ln in items:
        if bad:
            n_bad += 1
            continue
        v, vals = tuple_values(b[off:off + ln].tobytes(), atts, keys, cols, truth)
        if v in (TUPLE, UNDECIDED):
            n_bad += 1
        elif v == OK:
            rows.append((pos, vals))
    return (OK, n, len(rows), n_bad), rows


def order_key(key):
    """what a block's groups are sorted by: NULL after every value; bytes by Python's ordering, integers by value"""
    return tuple((1,) if v is None else (0, v) for v in key)


def key_cell(value):
    """the cryo_group_key of a text value (None: NULL) as a tuple"""
    v = value or b""
    return (list(v) + [0] * (32 - len(v)), len(v), 0)


def group_call(blocks, atts, keys, by, cols, truth=None):
    """(rows, records, cells of shape (groups, ncols), total, key cells of shape (groups, ntext)) of a CRYO_GROUP_TEXT call, a
    multi-handle call included: blocks[i] a decoded block or None (a rejected stream)"""
    text = [j for j, (_, typ) in enumerate(by) if typ == BYTES]
    rows, recs, cells, kcells = np.zeros(len(blocks), gr.ROW), [], [], []
    for i, block in enumerate(blocks):
        row, matches = _reduce(block, atts, keys, list(by) + list(cols), truth)
        groups = {}
        for pos, m in matches:
            g = groups.setdefault(tuple(m[:len(by)]), [0, [[] for _ in cols]])
            g[0] += 1
            for j, v in enumerate(m[len(by):]):
                if v is not None:
                    g[1][j].append((pos, v))
        rows[i] = row + (len(groups), 0, len(recs))
        for key in sorted(groups, key=order_key):
            k = [0 if v is None else len(v) if isinstance(v, bytes) else v for v in key] + [0] * (2 - len(key))
            recs.append((k, groups[key][0], sum(1 << j for j, v in enumerate(key) if v is None)))
            cells.append([flr.cell_of(v, cols[j][1], True) for j, v in enumerate(groups[key][1])])
            kcells.append([key_cell(key[j]) for j in text])
    r = np.zeros(len(recs), gr.REC)
    c = np.zeros((len(recs), len(cols)), gr.CELL)
    kc = np.zeros((len(recs), len(text)), KEY)
    for g, rec in enumerate(recs):
        r[g] = rec
        for j, cell in enumerate(cells[g]):
            c[g, j] = cell
        for j, cell in enumerate(kcells[g]):
            kc[g, j] = cell
    return rows, r, c, len(recs), kc


def groups_of(result, by, i):
    """block i of a call's result -- the reference's or the library's -- read back as [(key tuple, n_rows)] in the order it has:
    None for NULL, an integer column's value, a text column's bytes taken from its key cell and its record's length"""
    rows, recs, _, _, kc = result
    text = [j for j, (_, typ) in enumerate(by) if typ == BYTES]
    out = []
    first, n = int(rows[i]["first_group"]), int(rows[i]["n_groups"])
    for g in range(first, first + n):
        key = []
        for j in range(len(by)):
            if int(recs[g]["nulls"]) >> j & 1:
                key.append(None)
            elif j in text:
                cell = kc[g, text.index(j)]
                assert int(cell["len"]) == int(recs[g]["key"][j]) and int(cell["rsv"]) == 0 and not cell["bytes"][int(cell["len"]):].any()
                key.append(bytes(cell["bytes"][:int(cell["len"])]))
            else:
                key.append(int(recs[g]["key"][j]))
        out.append((tuple(key), int(recs[g]["n_rows"])))
    return out
