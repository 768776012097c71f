"""The calls the walk tests make of the newer kernels and routes on the wide tuples of tests/walk_gen.py: which calls a plan
gives under a route, the reference of a call, the check of a result against the construction -- shared by tests/test_walk_cpu.py
(the references' results) and tests/test_gpu_walk_routes.py (the library's) --, and the device-resident and host-buffer forms of
the text and bucket grouping over any descriptor.  Test infrastructure only.

A call is (kind, keys, truth, args): kind one of KINDS; args the aggregate columns, (by, cols), the projected columns,
(by, limit, cols), (by, cols) or (by, cols, buckets)."""
import bucket_ref as bk
import float_ref as flr
import group_text_ref as gt
import like_ref as lr
import set_key_ref as sr
import topn_ref as tn
import walk_gen as wg

KINDS = ["filter", "agg", "group", "project", "topn", "group_text", "group_bucket"]
NEW_KINDS = ["topn", "group_text", "group_bucket"]
ROUTES = ["float", "like", "table"]
PLAIN_KEYSETS = (0, 1, 3)


# ---- what a plan gives ----
def matches_of(case, blk, keys, truth=None):
    """by construction: how many of a block's uncut items match"""
    return sum(1 for i, cut in blk.items if wg.expect_match(case.rows[i], keys, truth) is True)


def limits(case, blks, keys, truth=None):
    """1, one below block 0's match count, that count, and more than a block holds"""
    m = matches_of(case, blks[0], keys, truth)
    return (1, max(1, m - 1), max(1, m), 1000)


def keysets_of(plan, route):
    """[(keys, truth)] of a route"""
    if route == "plain":
        return [(plan.keysets[i], None) for i in PLAIN_KEYSETS]
    if route == "float":
        return [(k, None) for k in plan.float_keysets]
    if route == "like":
        return [(k, None) for k in plan.like_keysets]
    return [(plan.set_keysets[0], None), (plan.set_keysets[3], None), (plan.table_keys, plan.table)]


def all_keysets(plan):
    """every key set a route uses, and the two set keys the table route leaves out"""
    out = [ks for route in ["plain"] + ROUTES for ks in keysets_of(plan, route)]
    return out + [(plan.set_keysets[1], None), (plan.set_keysets[2], None)]


def runs(plan, kind, route):
    """whether the plan's descriptor can carry the call under the route"""
    if route == "float" and not plan.float_col:
        return False
    if route == "like" and not plan.text_col:
        return False
    return kind != "group_text" or bool(plan.text_col)


def topn_calls(case, blks, plan, keys, truth, float_by=False, short=False):
    """the ordered calls of one key set: the plan's pairing of order specs, column lists and kinds of limit; short: the first
    and the last pairing alone; float_by: the float order specs over the widest column lists"""
    lim = limits(case, blks, keys, truth)
    if float_by:
        return [("topn", keys, truth, (by, lim[1 + j], plan.topn_cols[-1 - j])) for j, by in enumerate(plan.topn_float_by)]
    pairs = plan.topn_calls if not short else [plan.topn_calls[1], plan.topn_calls[len(plan.topn_cols) - 1]]
    return [("topn", keys, truth, (plan.topn_by[b], lim[k], plan.topn_cols[c])) for b, c, k in pairs]


def calls(case, blks, plan, kind, route, short=False):
    """the calls of one kind under a route"""
    fagg = [plan.float_agg] if route == "float" else []
    out = []
    for n, (keys, truth) in enumerate(keysets_of(plan, route)):
        if kind == "filter":
            out.append((kind, keys, truth, ()))
        elif kind == "agg":
            out.append((kind, keys, truth, plan.agg_cols[:3] + fagg if fagg else plan.agg_cols))
        elif kind == "group":
            out.append((kind, keys, truth, (plan.by, plan.group_cols[:3] + fagg if fagg else plan.group_cols)))
        elif kind == "project":
            out.append((kind, keys, truth, plan.project_cols))
        elif kind == "topn":
            out += topn_calls(case, blks, plan, keys, truth, route == "float", short or route != "plain")
        elif kind == "group_text":
            out += [(kind, keys, truth, (by, plan.group_cols[:2] + fagg)) for by in plan.text_by]
        else:
            picked = plan.buckets if route == "plain" and not short else [plan.buckets[n % len(plan.buckets)]]
            out += [(kind, keys, truth, (by, plan.group_cols[:2] + fagg, buckets)) for by, buckets in picked]
    return out


# ---- a call's reference and its check ----
def reference(blocks, atts, call, route="like"):
    """the reference's result: the module that states the call's rules where the route's keys are its own, like_ref -- which
    knows every kind of key -- otherwise"""
    kind, keys, truth, args = call
    if kind == "topn":
        return (tn if route in ("plain", "float", "table") else lr).topn_call(blocks, atts, keys, *args, truth)
    if kind == "group_text":
        return gt.group_call(blocks, atts, keys, *args, truth) if route != "like" else lr.text_group_call(blocks, atts, keys, *args, truth)
    if kind == "group_bucket":
        return bk.group_call(blocks, atts, keys, *args, truth) if route != "like" else lr.bucket_group_call(blocks, atts, keys, *args, truth)
    if route == "table" and truth is None:
        if kind == "filter":
            return sr.filter_call(blocks, atts, keys)
        if kind == "group":
            return sr.group_call(blocks, atts, keys, *args)
        return (sr.agg_call if kind == "agg" else sr.project_call)(blocks, atts, keys, args)
    mod = lr if route == "like" else flr
    if kind == "filter":
        return mod.filter_call(blocks, atts, keys, 0, truth)
    if kind == "group":
        return mod.group_call(blocks, atts, keys, *args, truth)
    return (mod.agg_call if kind == "agg" else mod.project_call)(blocks, atts, keys, args, truth)


def check(case, blks, call, result, what=""):
    """a result -- a reference's or the library's -- against the construction"""
    kind, keys, truth, args = call
    what = (what, case.name, kind, keys, truth, args)
    if kind == "filter":
        wg.check_filter(case, blks, keys, result, what, truth)
    elif kind == "agg":
        wg.check_agg(case, blks, keys, args, result, what, truth)
    elif kind == "group":
        wg.check_group(case, blks, keys, *args, result, what, truth)
    elif kind == "project":
        wg.check_project(case, blks, keys, args, result, what, truth)
    elif kind == "topn":
        wg.check_topn(case, blks, keys, *args, result, what, truth)
    elif kind == "group_text":
        wg.check_group_text(case, blks, keys, *args, result, what, truth)
    else:
        wg.check_group_bucket(case, blks, keys, *args, result, what, truth)
