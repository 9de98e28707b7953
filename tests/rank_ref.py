"""The reference's rank restated in Python, for the rank tests.

`rank_ref` is a literal reading of polars-ops/src/series/ops/rank.rs:68 rank:
the stable TotalOrd arg-sort with the nulls last (sort/arg_sort.rs:7 and the
swapped comparator of sort/mod.rs:71 for `descending`), the `neq` array of
consecutive sorted values (tot_ne), rank_impl (:49) and the five flush
closures (:113-:190), early returns included.  `starts` runs it on every
segment's rows, as Expr.over does (window.rs:356, GroupsToRows).

`rank_closed` is a vectorised numpy closed form of the same ranks, for inputs
too large for the loop; tests/test_rank.py pins the two to each other."""

import functools
import math

import numpy as np

METHODS = ("average", "min", "max", "dense", "ordinal")


def tot_cmp(a, b):
    """TotalOrd (polars-utils/src/total_ord.rs): NaN is the greatest value and
    equal to itself, -0.0 == 0.0."""
    an = isinstance(a, float) and math.isnan(a)
    bn = isinstance(b, float) and math.isnan(b)
    if an or bn:
        return int(an) - int(bn)
    return (a > b) - (a < b)


def arg_sort_ref(values, valid, descending):
    """Row ids of the non-null rows in sorted order (the reference sorts with
    nulls_last and slices the nulls off): a stable sort, so ties keep their
    row order ascending and descending alike."""
    cmp = (lambda i, j: tot_cmp(values[j], values[i])) if descending else (lambda i, j: tot_cmp(values[i], values[j]))
    return sorted((i for i in range(len(values)) if valid[i]), key=functools.cmp_to_key(cmp))


def rank_impl(idxs, neq, flush_ties):
    if not idxs:
        return
    ties = [idxs[0]]
    for eq_idx, idx in enumerate(idxs[1:]):
        if neq[eq_idx]:
            flush_ties(ties)
            ties = []
        ties.append(idx)
    flush_ties(ties)


def _rank_one(values, valid, method, descending):
    """rank.rs:68 on one column: (list of ranks, list of validity)."""
    n = len(values)
    null_count = sum(1 for v in valid if not v)
    if null_count == n:  # (also n == 0)
        return [0] * n, [False] * n
    if n == 1:
        return [1.0 if method == "average" else 1], [True]
    sort_idx = arg_sort_ref(values, valid, descending)
    out = [0.0 if method == "average" else 0] * n
    if method == "ordinal":
        rank = 0
        for i in sort_idx:
            out[i] = rank + 1
            rank += 1
        return out, list(valid)
    sv = [values[i] for i in sort_idx]
    neq = [tot_cmp(sv[k + 1], sv[k]) != 0 for k in range(len(sv) - 1)]
    state = {"rank": 1}

    def average(ties):
        first = state["rank"]
        state["rank"] += len(ties)
        last = state["rank"] - 1
        avg = 0.5 * (float(first) + float(last))
        for i in ties:
            out[i] = avg

    def rmin(ties):
        for i in ties:
            out[i] = state["rank"]
        state["rank"] += len(ties)

    def rmax(ties):
        state["rank"] += len(ties)
        for i in ties:
            out[i] = state["rank"] - 1

    def dense(ties):
        for i in ties:
            out[i] = state["rank"]
        state["rank"] += 1

    rank_impl(sort_idx, neq, {"average": average, "min": rmin, "max": rmax, "dense": dense}[method])
    return out, list(valid)


def _bounds(n, starts):
    if starts is None or n == 0:
        return [0, n]
    st = np.asarray(starts, bool).copy()
    st[0] = True
    return np.flatnonzero(st).tolist() + [n]


def rank_ref(values, valid, method="average", descending=False, starts=None):
    """(ranks, validity) as numpy arrays: uint32 ranks, float64 for "average";
    a null row's rank is 0.  `starts`: the ranks restart at every set row (the
    rows of a segment are one group in its row order)."""
    assert method in METHODS
    vals = list(values.tolist() if isinstance(values, np.ndarray) else values)
    ok_in = np.asarray(valid, bool).tolist()
    n = len(ok_in)
    out = np.zeros(n, np.float64 if method == "average" else np.uint32)
    ok = np.zeros(n, bool)
    bd = _bounds(n, starts)
    for a, b in zip(bd[:-1], bd[1:]):
        r, k = _rank_one(vals[a:b], ok_in[a:b], method, descending)
        out[a:b] = r
        ok[a:b] = k
    return out, ok


def rank_closed(values, valid, method="average", descending=False, groups=None):
    """One method of rank_closed_all."""
    assert method in METHODS
    return rank_closed_all(values, valid, descending, groups, (method,))[method]


def rank_closed_all(values, valid, descending=False, groups=None, methods=METHODS):
    """The same ranks in closed form, {method: (ranks, validity)} from one
    sort.  `groups`: one integer group id per row (any order, rows of a group
    need not be adjacent); None: one group.
    Sort the rows by (group, null, value) stably; with s the last group start,
    a the last tie start at or before sorted row j and b the next tie start
    after it: ordinal j - s + 1, min a - s + 1, max b - s, average the mean of
    min and max, dense the tie starts in [s, j]."""
    ok = np.asarray(valid, bool)
    res = ranks_from_starts(*sorted_inputs(values, ok, descending, groups), methods)
    return {m: (r, ok.copy()) for m, r in res.items()}


def sorted_inputs(values, valid, descending=False, groups=None):
    """(order, sorted validity, tie starts, segment starts): the rows stably
    sorted by (group, null, value), which sorted rows begin a run of equal
    (group, value) and which a group -- what plgpu_rank is given."""
    v = np.asarray(values)
    ok = np.asarray(valid, bool)
    n = len(ok)
    if n == 0:
        return np.zeros(0, np.int64), ok.copy(), ok.copy(), ok.copy()
    g = np.zeros(n, np.int64) if groups is None else np.asarray(groups, np.int64)
    if v.dtype.kind == "f":
        v = v + 0.0  # -0.0 -> 0.0; np.unique puts NaN last and, equal_nan, as one value
    code = np.unique(np.where(ok, v, v[ok][0] if ok.any() else v[0]), return_inverse=True)[1].reshape(-1).astype(np.int64)
    if descending:
        code = code.max() - code
    code = np.where(ok, code, 0)
    order = np.lexsort((code, ~ok, g))  # stable; the last key is the primary one
    sg, sn, sc = g[order], ~ok[order], code[order]
    seg = np.ones(n, bool)
    seg[1:] = sg[1:] != sg[:-1]
    tie = seg.copy()
    tie[1:] |= (sn[1:] != sn[:-1]) | (sc[1:] != sc[:-1])
    return order, ~sn, tie, seg


def ranks_from_starts(order, sorted_valid, tie, seg, methods=METHODS):
    """{method: ranks in row order} from the sorted layout alone: row 0 starts
    a segment and a segment start is a tie start, whatever the bitmaps say."""
    n = len(order)
    if n == 0:
        return {m: np.zeros(0, np.float64 if m == "average" else np.uint32) for m in methods}
    j = np.arange(n, dtype=np.int64)
    seg = np.asarray(seg, bool).copy()
    seg[0] = True
    tie = np.asarray(tie, bool) | seg
    sn = ~np.asarray(sorted_valid, bool)
    s = np.maximum.accumulate(np.where(seg, j, 0))
    a = np.maximum.accumulate(np.where(tie, j, 0))
    nxt = np.minimum.accumulate(np.where(tie, j, n)[::-1])[::-1]  # first tie start at or after j
    b = np.append(nxt[1:], n)
    cum = np.cumsum(tie)
    keep = ~sn
    res = {}
    for method in methods:
        if method == "ordinal":
            r = j - s + 1
        elif method == "min":
            r = a - s + 1
        elif method == "max":
            r = b - s
        elif method == "dense":
            r = cum - cum[s] + 1
        else:
            r = 0.5 * ((a - s + 1).astype(np.float64) + (b - s).astype(np.float64))
        out = np.zeros(n, np.float64 if method == "average" else np.uint32)
        out[order[keep]] = r[keep]
        res[method] = out
    return res
