"""The reference's as-of join restated in Python, for the join_asof tests.

Two independent readings, both returning (rows, ok): `rows[i]` is the right row
matched to left row i (int64, -1 where `ok[i]` is False).

`asof_ref_scan`    a literal reading of the three AsofJoinState::next machines
                   (polars-ops/src/frame/join/asof/mod.rs:46-199), of
                   join_asof_impl and the tolerance filter (default.rs:11, :126)
                   and of asof_in_group (groups.rs:38): one running state per
                   group, keyed by the group's first right row, the left rows
                   taken in order.  It needs what the reference needs: left keys
                   ascending (within each group), right keys ascending.
`asof_ref_bounds`  the closed forms over the non-null right keys of a row's
                   group, with numpy.searchsorted: lb(x) the first position
                   whose value is >= x, ub(x) the first whose value is > x.

Where both differ from the reference, on purpose (DESIGN.md "As-of join"):
  * float keys compare by TotalOrd (NaN greatest and equal to itself, -0.0 ==
    0.0) where the reference uses partial_cmp / == ; marked "TotalOrd" below;
  * with `by`, a right row whose `on` is null is left out of its group wherever
    it stands (the reference's single numeric `by` path reads such a row's value
    slot, groups.rs:101-110); marked "null on" below.

Keys are numpy arrays of one dtype (integers or floats); a validity is a bool
array or None; `by_left` / `by_right` are lists of columns, each a list or
array of hashable values with None for null.  abs_diff is exact for integers
(Python integers) and rounded in the key's own type for floats."""

import numpy as np


# ------------------------------------------------------------------ order
def _is_float(a):
    return np.asarray(a).dtype.kind == "f"


def _nan(x):
    return isinstance(x, (float, np.floating)) and x != x


def _lt(a, b):
    """a < b.  TotalOrd: NaN is the greatest value."""
    if _nan(a):
        return False
    if _nan(b):
        return True
    return a < b


def _eq(a, b):
    """a == b.  TotalOrd: NaN equals NaN."""
    if _nan(a) or _nan(b):
        return _nan(a) and _nan(b)
    return a == b


def _abs_diff(a, b):
    if isinstance(a, np.floating):
        with np.errstate(invalid="ignore", over="ignore"):
            return abs(a - b)  # in the key's own float type
    return abs(int(a) - int(b))


def _abs_tol(tolerance, dtype):
    if tolerance is None:
        return None
    if dtype.kind == "f":
        return abs(dtype.type(tolerance))
    return abs(int(tolerance))


def _scalar(v):
    return v if isinstance(v, np.floating) else int(v)


# ------------------------------------------------------------------ groups
def _codes(by_left, by_right, n_left, n_right):
    """One int64 code per row and side for its `by` tuple, -1 where the tuple
    holds a null; equal tuples get equal codes on both sides."""
    lc, rc = np.zeros(n_left, np.int64), np.zeros(n_right, np.int64)
    lnull, rnull = np.zeros(n_left, bool), np.zeros(n_right, bool)
    for cl, cr in zip(by_left, by_right):
        both = list(cl) + list(cr)
        null = np.array([v is None for v in both], bool)
        vals = np.array([0 if v is None else v for v in both]) if not any(isinstance(v, str) for v in both) \
            else np.array(["" if v is None else v for v in both])
        _, inv = np.unique(vals, return_inverse=True)
        inv = inv.astype(np.int64).reshape(-1)
        m = int(inv.max()) + 1 if len(inv) else 1
        pair = np.concatenate([lc, rc]) * m + inv
        _, pair = np.unique(pair, return_inverse=True)
        pair = pair.astype(np.int64).reshape(-1)
        lc, rc = pair[:n_left], pair[n_left:]
        lnull |= null[:n_left]
        rnull |= null[n_left:]
    lc = np.where(lnull, -1, lc)
    rc = np.where(rnull, -1, rc)
    return lc, rc


def _valid(valid, n):
    return np.ones(n, bool) if valid is None else np.asarray(valid, bool)


# ------------------------------------------------------- reading 1: the scan
class _Forward:
    def __init__(self, allow_eq):
        self.scan_offset, self.allow_eq = 0, allow_eq

    def next(self, l, right, n_right):
        while self.scan_offset < n_right:
            rv = right(self.scan_offset)
            if rv is not None:
                # ge_allow_eq (TotalOrd: a NaN right value is >= every left value)
                if (_eq(rv, l) and self.allow_eq) or _lt(l, rv):
                    return self.scan_offset
            self.scan_offset += 1
        return None


class _Backward:
    def __init__(self, allow_eq):
        self.best_bound, self.scan_offset, self.allow_eq = None, 0, allow_eq

    def next(self, l, right, n_right):
        while self.scan_offset < n_right:
            rv = right(self.scan_offset)
            if rv is not None:
                # lt_allow_eq (TotalOrd: the reference stalls here at a NaN)
                if (_eq(rv, l) and self.allow_eq) or _lt(rv, l):
                    self.best_bound = self.scan_offset
                else:
                    break
            self.scan_offset += 1
        return self.best_bound


class _Nearest:
    def __init__(self, allow_eq):
        self.strictly_smaller, self.upper_candidate, self.allow_eq = None, 0, allow_eq

    def next(self, l, right, n_right):
        while self.upper_candidate < n_right:
            v = right(self.upper_candidate)
            if v is None:
                self.upper_candidate += 1
                continue
            if _lt(l, v):  # TotalOrd for `>`
                break
            self.upper_candidate += 1
        if self.allow_eq and self.upper_candidate > 0:
            v = right(self.upper_candidate - 1)
            if v is not None and _eq(v, l):  # TotalOrd for `==`
                return self.upper_candidate - 1

        def same(a, b):
            return (a is None and b is None) or (a is not None and b is not None and _eq(a, b))

        while self.upper_candidate + 1 < n_right and same(right(self.upper_candidate + 1),
                                                          right(self.upper_candidate)):
            self.upper_candidate += 1
        cursor = self.strictly_smaller if self.strictly_smaller is not None else 0
        while cursor < self.upper_candidate:
            v = right(cursor)
            if v is None:
                cursor += 1
                continue
            if not _lt(v, l):  # TotalOrd for `>=`
                break
            self.strictly_smaller = cursor
            cursor += 1

        def right_get(idx):
            return right(idx) if idx is not None and idx < n_right else None

        lower, upper = right_get(self.strictly_smaller), right_get(self.upper_candidate)
        if lower is None and upper is None:
            return None
        if upper is None:
            return self.strictly_smaller
        if lower is None:
            return self.upper_candidate
        if _abs_diff(l, upper) <= _abs_diff(l, lower):
            return self.upper_candidate
        return self.strictly_smaller


_STATES = {"forward": _Forward, "backward": _Backward, "nearest": _Nearest}


def asof_ref_scan(left, lvalid, right, rvalid, strategy="backward", allow_eq=True, tolerance=None,
                  by_left=None, by_right=None):
    left, right = np.asarray(left), np.asarray(right)
    n, nr = len(left), len(right)
    lv, rv = _valid(lvalid, n), _valid(rvalid, nr)
    rows, ok = np.full(n, -1, np.int64), np.zeros(n, bool)
    tol = _abs_tol(tolerance, left.dtype)

    def keep(l, r):
        return tol is None or bool(_abs_diff(l, r) <= tol)

    if by_left is None:
        # join_asof_impl
        if not lv.any() or not rv.any():
            return rows, ok
        state = _STATES[strategy](allow_eq)

        def get(j):
            return _scalar(right[j]) if rv[j] else None

        for i in range(n):
            if not lv[i]:
                continue
            l = _scalar(left[i])
            r = state.next(l, get, nr)
            if r is not None and keep(l, _scalar(right[r])):
                rows[i], ok[i] = r, True
        return rows, ok
    # _join_asof_by / asof_in_group
    lc, rc = _codes(by_left, by_right, n, nr)
    groups: dict = {}
    for j in range(nr):
        if rc[j] >= 0 and rv[j]:  # "null on": left out of the group
            groups.setdefault(int(rc[j]), []).append(j)
    states: dict = {}
    for i in range(n):
        if lc[i] < 0 or not lv[i]:
            continue
        idxs = groups.get(int(lc[i]))
        if not idxs:
            continue
        state = states.setdefault(idxs[0], _STATES[strategy](allow_eq))
        l = _scalar(left[i])
        g = state.next(l, lambda k: _scalar(right[idxs[k]]), len(idxs))
        if g is not None and keep(l, _scalar(right[idxs[g]])):
            rows[i], ok[i] = idxs[g], True
    return rows, ok


# ---------------------------------------------------- reading 2: the bounds
def _diff_arr(a, b):
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore", over="ignore"):
            return np.abs(a - b)
    return abs(a.astype(object) - b.astype(object))  # Python integers: exact


def _le(a, b):
    with np.errstate(invalid="ignore"):
        return np.asarray(a <= b, dtype=bool)


def _bounds_group(l, vals, strategy, allow_eq, tol):
    """Positions in `vals` (ascending, no nulls) for the left keys `l`."""
    n = len(vals)
    if n == 0 or len(l) == 0:
        return np.full(len(l), -1, np.int64), np.zeros(len(l), bool)
    lb = np.searchsorted(vals, l, side="left").astype(np.int64)   # numpy orders NaN last: TotalOrd
    ub = np.searchsorted(vals, l, side="right").astype(np.int64)
    if strategy == "backward":
        p = (ub if allow_eq else lb) - 1
        ok = p >= 0
    elif strategy == "forward":
        p = lb if allow_eq else ub
        ok = p < n
    else:
        has_eq = (ub > lb) & bool(allow_eq)
        lower = lb - 1
        hl, hu = lower >= 0, ub < n
        uv = vals[np.minimum(ub, n - 1)]
        upper = np.searchsorted(vals, uv, side="right").astype(np.int64) - 1
        lo_v = vals[np.maximum(lower, 0)]
        take_up = hu & (~hl | _le(_diff_arr(l, uv), _diff_arr(l, lo_v)))
        p = np.where(has_eq, ub - 1, np.where(take_up, upper, lower))
        ok = has_eq | hl | hu
    p = np.where(ok, p, 0)
    if tol is not None:
        ok = ok & _le(_diff_arr(l, vals[p]), tol)
    return np.where(ok, p, -1), ok


def asof_ref_bounds(left, lvalid, right, rvalid, strategy="backward", allow_eq=True, tolerance=None,
                    by_left=None, by_right=None, codes=None):
    """`codes`: (left codes, right codes) as `_codes` gives them, for callers
    whose `by` keys are already integers (-1: a tuple with a null)."""
    left, right = np.asarray(left), np.asarray(right)
    n, nr = len(left), len(right)
    lv, rv = _valid(lvalid, n), _valid(rvalid, nr)
    rows, ok = np.full(n, -1, np.int64), np.zeros(n, bool)
    tol = _abs_tol(tolerance, left.dtype)
    if by_left is None and codes is None:
        li, ri = np.flatnonzero(lv), np.flatnonzero(rv)
        p, o = _bounds_group(left[li], right[ri], strategy, allow_eq, tol)
        rows[li] = np.where(o, ri[np.maximum(p, 0)] if len(ri) else -1, -1)
        ok[li] = o
        return rows, ok
    lc, rc = codes if codes is not None else _codes(by_left, by_right, n, nr)
    lc, rc = np.where(lv, lc, -1), np.where(rv, rc, -1)  # "null on": left out of the group
    order = np.argsort(rc, kind="stable")
    src = rc[order]
    lorder = np.argsort(lc, kind="stable")
    lsrc = lc[lorder]
    for g in np.unique(src[src >= 0]):
        ri = order[np.searchsorted(src, g, "left"):np.searchsorted(src, g, "right")]
        li = lorder[np.searchsorted(lsrc, g, "left"):np.searchsorted(lsrc, g, "right")]
        if len(li) == 0:
            continue
        p, o = _bounds_group(left[li], right[ri], strategy, allow_eq, tol)
        rows[li] = np.where(o, ri[np.maximum(p, 0)], -1)
        ok[li] = o
    return rows, ok
