"""The reference's median / quantile, restated for the tests.

polars-core/src/chunked_array/ops/aggregate/quantile.rs: quantile_idx (:16),
linear_interpol (:46), midpoint_interpol (:54) and generic_quantile (:106);
median is quantile(0.5, "linear") (:168).  Python floats are f64 and Python
does not contract a * b + c, so the arithmetic below is the reference's own.

Two forms, pinned to each other by tests/test_quantile.py:
  quantile_ref     the literal restatement, segment by segment;
  quantile_closed  the same as numpy array arithmetic, for large inputs.
Both take the sorted layout plgpu_segment_quantile takes: within every
segment the non-null values ascending in TotalOrd (NaN greatest), then the
segment's nulls.  sorted_layout builds it from a column in row order.
Both return (values, ok): one Float64 per segment, 0.0 where the segment
holds no value, and the validity."""

import math

import numpy as np

METHODS = ("nearest", "higher", "lower", "midpoint", "linear", "equiprobable")


def _round_half_away(x: float) -> int:
    """Rust's f64::round for x >= 0: halves away from zero, never to even.
    (x - floor(x) is exact; this is floor(x + 0.5) wherever that sum is.)"""
    f = math.floor(x)
    return f + 1 if x - f >= 0.5 else f


def quantile_idx(quantile: float, length: int, null_count: int, method: str):
    """quantile.rs:16: (idx, float_idx, top_idx) into the column sorted
    ascending with its nulls first."""
    nonnull_count = float(length - null_count)
    float_idx = (nonnull_count - 1.0) * quantile + float(null_count)
    if method == "nearest":
        idx = _round_half_away(float_idx)
        return idx, 0.0, idx
    if method in ("lower", "midpoint", "linear"):
        base_idx = int(float_idx)
    elif method == "higher":
        base_idx = math.ceil(float_idx)
    elif method == "equiprobable":
        idx = int(max(math.ceil(nonnull_count * quantile) - 1.0, 0.0)) + null_count
        return idx, 0.0, idx
    else:
        raise ValueError(method)
    base_idx = min(max(base_idx, 0), length - 1)
    top_idx = math.ceil(float_idx)
    return base_idx, float_idx, top_idx


def _f64(v) -> float:
    """`as f64` of a value of the column (an integer rounds to nearest even)."""
    return float(v) if isinstance(v, (float, np.floating)) else float(int(v))


def generic_quantile(values, valid, quantile: float, method: str):
    """quantile.rs:106 on one group: `values` / `valid` in the sorted layout
    (non-null values ascending, then the nulls).  None for no value."""
    if not 0.0 <= quantile <= 1.0:
        raise ValueError("`quantile` should be between 0.0 and 1.0")
    length = len(values)
    null_count = length - int(np.count_nonzero(valid))
    if null_count == length:
        return None
    idx, float_idx, top_idx = quantile_idx(quantile, length, null_count, method)
    # sorted.get(i) of the reference's nulls-first sort is row i - null_count here
    lower = _f64(values[idx - null_count])
    if method not in ("midpoint", "linear") or top_idx == idx:
        return lower
    upper = _f64(values[idx + 1 - null_count])
    if lower == upper:
        return lower
    if method == "midpoint":
        return (lower + upper) / 2.0
    return (float_idx - float(idx)) * (upper - lower) + lower


def segment_bounds(n: int, seg):
    """(starts, ends) of the segments: `seg` None is one segment (also of an
    empty column); row 0 starts a segment whatever its bit says."""
    if seg is None:
        return np.array([0], np.int64), np.array([n], np.int64)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    s = np.asarray(seg, bool).copy()
    s[0] = True
    starts = np.flatnonzero(s).astype(np.int64)
    return starts, np.append(starts[1:], n).astype(np.int64)


def quantile_ref(values, valid, seg, quantile: float, method: str):
    """The literal form on every segment of the sorted layout."""
    values = np.asarray(values)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    starts, ends = segment_bounds(len(values), seg)
    out, ok = np.zeros(len(starts), np.float64), np.zeros(len(starts), bool)
    for g, (s, e) in enumerate(zip(starts.tolist(), ends.tolist())):
        r = generic_quantile(values[s:e], valid[s:e], quantile, method)
        if r is not None:
            out[g], ok[g] = r, True
    return out, ok


def quantile_closed(values, valid, seg, quantile: float, method: str):
    """The same, as array arithmetic over all segments at once."""
    values = np.asarray(values)
    n = len(values)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    starts, ends = segment_bounds(n, seg)
    length = ends - starts
    csum = np.concatenate([[0], np.cumsum(valid, dtype=np.int64)])
    nn = csum[ends] - csum[starts]
    nc = length - nn
    ok = nn > 0
    q = np.float64(quantile)
    nnf, ncf = nn.astype(np.float64), nc.astype(np.float64)
    fi = (nnf - 1.0) * q + ncf
    top = np.ceil(fi)
    last = np.maximum(length - 1, 0).astype(np.float64)
    if method == "nearest":
        f = np.floor(fi)
        idx = f + ((fi - f) >= 0.5)
    elif method == "equiprobable":
        idx = np.maximum(np.ceil(nnf * q) - 1.0, 0.0) + ncf
    elif method == "higher":
        idx = np.minimum(top, last)
    elif method in ("lower", "midpoint", "linear"):
        idx = np.minimum(np.floor(fi), last)
    else:
        raise ValueError(method)
    row = np.where(ok, starts + idx.astype(np.int64) - nc, 0)
    vals64 = values.astype(np.float64) if n else np.zeros(1, np.float64)
    lower = vals64[np.minimum(row, max(n - 1, 0))]
    out = lower
    if method in ("midpoint", "linear"):
        interp = ok & (top != idx)
        upper = vals64[np.minimum(row + 1, max(n - 1, 0))]
        with np.errstate(invalid="ignore", over="ignore"):
            mixed = (lower + upper) / 2.0 if method == "midpoint" else (fi - idx) * (upper - lower) + lower
        out = np.where(interp & ~(lower == upper), mixed, lower)
    return np.where(ok, out, 0.0), ok


def sorted_layout(values, valid=None, groups=None):
    """(sorted values, sorted validity, segment starts or None) of a column in
    row order: by group id ascending, the non-null values ascending with NaN
    greatest, then the nulls."""
    values = np.asarray(values)
    n = len(values)
    valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    if values.dtype.kind == "f":
        nan = np.isnan(values)
        body = np.where(nan, 0.0, values)
    else:
        nan, body = np.zeros(n, bool), values
    gk = np.zeros(n, np.int64) if groups is None else np.asarray(groups)
    order = np.lexsort((body, nan, ~valid, gk))
    sv, sok = values[order], valid[order]
    if groups is None:
        return sv, sok, None
    sg = gk[order]
    seg = np.ones(n, bool)
    seg[1:] = sg[1:] != sg[:-1]
    return sv, sok, seg
