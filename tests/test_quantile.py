"""CPU: the restated reference of median / quantile (tests/quantile_ref.py) --
its literal form and its numpy closed form pinned to each other and to the
reference's own cases (tests/golden/quantile_cases.json) -- and the expression
layer: names, repr, root names, argument checks and refusals.

distributed.group_by_agg refuses median / quantile before it looks for a process
group, so that refusal is reached here without one."""

import math

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden, unhex
from quantile_ref import (METHODS, generic_quantile, quantile_closed, quantile_idx, quantile_ref, segment_bounds,
                          sorted_layout)

QS = [0.0, 0.1, 0.24, 0.25, 0.26, 0.5, 0.75, 0.9, 1.0]
CASES = load_golden("quantile_cases.json")["cases"]


def same(a, aok, b, bok, what):
    """Exact: the same validity, values equal under == and NaN where NaN."""
    assert np.array_equal(aok, bok), what
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    bad = np.flatnonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))
    assert bad.size == 0, (what, bad[:8], a[bad[:8]], b[bad[:8]])


def _random_layout(rng, n, nsegs, null_mode, floats):
    groups = np.sort(rng.integers(0, nsegs, n))
    if floats:
        pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.25, 1e300, 5e-324, 3.0])
        vals = pool[rng.integers(0, len(pool), n)]
    else:
        vals = rng.integers(-50, 50, n).astype(np.int64)
    if null_mode == "none":
        valid = np.ones(n, bool)
    elif null_mode == "one":
        valid = np.ones(n, bool)
        valid[rng.integers(0, n)] = False
    elif null_mode == "most":
        valid = rng.random(n) < 0.15
    else:
        valid = np.zeros(n, bool)
    return sorted_layout(vals, valid, groups)


@pytest.mark.parametrize("null_mode", ["none", "one", "most", "all"])
@pytest.mark.parametrize("method", METHODS)
def test_literal_and_closed_forms_agree(method, null_mode):
    rng = np.random.default_rng(METHODS.index(method) * 7 + len(null_mode))
    for n, nsegs, floats in ((1, 1, False), (2, 1, True), (7, 3, False), (40, 1, True), (300, 25, False),
                             (300, 25, True), (301, 300, False)):
        sv, sok, seg = _random_layout(rng, n, nsegs, null_mode, floats)
        for q in QS:
            a, aok = quantile_ref(sv, sok, seg, q, method)
            b, bok = quantile_closed(sv, sok, seg, q, method)
            same(a, aok, b, bok, (method, null_mode, n, q))
            if nsegs == 1:
                c, cok = quantile_ref(sv, sok, None, q, method)
                same(a, aok, c, cok, (method, null_mode, n, q, "no segment column"))


def test_empty_columns():
    for m in METHODS:
        for f in (quantile_ref, quantile_closed):
            v, ok = f(np.zeros(0, np.int64), None, None, 0.5, m)        # one segment: one null row
            assert v.tolist() == [0.0] and ok.tolist() == [False]
            v, ok = f(np.zeros(0, np.int64), None, np.zeros(0, bool), 0.5, m)
            assert len(v) == 0 and len(ok) == 0


def test_index_rule_points():
    # a half rounds away from zero (quantile.rs:26 f64::round), not to even
    assert quantile_idx(0.5, 2, 0, "nearest")[0] == 1
    assert quantile_idx(0.5, 4, 0, "nearest")[0] == 2          # 1.5 -> 2
    assert quantile_idx(0.5, 6, 0, "nearest")[0] == 3          # 2.5 -> 3 (banker's rounding gives 2)
    assert quantile_idx(0.0, 5, 0, "equiprobable")[0] == 0
    assert quantile_idx(0.25, 4, 0, "equiprobable")[0] == 0
    assert quantile_idx(0.26, 4, 0, "equiprobable")[0] == 1
    assert quantile_idx(1.0, 4, 2, "equiprobable")[0] == 3
    # the null count enters float_idx: the index counts the nulls first
    idx, fi, top = quantile_idx(0.24, 7, 2, "linear")
    assert (idx, top) == (2, 3) and fi == (5.0 - 1.0) * 0.24 + 2.0
    assert quantile_idx(1.0, 7, 2, "higher")[0] == 6
    vals, ok = np.array([1, 2, 3, 4, 5, 0, 0]), np.array([1, 1, 1, 1, 1, 0, 0], bool)
    assert generic_quantile(vals, ok, 0.24, "linear") == (fi - 2.0) * (2.0 - 1.0) + 1.0
    # IEEE ==: infinities of opposite sign interpolate to NaN, equal neighbours to themselves
    inf = np.array([-np.inf, np.inf])
    assert math.isnan(generic_quantile(inf, np.ones(2, bool), 0.5, "midpoint"))
    assert math.isnan(generic_quantile(inf, np.ones(2, bool), 0.5, "linear"))
    assert generic_quantile(np.array([np.inf, np.inf]), np.ones(2, bool), 0.5, "linear") == np.inf
    assert math.isnan(generic_quantile(np.array([np.nan, np.nan]), np.ones(2, bool), 0.5, "midpoint"))
    # Int64 above 2^53 reads through `as f64`
    big = np.array([2 ** 53 + 1, 2 ** 63 - 1], np.int64)
    assert generic_quantile(big, np.ones(2, bool), 0.0, "lower") == float(2 ** 53)
    assert generic_quantile(big, np.ones(2, bool), 1.0, "nearest") == float(2 ** 63)
    with pytest.raises(ValueError):
        generic_quantile(vals, ok, 1.5, "linear")


def case_inputs(case):
    """(values Int64, validity, group id per row or None, q, method, expected, expected validity)."""
    raw = case["values"]
    valid = np.array([v is not None for v in raw], bool)
    vals = np.array([0 if v is None else v for v in raw], np.int64)
    gid = None
    if "keys" in case:
        (_, key), = case["keys"].items()
        first = {}
        gid = np.array([first.setdefault(k, len(first)) for k in key], np.int64)
    exp = case["expected"]
    eok = np.array([e is not None for e in exp], bool)
    ev = np.array([0.0 if e is None else unhex(e) for e in exp], np.float64)
    return vals, valid, gid, unhex(case["quantile"]), case["method"], ev, eok


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_golden_cases(case):
    vals, valid, gid, q, method, ev, eok = case_inputs(case)
    assert method in METHODS and case["dtype"] == "Int64"
    if case.get("median"):
        assert (q, method) == (0.5, "linear")
    sv, sok, seg = sorted_layout(vals, valid, gid)
    assert len(segment_bounds(len(sv), seg)[0]) == len(ev)
    for f in (quantile_ref, quantile_closed):
        got, ok = f(sv, sok, seg, q, method)
        same(got, ok, ev, eok, (case["name"], f.__name__))


def test_golden_covers_the_cited_cases():
    src = " ".join(c["source"] for c in CASES)
    for cited in ("test_statistics.py", "test_aggregations.py", "test_group_by.py", "test_window.py"):
        assert cited in src
    exp = {c["name"]: [unhex(e) for e in c["expected"]] for c in CASES}
    assert exp["statistics_q25_nearest"] == [2.0] and exp["statistics_q24_lower"] == [1.0]
    assert exp["statistics_q26_higher"] == [3.0] and exp["statistics_q24_midpoint"] == [1.5]
    assert exp["statistics_q24_linear"] == [1.96] and exp["statistics_median"] == [3.0]
    assert exp["group_by_shorthand_quantile_a"] == [2.0, 4.0] and exp["group_by_shorthand_quantile_c"] == [1.0, 1.0]
    assert exp["quantile_as_window"] == [1.0, 2.0]


# ------------------------------------------------------------- the expressions
class _Cols:
    """A frame stand-in for plans that are built and explained, never run."""

    def __init__(self, columns):
        self.columns = columns


def test_names_repr_and_roots():
    e = pl.col("x").median()
    assert e.kind == "agg" and e.op == "median" and e.value == (0.5, "linear")
    assert e.output_name() == "x" and e.meta_root_names() == ["x"]
    assert repr(e) == 'col("x").median()'
    e = pl.col("x").quantile(0.25, "linear")
    assert e.kind == "agg" and e.op == "quantile" and e.value == (0.25, "linear")
    assert repr(e) == "col(\"x\").quantile(0.25, interpolation='linear')"
    assert pl.col("x").quantile(0.5).value == (0.5, "nearest")
    assert repr(pl.median("x")) == repr(pl.col("x").median())
    assert repr(pl.quantile("x", 0.9)) == repr(pl.col("x").quantile(0.9, "nearest"))
    assert repr(pl.quantile("x", 0.9, "higher")) == repr(pl.col("x").quantile(0.9, interpolation="higher"))
    e = (pl.col("a") * pl.col("b")).median().alias("m")
    assert e.output_name() == "m" and e.meta_root_names() == ["a", "b"]
    assert pl.col("x").quantile(np.float32(0.5)).value[0] == 0.5
    assert pl.col("x").quantile(1).value[0] == 1.0 and pl.col("x").quantile(np.int64(0)).value[0] == 0.0
    for m in METHODS:
        assert pl.col("x").quantile(0.5, m).value == (0.5, m)
    plan = pl.LazyFrame(("scan", _Cols(["k", "x"]))).group_by("k").agg(pl.col("x").quantile(0.25, "linear"))
    assert "quantile(0.25, interpolation='linear')" in plan.explain()


def test_over_builds_and_inputs_are_checked():
    e = pl.col("x").median().over("k")
    assert e.kind == "over" and e.value == ("k",) and e.meta_root_names() == ["x", "k"]
    e = (pl.col("x") * 2).quantile(0.75, "midpoint").over("k1", "k2")
    assert e.value == ("k1", "k2")
    with pytest.raises(pl.InvalidOperationError, match="inside an aggregation's input"):
        pl.col("x").cum_sum().median()
    with pytest.raises(pl.InvalidOperationError, match="inside an aggregation's input"):
        pl.col("x").rank().quantile(0.5)
    with pytest.raises(pl.InvalidOperationError, match=r"window expression \(over\) inside an aggregation's input"):
        pl.col("x").sum().over("k").median()
    # the message of an expression over() does not take is the one tests/test_over.py pins
    with pytest.raises(pl.InvalidOperationError, match="only rolling_\\* functions and the aggregations") as ei:
        pl.col("x").sort().over("k")
    assert "median, quantile" in str(ei.value)


def test_quantile_argument_checks():
    for bad in (1.5, -0.1, float("nan"), np.float64("nan"), 2):
        with pytest.raises(pl.ComputeError, match="`quantile` should be between 0.0 and 1.0"):
            pl.col("x").quantile(bad)
        with pytest.raises(pl.ComputeError, match="`quantile` should be between 0.0 and 1.0"):
            pl.quantile("x", bad, "linear")
    with pytest.raises(pl.InvalidOperationError, match="a computed `quantile` is not supported on the GPU executor"):
        pl.col("x").quantile(pl.col("q"))
    with pytest.raises(pl.InvalidOperationError, match="`quantile` must be a real number"):
        pl.col("x").quantile("0.5")
    with pytest.raises(pl.InvalidOperationError, match="`quantile` must be a real number"):
        pl.col("x").quantile(True)
    with pytest.raises(ValueError) as ei:
        pl.col("x").quantile(0.5, "cubic")
    for m in METHODS:
        assert repr(m) in str(ei.value)
    # the shorthands check their arguments when they are built
    lf = pl.LazyFrame(("scan", _Cols(["k", "x"])))
    with pytest.raises(pl.ComputeError, match="`quantile` should be between 0.0 and 1.0"):
        lf.group_by("k").quantile(1.5)
    with pytest.raises(ValueError):
        lf.quantile(0.5, "cubic")
    assert "median" in lf.group_by("k").median().explain() and "quantile(0.5" in lf.quantile(0.5).explain()


def test_distributed_group_by_refuses_by_name():
    from polaroid_amd import distributed

    for e in (pl.col("x").median(), pl.col("x").quantile(0.5).alias("q")):
        with pytest.raises(pl.InvalidOperationError, match="median / quantile are not supported by the multi-GPU"):
            distributed.group_by_agg(None, "k", [pl.col("x").sum(), e])
