"""CPU: ewm_mean -- the restatement of the reference's loop (tests/ewm_ref.py)
pinned against the cases transcribed from the reference's own tests
(tests/golden/ewm_cases.json), so the yardstick of tests/test_gpu_ewm.py is
itself checked; Expr construction, names and repr; the decay conversions and
every ValueError of py-polars' _prepare_alpha; every refusal; and the argument
checks of plgpu_ewm_mean, which run before any device work."""

import ctypes as C
import math

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from ewm_ref import ewm_mean_ref, prepare_alpha

CASES = load_golden("ewm_cases.json")["cases"]


def golden_runs(case):
    """Every (params, ignore_nulls, min_samples) combination a case stands for."""
    p = dict(case["params"])
    for ign in case["ignore_nulls"]:
        for ms in case.get("min_samples", [p.get("min_samples", 1)]):
            yield {**p, "ignore_nulls": ign, "min_samples": ms}


def check_golden(case, got, what):
    """`got`: a list, None for a null row."""
    if case["compare"] == "null_count":
        assert sum(v is None for v in got) == case["expected_null_count"], (what, got)
        return
    exp = case["expected"]
    assert [v is None for v in got] == [v is None for v in exp], (what, got)
    for g, e in zip(got, exp):
        if e is None:
            continue
        if case["compare"] == "list":
            assert g == e, (what, got)
        elif case["compare"] == "abs1e-15":
            assert abs(g - e) <= 1e-15, (what, got)
        else:  # assert_series_equal's defaults
            assert abs(g - e) <= 1e-8 + 1e-5 * abs(e), (what, got)


# ------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatement_against_the_reference_cases(case):
    vals = np.array([0.0 if v is None else float(v) for v in case["values"]])
    valid = np.array([v is not None for v in case["values"]])
    for run in golden_runs(case):
        alpha = prepare_alpha(run.get("com"), None, None, run.get("alpha"))
        for ftype in (float, np.longdouble):
            out, ok = ewm_mean_ref(vals, valid, alpha, run.get("adjust", True), run["min_samples"],
                                   run["ignore_nulls"], ftype=ftype)
            got = [float(v) if k else None for v, k in zip(out, ok)]
            check_golden(case, got, (case["name"], run, ftype))


def test_golden_file_shape():
    names = set()
    for c in CASES:
        assert set(c) >= {"name", "source", "dtype", "values", "params", "ignore_nulls", "compare"}, c.get("name")
        assert c["name"] not in names
        names.add(c["name"])
        assert ":" in c["source"] and c["source"].split(":")[0].endswith((".py", ".rs"))
        assert c["compare"] in ("series", "abs1e-15", "list", "null_count")
        if c["compare"] != "null_count":
            assert len(c["values"]) == len(c["expected"])
    assert {"mean_int_com", "rs_with_null_noadjust_keep", "leading_nulls_count_3"} <= names


def test_restatement_segments_and_float32():
    vals = np.array([1.0, 2.0, 3.0, 10.0, 20.0, 30.0])
    valid = np.ones(6, bool)
    starts = np.array([0, 0, 0, 1, 0, 0], bool)
    out, ok = ewm_mean_ref(vals, valid, 0.5, starts=starts)
    a, _ = ewm_mean_ref(vals[:3], valid[:3], 0.5)
    b, _ = ewm_mean_ref(vals[3:], valid[3:], 0.5)
    assert ok.all() and out.tolist() == a.tolist() + b.tolist()
    f, _ = ewm_mean_ref(vals.astype(np.float32), valid, 0.3, ftype=np.float32)
    assert f.dtype == np.float32 and f[0] == 1.0


# ------------------------------------------------------------- construction
def test_nodes_names_and_repr():
    x = pl.col("close") * 2
    e = x.ewm_mean(alpha=0.25, adjust=False, min_samples=3, ignore_nulls=True)
    assert e.kind == "ewm" and e.op == "mean" and e.args[0] is x
    assert e.value == (0.25, False, 3, True)
    d = pl.col("close").ewm_mean(span=3)
    assert d.value == (0.5, True, 1, False)
    assert d.output_name() == "close" and d.meta_root_names() == ["close"]
    assert repr(d).startswith('col("close").ewm_mean(alpha=0.5') and "adjust=True" in repr(d)
    o = pl.col("close").ewm_mean(half_life=1).over("symbol")
    assert o.kind == "over" and o.value == ("symbol",) and o.output_name() == "close"
    assert o.meta_root_names() == ["close", "symbol"]
    assert ".ewm_mean(alpha=0.5" in repr(o) and '.over([col("symbol")])' in repr(o)
    assert type(pl.col("c").ewm_mean(alpha=1).value[0]) is float
    assert pl.col("c").ewm_mean(alpha=0.5, min_samples=np.int64(2)).value[2] == 2
    # compositions: below the top of an expression, and on another member of the family
    assert (pl.col("x") - pl.col("x").ewm_mean(span=12)).kind == "bin"
    assert pl.col("x").forward_fill().ewm_mean(alpha=0.1).kind == "ewm"
    assert pl.col("x").ewm_mean(alpha=0.1).diff().kind == "lag"
    assert (pl.col("a") - pl.col("b")).ewm_mean(com=1).alias("y").over("k", "j").value == ("k", "j")


def test_prepare_alpha_conversions():
    from polaroid_amd.expr import _prepare_alpha

    assert _prepare_alpha(com=2.0) == 1.0 / 3.0 and _prepare_alpha(com=0) == 1.0
    assert _prepare_alpha(span=20) == 2.0 / 21.0 and _prepare_alpha(span=1) == 1.0
    assert _prepare_alpha(half_life=2.5) == 1.0 - math.exp(-math.log(2.0) / 2.5)
    assert _prepare_alpha(alpha=0.3) == 0.3 and _prepare_alpha(alpha=1) == 1.0
    for kw in (dict(com=2.0), dict(span=7), dict(half_life=0.75), dict(alpha=0.125)):
        assert _prepare_alpha(**kw) == prepare_alpha(**kw)
        assert pl.col("c").ewm_mean(**kw).value[0] == prepare_alpha(**kw)


@pytest.mark.parametrize("kw, message", [
    (dict(span=1.5, half_life=0.75), "mutually exclusive"),
    (dict(com=0.5, alpha=0.5), "mutually exclusive"),
    (dict(alpha=0.5, span=1.5), "mutually exclusive"),
    (dict(com=1, span=2, half_life=3, alpha=0.5), "mutually exclusive"),
    (dict(), "one of `com`, `span`, `half_life`, or `alpha` must be set"),
    (dict(com=-0.5), "require `com` >= 0"),
    (dict(span=0.5), "require `span` >= 1"),
    (dict(half_life=0), "require `half_life` > 0"),
    (dict(alpha=-0.5), "require 0 < `alpha` <= 1"),
    (dict(alpha=-0.0000001), "require 0 < `alpha` <= 1"),
    (dict(alpha=0.0), "require 0 < `alpha` <= 1"),
    (dict(alpha=1.0000001), "require 0 < `alpha` <= 1"),
    (dict(alpha=1.5), "require 0 < `alpha` <= 1"),
    (dict(alpha=float("nan")), "require 0 < `alpha` <= 1"),
])
def test_param_validation(kw, message):
    """test_ewm_param_validation (py-polars/tests/unit/operations/test_ewm.py:177-200)."""
    with pytest.raises(ValueError, match=message):
        pl.col("values").ewm_mean(**kw, ignore_nulls=False)


# ----------------------------------------------------------------- refusals
@pytest.mark.parametrize("build, reason", [
    (lambda: pl.col("c").ewm_mean(alpha=0.5, min_samples=-1), "non-negative integer"),
    (lambda: pl.col("c").ewm_mean(alpha=0.5, min_samples=1.5), "must be an integer"),
    (lambda: pl.col("c").ewm_mean(alpha=0.5).sum(), "inside an aggregation"),
    (lambda: (pl.col("c") - pl.col("c").ewm_mean(span=3)).max(), "inside an aggregation"),
    (lambda: pl.col("c").sum().ewm_mean(alpha=0.5), "must be an elementwise expression"),
    (lambda: pl.col("c").sort().ewm_mean(alpha=0.5), "must be an elementwise expression"),
    # inside over() only an elementwise input is taken, as for its siblings
    (lambda: pl.col("c").shift(1).ewm_mean(alpha=0.5).over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").ewm_mean(alpha=0.5).cum_sum().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").ewm_mean(alpha=0.5).over("a").over("b"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").ewm_std(alpha=0.5), "ewm_std is not built"),
    (lambda: pl.col("c").ewm_var(span=3), "ewm_var is not built"),
    (lambda: pl.col("c").ewm_mean_by("t", half_life="1d"), "ewm_mean_by is not built"),
])
def test_refusals(build, reason):
    with pytest.raises(pl.InvalidOperationError) as ei:
        build()
    assert reason in str(ei.value)


def test_over_message_names_ewm_mean():
    with pytest.raises(pl.InvalidOperationError) as ei:
        pl.col("c").over("a")
    assert "ewm_mean" in str(ei.value)


class _Cols:
    def __init__(self, columns):
        self.columns = columns


def test_filter_predicate_and_explain():
    lf = pl.LazyFrame(("scan", _Cols(["a", "b"])))
    with pytest.raises(pl.InvalidOperationError) as ei:
        lf.filter(pl.col("b").ewm_mean(alpha=0.5) > 0)
    assert "filter predicate" in str(ei.value) and "ewm_mean" in str(ei.value)
    text = lf.with_columns(pl.col("b").ewm_mean(span=3).over("a")).explain()
    assert '.ewm_mean(alpha=0.5' in text and '.over([col("a")])' in text


def test_group_by_agg_refuses_the_node():
    from polaroid_amd import frame as F

    one = type("_Col", (), {"dtype": pl.Int64})()

    class _Frame:
        _cols = {"k": one, "v": one}
        columns = ["k", "v"]
        height = 0

    for e in (pl.col("v").ewm_mean(alpha=0.5), pl.col("v").ewm_mean(span=5).alias("p")):
        with pytest.raises(pl.InvalidOperationError) as ei:
            F._gb_lower(_Frame(), "k", [e], None)
        assert "not an aggregation" in str(ei.value) and "ewm_mean" in str(ei.value)


def test_refused_dtypes():
    """Boolean, String, Categorical and temporal columns are refused before
    any device work (on stand-ins that hold what the check reads)."""
    from polaroid_amd import _native as N

    def column(dtype, code, logical=None, cat=None):
        col = type("_C", (), {"dtype": code})()
        return type("_S", (), {"dtype": dtype, "_col": col, "_cat_codes": lambda self: cat,
                               "_logical_dtype": lambda self: logical})()

    for s in (column(pl.Boolean, N.BOOL), column(pl.String, N.STR), column(pl.String, N.U32, cat=("d", "codes")),
              column(pl.Date, N.I32, logical=pl.Date), column(pl.Datetime("us"), N.I64, logical=pl.Datetime("us")),
              column(pl.Duration("ns"), N.I64, logical=pl.Duration("ns"))):
        with pytest.raises(pl.InvalidOperationError) as ei:
            pl.Series._ewm_mean(s, 0.5, True, 1, False)
        assert "ewm_mean of a" in str(ei.value) and "must be numeric" in str(ei.value)


# ------------------------------------------------- the C entry point, no GPU
@pytest.fixture(scope="module")
def N():
    from polaroid_amd import _native

    _native.lib()
    return _native


def _host_col(N, dtype, n, nullable=False):
    c = N.Column()
    c.dtype, c.length = dtype, n
    c.values = 0x1000  # never dereferenced: validation fails before any device work
    if nullable:
        c.validity = 0x2000
    return c


def test_ewm_mean_argument_checks(N):
    L = N.lib()
    out = N.Column()
    v = _host_col(N, N.F64, 8)

    def call(values, starts, alpha=0.5, min_samples=1):
        return L.plgpu_ewm_mean(values, starts, alpha, 1, 0, min_samples, C.byref(out), None)

    assert call(None, None) == N.ERR_INVALID
    assert L.plgpu_ewm_mean(C.byref(v), None, 0.5, 1, 0, 1, None, None) == N.ERR_INVALID
    for alpha in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert call(C.byref(v), None, alpha=alpha) == N.ERR_INVALID, alpha
        assert "alpha" in L.plgpu_last_error().decode()
    assert call(C.byref(v), None, min_samples=-1) == N.ERR_INVALID
    assert "min_samples" in L.plgpu_last_error().decode()
    assert call(C.byref(v), C.byref(_host_col(N, N.I64, 8))) == N.ERR_INVALID          # starts not Boolean
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 8, nullable=True))) == N.ERR_INVALID
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 9))) == N.ERR_INVALID          # lengths differ
    for dt in (N.STR, N.BOOL, N.I8, N.I16, N.I32, N.I64, N.U8, N.U16, N.U32, N.U64):
        assert call(C.byref(_host_col(N, dt, 8)), None) == N.ERR_SCHEMA, dt
        assert "Float32 / Float64" in L.plgpu_last_error().decode()
    assert N.lib().plgpu_abi_version() == 1
    assert N.CUM_BLOCK % N.CUM_THREADS == 0 and N.CUM_TOTALS_THREADS % 64 == 0
