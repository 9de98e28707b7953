"""CPU: rank -- the restatement of the reference's rank (tests/rank_ref.py)
pinned against the cases transcribed from the reference's own tests and
docstrings (tests/golden/rank_cases.json) and against its numpy closed form, so
the yardsticks of tests/test_gpu_rank.py are themselves checked; Expr
construction, names and repr; every refusal and ValueError; and the argument
checks of plgpu_rank, which run before any device work."""

import ctypes as C

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from rank_ref import METHODS, rank_closed, rank_closed_all, rank_ref

CASES = load_golden("rank_cases.json")["cases"]
_NP = {"Int32": np.int32, "Int64": np.int64, "UInt32": np.uint32, "Float64": np.float64}


def case_inputs(case):
    """(values, validity, segment starts or None, group ids or None) of a fixture case."""
    vals = np.array([0 if v is None else v for v in case["values"]], dtype=_NP[case["dtype"]])
    valid = np.array([v is not None for v in case["values"]], dtype=bool)
    starts = groups = None
    if "keys" in case:
        (key,) = case["keys"].values()  # the fixture's keys arrive sorted
        groups = np.array(key, dtype=np.int64)
        starts = np.append(True, groups[1:] != groups[:-1])
    return vals, valid, starts, groups


def check_case(case, ranks, ok, what):
    """`ranks`, `ok`: numpy arrays; exact in values, nulls and dtype."""
    exp = case["expected"]
    assert ranks.dtype == (np.float64 if case["expected_dtype"] == "Float64" else np.uint32), what
    assert ok.tolist() == [e is not None for e in exp], (what, ok)
    assert [r for r, k in zip(ranks.tolist(), ok) if k] == [e for e in exp if e is not None], (what, ranks)


# ------------------------------------------------------------- the yardsticks
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_restatements_against_the_reference_cases(case):
    vals, valid, starts, groups = case_inputs(case)
    check_case(case, *rank_ref(vals, valid, case["method"], case["descending"], starts), "restatement")
    check_case(case, *rank_closed(vals, valid, case["method"], case["descending"], groups), "closed form")


def test_golden_file_shape():
    names = set()
    for c in CASES:
        assert set(c) >= {"name", "source", "dtype", "values", "method", "descending", "expected_dtype",
                          "expected"}, c.get("name")
        assert c["name"] not in names
        names.add(c["name"])
        assert ":" in c["source"] and c["source"].split(":")[0].endswith((".py", ".rs"))
        assert c["method"] in METHODS and c["dtype"] in _NP
        assert c["expected_dtype"] == ("Float64" if c["method"] == "average" else "UInt32")
        assert len(c["values"]) == len(c["expected"])
        for key in c.get("keys", {}).values():
            assert len(key) == len(c["values"])
    assert {"rs_rank_ordinal", "rs_all_null_dense", "rs_empty_max", "rs_reverse_dense", "py_nulls_two",
            "py_df_max", "py_series_dense_descending", "py_so_4109_average", "doc_over"} <= names
    assert {c["method"] for c in CASES} == set(METHODS)


def _random_column(rng, n, kind):
    if kind == "float":
        pool = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.25, 3.0, 1e300, -1e-300])
        vals = pool[rng.integers(0, len(pool), n)]
    else:
        vals = rng.integers(-3, 4, n).astype(np.int64)
    return vals, rng.random(n) >= 0.25


@pytest.mark.parametrize("kind", ["float", "int"])
def test_restatement_and_closed_form_agree(kind):
    """Random small inputs with NaN, +-0.0, +-inf and nulls, plain and in
    segments: the loop and the closed form give the same bits."""
    rng = np.random.default_rng(7)
    for trial in range(120):
        n = int(rng.integers(0, 40))
        vals, valid = _random_column(rng, n, kind)
        if trial % 3 == 0:
            valid[:] = trial % 2 == 0
        starts = np.append(True, rng.random(max(n - 1, 0)) < 0.2)[:n]
        groups = np.cumsum(starts) - 1
        for desc in (False, True):
            both = rank_closed_all(vals, valid, desc, groups)
            for m in METHODS:
                for st, got in ((None, rank_closed(vals, valid, m, desc)), (starts, both[m])):
                    r, ok = rank_ref(vals, valid, m, desc, st)
                    assert r.dtype == got[0].dtype and np.array_equal(ok, got[1]), (trial, m, desc)
                    assert np.array_equal(r.view(np.uint8), got[0].view(np.uint8)), (trial, m, desc, vals, valid)


def test_restatement_ties_and_order():
    nan = float("nan")
    vals = np.array([0.0, nan, -0.0, 1.0, nan, np.inf])
    ok = np.ones(6, bool)
    assert rank_ref(vals, ok, "min")[0].tolist() == [1, 5, 1, 3, 5, 4]          # -0.0 ties 0.0, NaN ties NaN, greatest
    assert rank_ref(vals, ok, "ordinal")[0].tolist() == [1, 5, 2, 3, 6, 4]
    assert rank_ref(vals, ok, "ordinal", True)[0].tolist() == [5, 1, 6, 4, 2, 3]  # ties in row order descending too
    assert rank_ref(vals, ok, "dense", True)[0].tolist() == [4, 1, 4, 3, 1, 2]
    # rows of a closed-form group need not be adjacent
    g = np.array([1, 0, 1, 0, 1, 0])
    v = np.array([5, 5, 3, 9, 3, 1])
    assert rank_closed(v, ok, "max", False, g)[0].tolist() == [3, 2, 2, 3, 2, 1]


# ------------------------------------------------------------- construction
def test_nodes_names_and_repr():
    x = pl.col("volume") * 2
    e = x.rank("dense", descending=True)
    assert e.kind == "rank" and e.op == "dense" and e.value == (True,) and e.args[0] is x
    d = pl.col("volume").rank()
    assert d.op == "average" and d.value == (False,)
    assert d.output_name() == "volume" and d.meta_root_names() == ["volume"]
    assert repr(pl.col("x").rank("dense", descending=True)) == 'col("x").rank(method=\'dense\', descending=True)'
    assert repr(d) == 'col("volume").rank(method=\'average\', descending=False)'
    o = pl.col("volume").rank("dense", descending=True).over("symbol")
    assert o.kind == "over" and o.value == ("symbol",) and o.output_name() == "volume"
    assert o.meta_root_names() == ["volume", "symbol"]
    assert repr(o) == 'col("volume").rank(method=\'dense\', descending=True).over([col("symbol")])'
    for m in METHODS:
        assert pl.col("c").rank(m).op == m and pl.col("c").rank(method=m, seed=3).op == m
    # compositions: below the top of an expression, and on another member of the family
    assert (pl.col("x").rank("ordinal") <= 3).kind == "bin"
    assert pl.col("x").forward_fill().rank().kind == "rank"
    assert pl.col("x").rank().diff().kind == "lag"
    assert (pl.col("a") - pl.col("b")).rank("min").alias("y").over("k", "j").value == ("k", "j")
    assert pl.col("x").rank().over(["k%d" % i for i in range(7)]).kind == "over"


@pytest.mark.parametrize("method", ["first", "Dense", "", None, 3])
def test_unknown_method_is_a_value_error(method):
    with pytest.raises(ValueError, match="`method` must be one of"):
        pl.col("c").rank(method)
    s = type("_S", (), {})()
    with pytest.raises(ValueError, match="`method` must be one of"):
        pl.Series._rank(s, method)


# ----------------------------------------------------------------- refusals
@pytest.mark.parametrize("build, reason", [
    (lambda: pl.col("c").rank("random"), "rank(method='random')"),
    (lambda: pl.col("c").rank("random", seed=1), "rank(method='random')"),
    (lambda: pl.Series._rank(None, "random"), "rank(method='random')"),
    (lambda: pl.col("c").rank().sum(), "inside an aggregation"),
    (lambda: (pl.col("c").rank("ordinal") <= 3).max(), "inside an aggregation"),
    (lambda: pl.col("c").sum().rank(), "must be an elementwise expression"),
    (lambda: pl.col("c").sort().rank(), "must be an elementwise expression"),
    # inside over() only an elementwise input is taken, as for its siblings
    (lambda: pl.col("c").shift(1).rank().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").rank().cum_sum().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").rank().over("a").over("b"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").rank().over("a", order_by="b"), "over(order_by=...)"),
    (lambda: pl.col("c").rank().over(["k%d" % i for i in range(8)]), "the sort takes 8 columns"),
])
def test_refusals(build, reason):
    with pytest.raises(pl.InvalidOperationError) as ei:
        build()
    assert reason in str(ei.value)


def test_messages_name_rank():
    with pytest.raises(pl.InvalidOperationError) as ei:
        pl.col("c").over("a")
    assert "rank" in str(ei.value)
    with pytest.raises(pl.InvalidOperationError) as ei:
        pl.col("c").rank().sum()
    assert "/ rank)" in str(ei.value)
    with pytest.raises(pl.InvalidOperationError) as ei:
        pl.col("c").rank().over(["k%d" % i for i in range(8)])
    assert "at most 7 keys" in str(ei.value)


class _Cols:
    def __init__(self, columns):
        self.columns = columns


def test_filter_predicate_and_explain():
    lf = pl.LazyFrame(("scan", _Cols(["a", "b"])))
    with pytest.raises(pl.InvalidOperationError) as ei:
        lf.filter(pl.col("b").rank("ordinal") <= 3)
    assert "filter predicate" in str(ei.value) and "rank" in str(ei.value)
    text = lf.with_columns(pl.col("b").rank("dense", descending=True).over("a")).explain()
    assert ".rank(method='dense', descending=True)" in text and '.over([col("a")])' in text
    assert ".rank(method='min', descending=False)" in lf.select(pl.col("b").rank("min")).explain()


def test_group_by_agg_refuses_the_node():
    from polaroid_amd import frame as F

    one = type("_Col", (), {"dtype": pl.Int64})()

    class _Frame:
        _cols = {"k": one, "v": one}
        columns = ["k", "v"]
        height = 0

    for e in (pl.col("v").rank(), pl.col("v").rank("dense").alias("p")):
        with pytest.raises(pl.InvalidOperationError) as ei:
            F._gb_lower(_Frame(), "k", [e], None)
        assert "not an aggregation" in str(ei.value) and "rank" in str(ei.value)


def test_refused_dtypes():
    """String, Categorical and UInt64 columns are refused by name before any
    device work (on stand-ins that hold what the check reads)."""
    from polaroid_amd import _native as N

    def column(dtype, code, cat=None):
        col = type("_C", (), {"dtype": code})()
        return type("_S", (), {"dtype": dtype, "_col": col, "_cat_codes": lambda self: cat,
                               "_logical_dtype": lambda self: None})()

    for s, name in ((column(pl.String, N.STR), "String"), (column(pl.String, N.U32, cat=("d", "codes")), "String"),
                    (column(pl.UInt64, N.U64), "UInt64")):
        for m in METHODS:
            with pytest.raises(pl.InvalidOperationError) as ei:
                pl.Series._rank(s, m)
            assert f"rank of a {name}" in str(ei.value) and "not supported" in str(ei.value)


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


def test_rank_argument_checks(N):
    L = N.lib()
    out = N.Column()
    idx, sv, tie, seg, v = (_host_col(N, N.U32, 8), _host_col(N, N.I64, 8, nullable=True), _host_col(N, N.BOOL, 8),
                            _host_col(N, N.BOOL, 8), _host_col(N, N.I64, 8, nullable=True))

    def call(idx=idx, sv=sv, tie=tie, seg=seg, v=v, method=1, out=out):
        ref = lambda c: None if c is None else C.byref(c)  # noqa: E731
        return L.plgpu_rank(ref(idx), ref(sv), ref(tie), ref(seg), ref(v), method, ref(out), None)

    for name in ("idx", "sv", "tie", "v", "out"):
        assert call(**{name: None}) == N.ERR_INVALID, name
        assert "NULL" in L.plgpu_last_error().decode()
    for method in (0, 6, -1, 99):
        assert call(method=method) == N.ERR_INVALID, method
        assert "method" in L.plgpu_last_error().decode()
    # lengths that differ
    assert call(idx=_host_col(N, N.U32, 9)) == N.ERR_INVALID
    assert call(sv=_host_col(N, N.I64, 7)) == N.ERR_INVALID
    assert call(tie=_host_col(N, N.BOOL, 9)) == N.ERR_INVALID
    assert call(seg=_host_col(N, N.BOOL, 7)) == N.ERR_INVALID
    assert call(v=_host_col(N, N.I64, 9)) == N.ERR_INVALID
    # the index: null-free UInt32
    for dt in (N.I32, N.I64, N.U64, N.F64, N.BOOL):
        assert call(idx=_host_col(N, dt, 8)) == N.ERR_INVALID, dt
    assert call(idx=_host_col(N, N.U32, 8, nullable=True)) == N.ERR_INVALID
    assert "UInt32" in L.plgpu_last_error().decode()
    # the start columns: null-free Boolean
    for which in ("tie", "seg"):
        assert call(**{which: _host_col(N, N.U32, 8)}) == N.ERR_INVALID
        assert call(**{which: _host_col(N, N.BOOL, 8, nullable=True)}) == N.ERR_INVALID
        assert "Boolean" in L.plgpu_last_error().decode()
    assert N.RANK == {"average": 1, "min": 2, "max": 3, "dense": 4, "ordinal": 5}
    assert N.lib().plgpu_abi_version() == 1
