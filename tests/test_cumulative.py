"""CPU: cumulative and lag expressions (cum_sum / cum_min / cum_max /
cum_count, shift, diff) -- construction, names, repr, every refusal; the
plugin's translation of the visitor's Function nodes (expr_nodes.rs:1223-1224,
:1265-1269, :1280), plain and as a Window's function, against the
NodeTraverser model of tests/test_polars_engine.py; the argument checks of
plgpu_cumulative and plgpu_lag, which run before any device work; and the
shape of tests/golden/cumulative_cases.json."""

import ctypes as C

import pytest

import polaroid_amd as pl
from conftest import load_golden
from polaroid_amd import polars_engine as PE
from test_polars_engine import FakeNT, FakePolarsDF, PyExprIR, _Enum, _node, _table


# ------------------------------------------------------------ construction
def test_cum_and_lag_nodes():
    x = pl.col("v") * 2
    for op in ("sum", "min", "max", "count"):
        e = getattr(x, "cum_" + op)()
        assert e.kind == "cum" and e.op == op and e.args[0] is x
        assert getattr(x, "cum_" + op)(reverse=False).kind == "cum"
    s = pl.col("v").shift(2, fill_value=0)
    assert s.kind == "lag" and s.op == "shift" and s.value == (2, 0)
    assert pl.col("v").shift().value == (1, None)
    assert pl.col("v").shift(-3, fill_value=pl.lit(1.5)).value == (-3, 1.5)
    assert pl.col("v").shift(pl.lit(4)).value == (4, None)
    import numpy as np

    assert pl.col("v").shift(np.int64(3)).value == (3, None) and type(pl.col("v").shift(np.int32(3)).value[0]) is int
    assert pl.col("v").diff(np.int64(2)).value == (2,)
    # a literal null n: every row shifted out (test_shift.py:124)
    assert pl.col("v").shift(None).value == (None, None)
    assert pl.col("v").shift(None, fill_value=1).value == (None, 1)
    assert pl.col("v").shift(pl.lit(None)).value == (None, None)
    d = pl.col("v").diff()
    assert d.kind == "lag" and d.op == "diff" and d.value == (1,)
    assert pl.col("v").diff(-2, "ignore").value == (-2,)


def test_names_roots_and_repr():
    e = pl.col("volume").cum_sum()
    assert e.output_name() == "volume" and e.meta_root_names() == ["volume"]
    assert repr(e) == 'col("volume").cum_sum()'
    assert repr(pl.col("high").cum_max()) == 'col("high").cum_max()'
    assert repr(pl.col("c").shift(1)).startswith('col("c").shift(1')
    assert repr(pl.col("c").diff(2)).startswith('col("c").diff(2')
    o = pl.col("volume").cum_sum().over("symbol")
    assert o.kind == "over" and o.output_name() == "volume"
    assert o.meta_root_names() == ["volume", "symbol"]
    assert repr(o) == 'col("volume").cum_sum().over([col("symbol")])'
    ret = pl.col("close") / pl.col("close").shift(1).over("symbol", "day") - 1
    assert ret.output_name() == "close"
    assert ret.meta_root_names() == ["close", "symbol", "day"]
    assert ".shift(1" in repr(ret) and '.over([col("symbol"), col("day")])' in repr(ret)
    assert (pl.col("a") * pl.col("b")).diff().over("k").alias("d").output_name() == "d"
    assert (pl.col("a") * pl.col("b")).diff().over("k").meta_root_names() == ["a", "b", "k"]


def test_over_accepts_the_third_family():
    x = pl.col("close") - pl.col("open")
    for f in (x.cum_sum(), x.cum_min(), x.cum_max(), x.cum_count(), x.shift(3), x.shift(-1, fill_value=0.0),
              x.diff(), x.diff(-2)):
        assert f.over("k").kind == "over"
        assert f.alias("y").over("k", "j").value == ("k", "j")
    # the input may hold a window expression (it is elementwise)
    assert (x - x.mean().over("k")).cum_sum().over("k").kind == "over"
    # plain composition outside over()
    assert pl.col("x").shift(1).cum_sum().kind == "cum"
    assert pl.col("x").cum_sum().rolling_mean(3).kind == "rolling"
    assert pl.col("x").rolling_sum(3).diff().kind == "lag"


# ----------------------------------------------------------------- refusals
@pytest.mark.parametrize("build, reason", [
    (lambda: pl.col("c").cum_sum(reverse=True), "reverse=True"),
    (lambda: pl.col("c").cum_min(reverse=True), "reverse=True"),
    (lambda: pl.col("c").cum_max(reverse=True), "reverse=True"),
    (lambda: pl.col("c").cum_count(reverse=True), "reverse=True"),
    (lambda: pl.col("c").shift(pl.col("n")), "computed `n`"),
    (lambda: pl.col("c").shift(1.5), "`n` must be an integer"),
    (lambda: pl.col("c").shift(True), "`n` must be an integer"),
    (lambda: pl.col("c").diff(None), "`n` must be an integer"),
    (lambda: pl.col("c").diff(pl.col("n")), "computed `n`"),
    (lambda: pl.col("c").shift(1, fill_value=pl.col("d")), "computed `fill_value`"),
    (lambda: pl.col("c").shift(1, fill_value=pl.col("d").mean()), "computed `fill_value`"),
    (lambda: pl.col("c").diff(1, "drop"), "changes the length"),
    (lambda: pl.col("c").cum_prod(), "no exact"),
    (lambda: pl.col("c").pct_change(), "forward_fill"),
    (lambda: pl.col("c").cum_sum().sum(), "inside an aggregation"),
    (lambda: (pl.col("c") - pl.col("c").shift(1)).max(), "inside an aggregation"),
    (lambda: pl.col("c").diff().std(), "inside an aggregation"),
    (lambda: pl.col("c").sum().cum_sum(), "must be an elementwise expression"),
    (lambda: pl.col("c").sort().shift(1), "must be an elementwise expression"),
    (lambda: pl.col("c").max().diff(), "must be an elementwise expression"),
    # inside over() only an elementwise input is taken, as for rolling
    (lambda: pl.col("c").shift(1).cum_sum().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").rolling_mean(2).diff().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").cum_sum().rolling_sum(2).over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").cum_sum().over("a").over("b"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").cum_sum().over("a").sum(), "inside an aggregation"),
])
def test_refusals(build, reason):
    with pytest.raises(pl.InvalidOperationError) as ei:
        build()
    assert reason in str(ei.value)


def test_over_message_names_the_new_family():
    with pytest.raises(pl.InvalidOperationError) as ei:
        pl.col("c").over("a")
    assert "only rolling_* functions and the aggregations" in str(ei.value)
    assert "cum_sum / cum_min / cum_max / cum_count / shift / diff" in str(ei.value)


class _Cols:
    def __init__(self, columns):
        self.columns = columns


def test_filter_predicate_and_explain():
    lf = pl.LazyFrame(("scan", _Cols(["a", "b"])))
    with pytest.raises(pl.InvalidOperationError) as ei:
        lf.filter(pl.col("b").diff() > 0)
    assert "filter predicate" in str(ei.value)
    with pytest.raises(pl.InvalidOperationError) as ei:
        lf.filter(pl.col("b").cum_sum() > 10)
    assert "filter predicate" in str(ei.value)
    text = lf.with_columns(pl.col("b").cum_sum().over("a"), pl.col("b").shift(1).alias("p")).explain()
    assert '.cum_sum().over([col("a")])' in text and ".shift(1" in text


def test_group_by_agg_refuses_the_new_nodes():
    """They are not aggregations: the group-by's lowering names the reason
    (it runs before any device work once the frame exists; here on a frame
    stand-in that only has to hold the key)."""
    from polaroid_amd import frame as F

    one = type("_Col", (), {"dtype": pl.Int64})()

    class _Frame:
        _cols = {"k": one, "v": one}
        columns = ["k", "v"]
        height = 0

    for e in (pl.col("v").cum_sum(), pl.col("v").shift(1).alias("p"), pl.col("v").diff()):
        with pytest.raises(pl.InvalidOperationError) as ei:
            F._gb_lower(_Frame(), "k", [e], None)
        assert "not an aggregation" in str(ei.value)


# ------------------------------------------------------------------- plugin
def _fn(name, *extra):
    """FunctionExpr as the visitor hands it over: function_data (name, ...)."""
    return lambda nt, inputs: nt.e("Function", function_data=(name, *extra), input=inputs, options=None)


def _ir(function, inputs, node_kind="HStack", window=False, wrap=None, table=None, dtypes=None):
    """with_columns / select(<function>(inputs)[.over("k")]); dtypes: the
    scan schema's dtype of some columns, as the visitor names it"""
    table = table if table is not None else _table()[0]
    nt = FakeNT(table)
    nt.dtypes.update(dtypes or {})
    names = table.column_names
    scan = nt.p("DataFrameScan", names, df=FakePolarsDF(table), projection=None, selection=None)
    top = function(nt, [i(nt) for i in inputs])
    if window:
        top = nt.e("Window", function=top, partition_by=[nt.col("k")], order_by=None, order_by_descending=False,
                   order_by_nulls_last=False, options=type("WindowMapping", (), {"kind": "groups_to_rows"})())
    if wrap:
        top = wrap(nt, top)
    if node_kind == "HStack":
        nt.p("HStack", names + ["out"], input=scan, exprs=[PyExprIR(top, "out")])
    else:
        nt.p("Select", ["out"], input=scan, expr=[PyExprIR(top, "out")])
    return nt


def _c(name):
    return lambda nt: nt.col(name)


def _l(v):
    return lambda nt: nt.lit(v)


_ACCEPTED = [
    ("cum_sum", _fn("cum_sum", False), [_c("v")], ("cum", "sum", (False,))),
    ("cum_min", _fn("cum_min", False), [_c("v")], ("cum", "min", (False,))),
    ("cum_max", _fn("cum_max", False), [_c("v")], ("cum", "max", (False,))),
    ("cum_count", _fn("cum_count", False), [_c("v")], ("cum", "count", (False,))),
    ("shift", _fn("shift"), [_c("v"), _l(2)], ("lag", "shift", (2, None))),
    ("shift_and_fill", _fn("shift_and_fill"), [_c("v"), _l(-1), _l(0.5)], ("lag", "shift", (-1, 0.5))),
    ("diff", _fn("diff", "ignore"), [_c("v"), _l(1)], ("lag", "diff", (1,))),
    ("diff_enum", _fn("diff", _Enum("NullBehavior", "Ignore")), [_c("w"), _l(3)], ("lag", "diff", (3,))),
]


@pytest.mark.parametrize("node_kind", ["HStack", "Select"])
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("name, function, inputs, want", _ACCEPTED, ids=[a[0] for a in _ACCEPTED])
def test_translate_accepted_forms(name, function, inputs, want, window, node_kind):
    nt = _ir(function, inputs, node_kind, window)
    plan = PE.translate(nt)
    assert plan[0] == ("with_columns" if node_kind == "HStack" else "select")
    (e,) = plan[2]
    assert e.output_name() == "out"
    f = e.args[0]
    if window:
        assert f.kind == "over" and f.value == ("k",)
        f = f.args[0]
    assert (f.kind, f.op, f.value) == want
    assert f.args[0].kind == "col"
    PE.execute_with_polaroid(nt, None)
    assert callable(nt.udf)


@pytest.mark.parametrize("function, inputs, dtype", [
    (_fn("cum_max", False), [_c("v")], "UInt64"),
    (_fn("cum_min", False), [_c("v")], "UInt64"),
    (_fn("cum_min", False), [_c("v")], "Date"),
    (_fn("cum_max", False), [_c("v")], "Datetime(time_unit='ns', time_zone=None)"),
    (_fn("cum_sum", False), [_c("v")], "Duration(time_unit='us')"),
    (_fn("cum_sum", False), [_c("v")], "Boolean"),
    (_fn("diff", "ignore"), [_c("v"), _l(1)], "Datetime(time_unit='ms', time_zone=None)"),
    (_fn("diff", "ignore"), [_c("v"), _l(1)], "Duration(time_unit='ns')"),
    (_fn("shift"), [_c("v"), _l(1)], "Date"),
    (_fn("shift"), [_c("v"), _l(None)], "Int32"),          # a literal null n
    (_fn("shift_and_fill"), [_c("v"), _l(None), _l(1)], "Int32"),
])
def test_translate_dtypes_the_series_layer_takes(function, inputs, dtype):
    nt = _ir(function, inputs, dtypes={"v": dtype})
    assert PE.translate(nt)[2][0].args[0].kind in ("cum", "lag")


def test_translate_a_return():
    """close / close.shift(1).over(k) - 1"""
    nt = _ir(_fn("shift"), [_c("v"), _l(1)], window=True,
             wrap=lambda t, w: t.bin(t.bin(t.col("v"), "TrueDivide", w), "Minus", t.lit(1)))
    e = PE.translate(nt)[2][0].args[0]
    assert e.kind == "bin" and e.args[0].args[1].kind == "over"
    assert e.args[0].args[1].args[0].kind == "lag"


def _below_agg(nt, top):
    return nt.e("Agg", name="sum", arguments=[top], options=None)


def _string_table():
    import pyarrow as pa

    return pa.table({"k": pa.array([1, 1, 2]), "v": pa.array(["x", "y", "z"]), "w": pa.array([True, False, True])})


@pytest.mark.parametrize("kw, reason", [
    (dict(function=_fn("cum_sum", True), inputs=[_c("v")]), "reverse=True"),
    (dict(function=_fn("cum_max", True), inputs=[_c("v")], window=True), "reverse=True"),
    (dict(function=_fn("diff", "drop"), inputs=[_c("v"), _l(1)]), "null_behavior drop"),
    (dict(function=_fn("diff", _Enum("NullBehavior", "Drop")), inputs=[_c("v"), _l(1)]), "null_behavior drop"),
    (dict(function=_fn("shift"), inputs=[_c("v"), _c("w")]), "shift's n is computed"),
    (dict(function=_fn("shift"), inputs=[_c("v"), _c("w")], window=True), "shift's n is computed"),
    (dict(function=_fn("diff", "ignore"), inputs=[_c("v"), _c("w")]), "diff's n is computed"),
    (dict(function=_fn("shift_and_fill"), inputs=[_c("v"), _l(1), _c("w")]), "fill_value is computed"),
    (dict(function=_fn("cum_prod", False), inputs=[_c("v")]), "cum_prod"),
    (dict(function=_fn("pct_change"), inputs=[_c("v"), _l(1)]), "pct_change"),
    (dict(function=_fn("cum_sum", False), inputs=[_c("v")], table="str"), "cum_sum of a String"),
    (dict(function=_fn("shift"), inputs=[_c("v"), _l(1)], table="str"), "shift of a String"),
    (dict(function=_fn("cum_min", False), inputs=[_c("w")], table="str"), "cum_min of a Boolean"),
    (dict(function=_fn("diff", "ignore"), inputs=[_c("w"), _l(1)], table="str", window=True), "diff of a Boolean"),
    # every dtype the Series layer refuses at collect time is refused from the scan schema
    (dict(function=_fn("diff", "ignore"), inputs=[_c("v"), _l(1)], dtypes={"v": "Date"}), "diff of a Date"),
    (dict(function=_fn("diff", "ignore"), inputs=[_c("v"), _l(1)], dtypes={"v": "Date"}, window=True),
     "diff of a Date"),
    (dict(function=_fn("cum_sum", False), inputs=[_c("v")], dtypes={"v": "Date"}), "cum_sum of a Date"),
    (dict(function=_fn("cum_sum", False), inputs=[_c("v")],
          dtypes={"v": "Datetime(time_unit='us', time_zone=None)"}), "cum_sum of a Datetime"),
    (dict(function=_fn("cum_sum", False), inputs=[_c("v")], dtypes={"v": "Time"}), "dtype Time"),  # refused at the scan
    (dict(function=_fn("cum_max", False), inputs=[_c("v")], dtypes={"v": "Time"}), "dtype Time"),
    (dict(function=_fn("shift"), inputs=[_c("v"), _l(1)], dtypes={"v": "Categorical"}), "shift of a String"),
    (dict(function=_fn("diff", "ignore"), inputs=[_c("v"), _l(None)]), "`n` must be an integer"),
    (dict(function=_fn("cum_sum", False), inputs=[_c("v")], wrap=_below_agg, node_kind="Select"),
     "outside the expressions"),
    (dict(function=_fn("shift"), inputs=[_c("v"), _l(1)], wrap=_below_agg, node_kind="Select"),
     "outside the expressions"),
])
def test_unsupported_forms_stay_on_polars(kw, reason):
    kw = dict(kw)
    if kw.pop("table", None):
        kw["table"] = _string_table()
    nt = _ir(**kw)
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert reason in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None  # polars keeps the query


def test_in_a_filter_and_in_a_group_by_stay_on_polars():
    table = _table()[0]
    nt = FakeNT(table)
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(table), projection=None, selection=None)
    d = nt.e("Function", function_data=("diff", "ignore"), input=[nt.col("v"), nt.lit(1)], options=None)
    nt.p("Filter", ["k", "v", "w"], input=scan, predicate=PyExprIR(nt.bin(d, "Gt", nt.lit(0.0)), "v"))
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert "outside the expressions" in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None
    nt = FakeNT(table)
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(table), projection=None, selection=None)
    cs = nt.e("Function", function_data=("cum_sum", False), input=[nt.col("v")], options=None)
    a = nt.e("Agg", name="max", arguments=[cs], options=False)
    opts = _node("GroupbyOptions", slice=None, dynamic=None, rolling=None)
    nt.p("GroupBy", ["k", "out"], input=scan, keys=[PyExprIR(nt.col("k"), "k")], aggs=[PyExprIR(a, "out")],
         apply=None, maintain_order=True, options=opts)
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert "outside the expressions" in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None


# ------------------------------------------------- C entry points, no GPU
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


def test_native_tables(N):
    assert N.CUM == {"sum": 1, "min": 2, "max": 3, "count": 4}
    assert N.LAG == {"shift": 1, "diff": 2}
    assert N.CUM_TILE >= 64 and N.CUM_TILE % 64 == 0
    # CUM_TILE mirrors kTileRows = kTileThreads * kTilePer * kTileBlocks of the shared scan header
    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "polaroid_amd", "csrc", "seg_scan.hpp")).read()
    th = int(re.search(r"kTileThreads = (\d+);", src).group(1))
    per = int(re.search(r"kTilePer = (\d+);", src).group(1))
    blocks = int(re.search(r"kTileBlocks = (\d+);", src).group(1))
    totals = int(re.search(r"kTotalsThreads = (\d+);", src).group(1))
    assert th * per == N.CUM_BLOCK and th * per * blocks == N.CUM_TILE == 16384
    assert N.CUM_THREADS == th and N.CUM_TOTALS_THREADS == totals


def test_cumulative_argument_checks(N):
    L = N.lib()
    out = N.Column()
    v, seg = _host_col(N, N.F64, 8), _host_col(N, N.BOOL, 8)

    def call(values, starts, kind=N.CUM["sum"]):
        return L.plgpu_cumulative(values, starts, kind, C.byref(out), None)

    assert call(None, None) == N.ERR_INVALID
    assert L.plgpu_cumulative(C.byref(v), None, 1, None, None) == N.ERR_INVALID
    assert call(C.byref(v), None, kind=0) == N.ERR_INVALID
    assert call(C.byref(v), None, kind=5) == N.ERR_INVALID
    assert "kind" in L.plgpu_last_error().decode()
    for dt in (N.STR, N.BOOL, N.U32, N.F32, N.I8, N.I16, N.U8, N.U16):
        for kind in ("sum", "min", "max"):
            assert call(C.byref(_host_col(N, dt, 8)), None, kind=N.CUM[kind]) == N.ERR_SCHEMA, (dt, kind)
    assert call(C.byref(v), C.byref(_host_col(N, N.I64, 8))) == N.ERR_SCHEMA          # starts not Boolean
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 8, nullable=True))) == N.ERR_SCHEMA
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 9))) == N.ERR_SHAPE          # lengths differ
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 9)), kind=N.CUM["count"]) == N.ERR_SHAPE
    assert L.plgpu_last_error()
    assert seg.dtype == N.BOOL


def test_lag_argument_checks(N):
    L = N.lib()
    out = N.Column()
    v = _host_col(N, N.F64, 8)

    def call(values, starts, kind=N.LAG["shift"], n=1):
        return L.plgpu_lag(values, starts, kind, n, 0, 0, C.byref(out), None)

    assert call(None, None) == N.ERR_INVALID
    assert L.plgpu_lag(C.byref(v), None, 1, 1, 0, 0, None, None) == N.ERR_INVALID
    assert call(C.byref(v), None, kind=0) == N.ERR_INVALID
    assert call(C.byref(v), None, kind=3) == N.ERR_INVALID
    for dt in (N.STR, N.BOOL, N.I8, N.I16, N.U8, N.U16):
        assert call(C.byref(_host_col(N, dt, 8)), None) == N.ERR_SCHEMA, dt
        assert call(C.byref(_host_col(N, dt, 8)), None, kind=N.LAG["diff"]) == N.ERR_SCHEMA, dt
    for dt in (N.U32, N.U64):  # unsigned differences are taken as Int64 by the caller
        assert call(C.byref(_host_col(N, dt, 8)), None, kind=N.LAG["diff"]) == N.ERR_SCHEMA, dt
    assert call(C.byref(v), C.byref(_host_col(N, N.I32, 8))) == N.ERR_SCHEMA
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 8, nullable=True))) == N.ERR_SCHEMA
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 7))) == N.ERR_SHAPE
    assert L.plgpu_last_error()


# ------------------------------------------------------------------ golden
def test_golden_file_shape():
    g = load_golden("cumulative_cases.json")
    assert g["cases"], "no cases"
    names = set()
    for c in g["cases"]:
        assert set(c) >= {"name", "source", "op", "dtype", "values", "expected", "expected_dtype"}, c.get("name")
        assert c["name"] not in names
        names.add(c["name"])
        assert ":" in c["source"] and c["source"].split(":")[0].endswith(".py")
        assert c["op"] in ("cum_sum", "cum_min", "cum_max", "cum_count", "shift", "diff")
        assert len(c["values"]) == len(c["expected"])
        if "keys" in c:
            assert len(c["keys"]) == len(c["values"])
        if c["op"] == "diff":
            assert isinstance(c["n"], int)
        if c["op"] == "shift":
            assert c["n"] is None or isinstance(c["n"], int)
