"""CPU: the fill strategies (forward_fill / backward_fill / fill_null(strategy=...))
-- construction, names, repr, every refusal and ValueError; the plugin's
translation of the visitor's ("fill_null_with_strategy", strategy, limit)
Function node (expr_nodes.rs:1385), plain and as a Window's function, against
the NodeTraverser model of tests/test_polars_engine.py; the argument checks of
plgpu_fill, which run before any device work; and the shape of
tests/golden/fill_cases.json."""

import ctypes as C

import pytest

import polaroid_amd as pl
from conftest import load_golden
from polaroid_amd import polars_engine as PE
from test_polars_engine import FakeNT, FakePolarsDF, PyExprIR, _node, _table

STRATEGIES = ("forward", "backward", "min", "max", "mean", "zero", "one")


# ------------------------------------------------------------ construction
def test_fill_nodes():
    x = pl.col("v") * 2
    for op in STRATEGIES:
        e = x.fill_null(strategy=op)
        assert e.kind == "fill" and e.op == op and e.value == (None,) and e.args[0] is x
    assert pl.col("v").forward_fill().value == (None,) and pl.col("v").forward_fill().op == "forward"
    assert pl.col("v").backward_fill(3).value == (3,) and pl.col("v").backward_fill(3).op == "backward"
    assert pl.col("v").fill_null(strategy="forward", limit=0).value == (0,)
    assert pl.col("v").fill_null(strategy="backward", limit=pl.lit(2)).value == (2,)
    import numpy as np

    assert pl.col("v").forward_fill(np.int64(4)).value == (4,)
    assert type(pl.col("v").forward_fill(np.int32(4)).value[0]) is int
    # fill_null(value) keeps its own node
    f = pl.col("v").fill_null(0)
    assert f.kind == "fill_null" and f.args[1].kind == "lit"
    assert pl.col("v").fill_null(pl.col("w")).kind == "fill_null"


def test_names_roots_and_repr():
    e = pl.col("close").forward_fill()
    assert e.output_name() == "close" and e.meta_root_names() == ["close"]
    assert repr(e) == 'col("close").forward_fill(limit=None)'
    assert repr(pl.col("close").backward_fill(2)) == 'col("close").backward_fill(limit=2)'
    assert repr(pl.col("c").fill_null(strategy="mean")) == "col(\"c\").fill_null(strategy='mean')"
    o = pl.col("close").forward_fill().over("symbol")
    assert o.kind == "over" and o.output_name() == "close" and o.meta_root_names() == ["close", "symbol"]
    assert repr(o) == 'col("close").forward_fill(limit=None).over([col("symbol")])'
    ret = pl.col("x") / pl.col("x").forward_fill().shift(1) - 1
    assert ret.output_name() == "x" and ".forward_fill(limit=None).shift(1" in repr(ret)


def test_over_accepts_the_fill_family():
    x = pl.col("close") - pl.col("open")
    for f in [x.forward_fill(), x.backward_fill(1), x.fill_null(strategy="forward", limit=2)] + \
             [x.fill_null(strategy=op) for op in STRATEGIES]:
        assert f.over("k").kind == "over"
        assert f.alias("y").over("k", "j").value == ("k", "j")
    assert (x - x.mean().over("k")).forward_fill().over("k").kind == "over"
    # plain composition outside over(): the node is rowwise
    assert pl.col("x").forward_fill().diff().kind == "lag"
    assert pl.col("x").forward_fill().cum_sum().kind == "cum"
    assert pl.col("x").shift(1).backward_fill().kind == "fill"
    assert pl.col("x").forward_fill().rolling_mean(3).kind == "rolling"


# ----------------------------------------------------------------- refusals
@pytest.mark.parametrize("build, reason", [
    (lambda: pl.col("c").forward_fill(-1), "non-negative"),
    (lambda: pl.col("c").backward_fill(-3), "non-negative"),
    (lambda: pl.col("c").fill_null(strategy="forward", limit=-1), "non-negative"),
    (lambda: pl.col("c").forward_fill(1.5), "non-negative integer"),
    (lambda: pl.col("c").forward_fill(True), "non-negative integer"),
    (lambda: pl.col("c").forward_fill(pl.col("n")), "computed `limit`"),
    (lambda: pl.col("c").fill_null(), "needs a fill `value` or a `strategy`"),
    (lambda: pl.col("c").fill_null(None), "needs a fill `value` or a `strategy`"),
    (lambda: pl.col("c").forward_fill().sum(), "inside an aggregation"),
    (lambda: (pl.col("c") - pl.col("c").backward_fill()).max(), "inside an aggregation"),
    (lambda: pl.col("c").fill_null(strategy="zero").mean(), "inside an aggregation"),
    (lambda: pl.col("c").sum().forward_fill(), "must be an elementwise expression"),
    (lambda: pl.col("c").sort().backward_fill(), "must be an elementwise expression"),
    (lambda: pl.col("c").max().fill_null(strategy="min"), "must be an elementwise expression"),
    # inside over() only an elementwise input is taken
    (lambda: pl.col("c").shift(1).forward_fill().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").forward_fill().diff().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").forward_fill().backward_fill().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").forward_fill().over("a").over("b"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").forward_fill().over("a").sum(), "inside an aggregation"),
])
def test_refusals(build, reason):
    with pytest.raises(pl.InvalidOperationError) as ei:
        build()
    assert reason in str(ei.value)


@pytest.mark.parametrize("build, reason", [
    (lambda: pl.col("c").fill_null(1, strategy="forward"), "cannot specify both"),
    (lambda: pl.col("c").fill_null(pl.col("d"), strategy="zero"), "cannot specify both"),
    (lambda: pl.col("c").fill_null(strategy="max", limit=2), "can only specify `limit`"),
    (lambda: pl.col("c").fill_null(strategy="zero", limit=0), "can only specify `limit`"),
    (lambda: pl.col("c").fill_null(3, limit=1), "can only specify `limit`"),
    (lambda: pl.col("c").fill_null(strategy="nearest"), "strategy"),
    (lambda: pl.col("c").fill_null(strategy="Forward"), "strategy"),
])
def test_value_errors(build, reason):
    with pytest.raises(ValueError) as ei:
        build()
    assert reason in str(ei.value)


def test_over_message_names_the_fill_family():
    with pytest.raises(pl.InvalidOperationError) as ei:
        pl.col("c").over("a")
    assert "forward_fill / backward_fill" in str(ei.value)


class _Cols:
    def __init__(self, columns):
        self.columns = columns


def test_filter_predicate_and_explain():
    lf = pl.LazyFrame(("scan", _Cols(["a", "b"])))
    for pred in (pl.col("b").forward_fill() > 0, pl.col("b").fill_null(strategy="zero") > 0,
                 pl.col("b").backward_fill(1).is_null()):
        with pytest.raises(pl.InvalidOperationError) as ei:
            lf.filter(pred)
        assert "filter predicate" in str(ei.value) and "forward_fill" in str(ei.value)
    text = lf.with_columns(pl.col("b").forward_fill().over("a"), pl.col("b").backward_fill(2).alias("p")).explain()
    assert '.forward_fill(limit=None).over([col("a")])' in text and ".backward_fill(limit=2)" in text


def test_group_by_agg_refuses_the_fill_nodes():
    from polaroid_amd import frame as F

    one = type("_Col", (), {"dtype": pl.Int64})()

    class _Frame:
        _cols = {"k": one, "v": one}
        columns = ["k", "v"]
        height = 0

    for e in (pl.col("v").forward_fill(), pl.col("v").backward_fill(1).alias("p"),
              pl.col("v").fill_null(strategy="mean")):
        with pytest.raises(pl.InvalidOperationError) as ei:
            F._gb_lower(_Frame(), "k", [e], None)
        assert "not an aggregation" in str(ei.value)


# ------------------------------------------------------------------- plugin
def _fill_fn(strategy, limit=None):
    """FunctionExpr::FillNullWithStrategy as the visitor hands it over: the
    limit in the tuple, the column as the only input."""
    return lambda nt, inputs: nt.e("Function", function_data=("fill_null_with_strategy", strategy, limit),
                                   input=inputs, options=None)


def _ir(function, inputs, node_kind="HStack", window=False, wrap=None, table=None, dtypes=None):
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


_ACCEPTED = [("forward", None), ("forward", 0), ("forward", 3), ("backward", None), ("backward", 2),
             ("min", None), ("max", None), ("mean", None), ("zero", None), ("one", None)]


@pytest.mark.parametrize("node_kind", ["HStack", "Select"])
@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("strategy, limit", _ACCEPTED, ids=[f"{s}-{l}" for s, l in _ACCEPTED])
def test_translate_accepted_forms(strategy, limit, window, node_kind):
    nt = _ir(_fill_fn(strategy, limit), [_c("v")], node_kind, window)
    plan = PE.translate(nt)
    assert plan[0] == ("with_columns" if node_kind == "HStack" else "select")
    (e,) = plan[2]
    assert e.output_name() == "out"
    f = e.args[0]
    if window:
        assert f.kind == "over" and f.value == ("k",)
        f = f.args[0]
    assert (f.kind, f.op, f.value) == ("fill", strategy, (limit,))
    assert f.args[0].kind == "col"
    PE.execute_with_polaroid(nt, None)
    assert callable(nt.udf)


def test_fill_null_with_a_value_is_unchanged():
    fn = lambda nt, inputs: nt.e("Function", function_data=("fill_null",), input=inputs, options=None)  # noqa: E731
    nt = _ir(fn, [_c("v"), lambda t: t.lit(0.0)])
    e = PE.translate(nt)[2][0].args[0]
    assert e.kind == "fill_null"


@pytest.mark.parametrize("dtype", ["Int8", "UInt16", "Int32", "UInt64", "Float32", "Date",
                                   "Datetime(time_unit='ns', time_zone=None)", "Duration(time_unit='us')",
                                   "Categorical"])
def test_translate_dtypes_the_series_layer_takes(dtype):
    for window in (False, True):
        nt = _ir(_fill_fn("forward", 1), [_c("v")], window=window, dtypes={"v": dtype})
        f = PE.translate(nt)[2][0].args[0]
        assert (f.args[0] if window else f).kind == "fill"


def test_translate_a_composition():
    """x / x.forward_fill().over(k) - 1; a fill below another row-order
    function stays on polars, as a cum_* / shift / diff there does."""
    nt = _ir(_fill_fn("forward"), [_c("v")], window=True,
             wrap=lambda t, w: t.bin(t.bin(t.col("v"), "TrueDivide", w), "Minus", t.lit(1)))
    e = PE.translate(nt)[2][0].args[0]
    assert e.kind == "bin" and e.args[0].args[1].kind == "over" and e.args[0].args[1].args[0].kind == "fill"

    def nested(t, ff):
        return t.e("Function", function_data=("shift",), input=[ff, t.lit(1)], options=None)

    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(_ir(_fill_fn("forward"), [_c("v")], wrap=nested))
    assert "outside the expressions" in str(ei.value)


def _below_agg(nt, top):
    return nt.e("Agg", name="sum", arguments=[top], options=None)


def _string_table():
    import pyarrow as pa

    return pa.table({"k": pa.array([1, 1, 2]), "v": pa.array(["x", None, "z"]), "w": pa.array([True, None, True])})


@pytest.mark.parametrize("kw, reason", [
    (dict(function=_fill_fn("forward"), inputs=[_c("v")], table="str"), "fill_null of a String"),
    (dict(function=_fill_fn("backward", 1), inputs=[_c("v")], table="str", window=True), "fill_null of a String"),
    (dict(function=_fill_fn("min"), inputs=[_c("v")], table="str"), "fill_null of a String"),
    (dict(function=_fill_fn("forward"), inputs=[_c("w")], table="str"), "fill_null of a Boolean"),
    (dict(function=_fill_fn("zero"), inputs=[_c("w")], table="str", window=True), "fill_null of a Boolean"),
    (dict(function=_fill_fn("max"), inputs=[_c("v")], dtypes={"v": "Categorical"}), "fill_null of a String"),
    (dict(function=_fill_fn("forward"), inputs=[_c("v")], dtypes={"v": "Time"}), "dtype Time"),  # refused at the scan
    (dict(function=_fill_fn("mean"), inputs=[_c("v")], dtypes={"v": "Date"}), "strategy='mean') of a Date"),
    (dict(function=_fill_fn("mean"), inputs=[_c("v")], dtypes={"v": "Duration(time_unit='us')"}),
     "strategy='mean') of a Duration"),
    (dict(function=_fill_fn("forward", -1), inputs=[_c("v")]), "non-negative"),
    (dict(function=_fill_fn("nearest"), inputs=[_c("v")]), "strategy"),
    (dict(function=_fill_fn("forward"), inputs=[_c("v")], wrap=_below_agg, node_kind="Select"),
     "outside the expressions"),
    (dict(function=_fill_fn("zero"), inputs=[_c("v")], wrap=_below_agg, node_kind="Select"),
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
    d = nt.e("Function", function_data=("fill_null_with_strategy", "forward", None), input=[nt.col("v")], options=None)
    nt.p("Filter", ["k", "v", "w"], input=scan, predicate=PyExprIR(nt.bin(d, "Gt", nt.lit(0.0)), "v"))
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert "outside the expressions" in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None
    nt = FakeNT(table)
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(table), projection=None, selection=None)
    ff = nt.e("Function", function_data=("fill_null_with_strategy", "backward", 1), input=[nt.col("v")], options=None)
    a = nt.e("Agg", name="max", arguments=[ff], options=False)
    opts = _node("GroupbyOptions", slice=None, dynamic=None, rolling=None)
    nt.p("GroupBy", ["k", "out"], input=scan, keys=[PyExprIR(nt.col("k"), "k")], aggs=[PyExprIR(a, "out")],
         apply=None, maintain_order=True, options=opts)
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert "outside the expressions" in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None


# ------------------------------------------------- C entry point, no GPU
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
    assert N.FILL == {"forward": 1, "backward": 2}
    assert "plgpu_fill" in N.SIGNATURES and len(N.SIGNATURES["plgpu_fill"][1]) == 6
    # the fill kernels' tile is the scans': one geometry in the shared header, none of its own
    import os
    import re

    from conftest import ROOT

    csrc = os.path.join(ROOT, "polaroid_amd", "csrc")
    src = open(os.path.join(csrc, "seg_scan.hpp")).read()
    th = int(re.search(r"kTileThreads = (\d+);", src).group(1))
    per = int(re.search(r"kTilePer = (\d+);", src).group(1))
    blocks = int(re.search(r"kTileBlocks = (\d+);", src).group(1))
    totals = int(re.search(r"kTotalsThreads = (\d+);", src).group(1))
    assert th * per == N.CUM_BLOCK and th * per * blocks == N.CUM_TILE == 16384
    assert N.CUM_THREADS == th and N.CUM_TOTALS_THREADS == totals
    for f in ("cumulative.hip", "fill.hip", "ewm.hip"):
        assert not re.search(r"k(Cum|Fill|Ewm)(Threads|Per|Blocks?|Tile|Words|TotalsThreads)\b", open(os.path.join(csrc, f)).read())


def test_fill_argument_checks(N):
    L = N.lib()
    out = N.Column()
    v = _host_col(N, N.F64, 8, nullable=True)

    def call(values, starts, kind=N.FILL["forward"], limit=-1):
        return L.plgpu_fill(values, starts, kind, limit, C.byref(out), None)

    assert call(None, None) == N.ERR_INVALID
    assert L.plgpu_fill(C.byref(v), None, 1, -1, None, None) == N.ERR_INVALID
    assert call(C.byref(v), None, kind=0) == N.ERR_INVALID
    assert call(C.byref(v), None, kind=3) == N.ERR_INVALID
    assert "kind" in L.plgpu_last_error().decode()
    for dt in (N.STR, N.BOOL, N.I8, N.I16, N.U8, N.U16):
        for kind in N.FILL.values():
            assert call(C.byref(_host_col(N, dt, 8, nullable=True)), None, kind=kind) == N.ERR_SCHEMA, (dt, kind)
    assert L.plgpu_last_error()
    assert call(C.byref(v), C.byref(_host_col(N, N.I64, 8))) == N.ERR_INVALID          # starts not Boolean
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 8, nullable=True))) == N.ERR_INVALID
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 9))) == N.ERR_INVALID          # lengths differ
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 7)), kind=N.FILL["backward"]) == N.ERR_INVALID
    assert "segment starts" in L.plgpu_last_error().decode()
    assert L.plgpu_abi_version() == 1


# ------------------------------------------------------------------ golden
def test_golden_file_shape():
    g = load_golden("fill_cases.json")
    assert g["cases"], "no cases"
    names = set()
    for c in g["cases"]:
        assert set(c) >= {"name", "source", "op", "limit", "dtype", "values", "expected",
                          "expected_dtype"}, c.get("name")
        assert c["name"] not in names
        names.add(c["name"])
        assert ":" in c["source"] and c["source"].split(":")[0].endswith(".py")
        assert c["op"] in STRATEGIES
        assert c["limit"] is None or (isinstance(c["limit"], int) and c["op"] in ("forward", "backward"))
        assert c.get("method") in (None, f"{c['op']}_fill")
        assert len(c["values"]) == len(c["expected"])
        if "keys" in c:
            assert len(c["keys"]) == len(c["values"])
        if "chunks" in c:
            assert [x for ch in c["chunks"] for x in ch] == c["values"]
        # forward / backward only move values: every expected value occurs in the input
        if c["op"] in ("forward", "backward"):
            assert set(x for x in c["expected"] if x is not None) <= set(x for x in c["values"] if x is not None)
            assert all(e == v for e, v in zip(c["expected"], c["values"]) if v is not None)
    sources = {c["source"].split(":")[0] for c in g["cases"]}
    assert sources >= {"series/test_series.py", "dataframe/test_df.py", "lazyframe/test_lazyframe.py",
                       "operations/test_fill_null.py", "operations/test_group_by.py"}


def _ref_fill(values, op, limit):
    """The index loops of fill_forward_gather_limit / fill_backward_gather_limit
    (fill_null.rs:258 / :304) on a list."""
    n = len(values)
    lim = n if limit is None else limit
    out = list(values)
    last, cnt = None, 0
    for i in (range(n - 1, -1, -1) if op == "backward" else range(n)):
        if values[i] is not None:
            last, cnt = values[i], 0
        elif cnt < lim:
            cnt += 1
            out[i] = last
    return out


def test_golden_forward_backward_cases_follow_the_reference_loops():
    for c in load_golden("fill_cases.json")["cases"]:
        if c["op"] not in ("forward", "backward"):
            continue
        exp = list(c["values"])
        keys = c.get("keys", [0] * len(exp))
        for g in {repr(k) for k in keys}:
            rows = [i for i, k in enumerate(keys) if repr(k) == g]
            for i, v in zip(rows, _ref_fill([c["values"][i] for i in rows], c["op"], c["limit"])):
                exp[i] = v
        assert exp == c["expected"], c["name"]
