"""CPU: window expressions over groups (Expr.over) -- construction, names,
repr / explain, every refusal; the plugin's translation of the visitor's
Window node (expr_nodes.rs:400) against the NodeTraverser model of
tests/test_polars_engine.py; and the argument checks of the three C entry
points (plgpu_segment_starts, plgpu_rolling_segmented,
plgpu_invert_permutation), which run before any device work."""

import ctypes as C

import pytest

import polaroid_amd as pl
from polaroid_amd import polars_engine as PE
from test_polars_engine import FakeNT, FakePolarsDF, PyExprIR, _node, _table


# ------------------------------------------------------------ construction
def test_over_takes_names_lists_and_columns():
    f = pl.col("c").max()
    forms = [f.over("a", "b"), f.over(["a", "b"]), f.over(pl.col("a"), pl.col("b")), f.over([pl.col("a"), "b"]),
             f.over("a", ["b"])]
    for e in forms:
        assert e.kind == "over" and e.value == ("a", "b")
        assert e.args[0] is f
    assert f.over("a").value == ("a",)


def test_over_names_roots_and_repr():
    e = pl.col("c").max().over("a", "b")
    assert e.output_name() == "c"
    assert e.meta_root_names() == ["c", "a", "b"]
    assert repr(e) == 'col("c").max().over([col("a"), col("b")])'
    assert e.alias("m").output_name() == "m"
    assert pl.len().over("a").output_name() == "len"
    assert pl.len().over("a").meta_root_names() == ["a"]
    r = pl.col("close").rolling_mean(20, min_samples=1).over("symbol")
    assert r.output_name() == "close"
    assert r.meta_root_names() == ["close", "symbol"]
    assert "rolling_mean" in repr(r) and repr(r).endswith('.over([col("symbol")])')
    nested = pl.col("b") - pl.col("b").mean().over("a")
    assert nested.output_name() == "b"
    assert nested.meta_root_names() == ["b", "a"]
    assert (pl.col("x") * pl.col("y")).sum().over("k").meta_root_names() == ["x", "y", "k"]
    assert pl.col("x").std(ddof=0).over("k").args[0].value == 0


def test_over_in_explain():
    lf = pl.LazyFrame(("scan", _Cols(["a", "b"])))
    text = lf.with_columns(pl.col("b").rolling_sum(2).over("a"), pl.len().over("a")).explain()
    assert "WITH_COLUMNS" in text
    assert '.over([col("a")])' in text and "len().over" in text


class _Cols:
    """Stands in for a scanned frame where explain only reads its columns."""

    def __init__(self, columns):
        self.columns = columns


# ----------------------------------------------------------------- refusals
@pytest.mark.parametrize("build, reason", [
    (lambda: pl.col("c").max().over(pl.col("a") + 1), "computed partition keys"),
    (lambda: pl.col("c").max().over("a", pl.col("b").abs()), "computed partition keys"),
    (lambda: pl.col("c").max().over("a", order_by="b"), "order_by"),
    (lambda: pl.col("c").max().over("a", mapping_strategy="join"), "mapping_strategy"),
    (lambda: pl.col("c").max().over("a", mapping_strategy="explode"), "mapping_strategy"),
    (lambda: pl.col("c").rolling_mean(3).over("a").sum(), "inside an aggregation"),
    (lambda: (pl.col("c") - pl.col("c").mean().over("a")).max(), "inside an aggregation"),
    (lambda: pl.col("c").over("a"), "only rolling_* functions and the aggregations"),
    (lambda: (pl.col("c") + 1).over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").sort().over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").max().over("a").over("b"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").sum().rolling_mean(2).over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").rolling_mean(2).rolling_sum(2).over("a"), "only rolling_* functions and the aggregations"),
    (lambda: pl.col("c").max().over([]), "1..8 plain key columns"),
    (lambda: pl.col("c").max().over(*"abcdefghi"), "1..8 plain key columns"),
    (lambda: pl.col("c").max().over(3), "partition key"),
])
def test_over_refusals(build, reason):
    with pytest.raises(pl.InvalidOperationError) as ei:
        build()
    assert reason in str(ei.value)


def test_over_in_a_filter_predicate_is_refused():
    lf = pl.LazyFrame(("scan", _Cols(["a", "b"])))
    with pytest.raises(pl.InvalidOperationError) as ei:
        lf.filter(pl.col("b") > pl.col("b").mean().over("a"))
    assert "filter predicate" in str(ei.value)
    assert lf.filter(pl.col("b") > 1)._node[0] == "filter"


def test_over_duplicate_keys():
    with pytest.raises(pl.DuplicateError):
        pl.col("c").max().over("a", "a")


def test_over_accepts_every_listed_function():
    x = pl.col("close") * pl.col("volume")
    for name in ("sum", "mean", "min", "max", "count", "len", "first", "last"):
        assert getattr(x, name)().over("k").kind == "over"
    for name in ("std", "var"):
        assert getattr(x, name)(ddof=0).over("k").kind == "over"
    for name in ("sum", "mean", "min", "max", "var", "std"):
        assert getattr(x, "rolling_" + name)(5, min_samples=1).over("k").kind == "over"
    assert pl.len().over("k").kind == "over"
    # the rolling input may itself hold a window expression (it is elementwise)
    assert (x - x.mean().over("k")).rolling_mean(3).over("k").kind == "over"


# ------------------------------------------------------------------- plugin
def _window_ir(table, function, partition_by, node_kind="HStack", order_by=None, kind="groups_to_rows",
               wrap=None):
    """df.lazy().with_columns / select(<function>.over(partition_by))"""
    nt = FakeNT(table)
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(table), projection=None, selection=None)
    fn = function(nt)
    win = nt.e("Window", function=fn, partition_by=[p(nt) for p in partition_by], order_by=order_by,
               order_by_descending=False, order_by_nulls_last=False,
               options=type("WindowMapping", (), {"kind": kind})())  # PyWindowMapping.kind (expr_nodes.rs:423)
    top = wrap(nt, win) if wrap else win
    if node_kind == "HStack":
        nt.p("HStack", ["k", "v", "w", "out"], input=scan, exprs=[PyExprIR(top, "out")])
    else:
        nt.p("Select", ["out"], input=scan, expr=[PyExprIR(top, "out")])
    return nt


def _agg(name, column, options=None):
    return lambda nt: nt.e("Agg", name=name, arguments=[nt.col(column)], options=options)


def _colref(name):
    return lambda nt: nt.col(name)


def test_translate_window_in_hstack():
    nt = _window_ir(_table()[0], _agg("sum", "v"), [_colref("k")])
    plan = PE.translate(nt)
    assert plan[0] == "with_columns" and plan[1][0] == "polars_scan"
    (e,) = plan[2]
    assert e.output_name() == "out"
    w = e.args[0]
    assert w.kind == "over" and w.value == ("k",)
    assert w.args[0].kind == "agg" and w.args[0].op == "sum" and w.args[0].meta_root_names() == ["v"]


def test_translate_window_in_select_two_partition_columns():
    nt = _window_ir(_table()[0], _agg("std", "v", options=1), [_colref("k"), _colref("w")], node_kind="Select")
    plan = PE.translate(nt)
    assert plan[0] == "select"
    w = plan[2][0].args[0]
    assert w.kind == "over" and w.value == ("k", "w")
    assert w.args[0].op == "std" and w.args[0].value == 1


def test_translate_len_window_and_nested_window():
    nt = _window_ir(_table()[0], lambda t: t.e("Len"), [_colref("k")])
    w = PE.translate(nt)[2][0].args[0]
    assert w.kind == "over" and w.args[0].kind == "len"
    # v - v.mean().over(k)
    nt = _window_ir(_table()[0], _agg("mean", "v"), [_colref("k")],
                    wrap=lambda t, win: t.bin(t.col("v"), "Minus", win))
    e = PE.translate(nt)[2][0].args[0]
    assert e.kind == "bin" and e.args[1].kind == "over"


@pytest.mark.parametrize("kw, reason", [
    (dict(function=_agg("median", "v")), "aggregation median"),
    (dict(function=_colref("v")), "window function Column"),
    (dict(function=_agg("min", "v", options=True)), "NaN propagation"),
    (dict(partition_by=[lambda nt: nt.bin(nt.col("k"), "Plus", nt.lit(1))]), "partitioned by an expression"),
    (dict(order_by=0), "order_by"),
    (dict(kind="join"), "window mapping join"),
    (dict(kind="explode"), "window mapping explode"),
])
def test_unsupported_windows_stay_on_polars(kw, reason):
    args = dict(function=_agg("sum", "v"), partition_by=[_colref("k")])
    args.update(kw)
    nt = _window_ir(_table()[0], **args)
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert reason in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None  # polars keeps the query


def test_window_dtype_gates_apply_as_in_group_by():
    import pyarrow as pa

    table = pa.table({"k": pa.array([1, 1, 2]), "v": pa.array(["x", "y", "z"]), "w": pa.array([True, False, True])})
    for fn, reason in ((_agg("max", "v"), "String"), (_agg("min", "w"), "Boolean")):
        nt = _window_ir(table, fn, [_colref("k")])
        with pytest.raises(PE.Unsupported) as ei:
            PE.translate(nt)
        assert reason in str(ei.value)


def _window_elsewhere(where):
    """A Window node where the mirror does not lower one: in the input of a
    group-by's aggregation, of a select of aggregations, of another window's
    aggregation, and in a Filter predicate."""
    nt = FakeNT(_table()[0])
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(_table()[0]), projection=None, selection=None)

    def win():
        return nt.e("Window", function=_agg("mean", "v")(nt), partition_by=[nt.col("k")], order_by=None,
                    order_by_descending=False, order_by_nulls_last=False,
                    options=type("WindowMapping", (), {"kind": "groups_to_rows"})())

    if where == "filter":  # filter(v > v.mean().over(k))
        nt.p("Filter", ["k", "v", "w"], input=scan, predicate=PyExprIR(nt.bin(nt.col("v"), "Gt", win()), "v"))
        return nt
    # (v - v.mean().over(k)).sum()
    a = nt.e("Agg", name="sum", arguments=[nt.bin(nt.col("v"), "Minus", win())], options=None)
    if where == "group_by":
        opts = _node("GroupbyOptions", slice=None, dynamic=None, rolling=None)
        nt.p("GroupBy", ["k", "out"], input=scan, keys=[PyExprIR(nt.col("k"), "k")], aggs=[PyExprIR(a, "out")],
             apply=None, maintain_order=True, options=opts)
    elif where == "select_aggs":
        nt.p("Select", ["out"], input=scan, expr=[PyExprIR(a, "out")])
    else:  # (v - v.mean().over(k)).sum().over(k) in with_columns
        outer = nt.e("Window", function=a, partition_by=[nt.col("k")], order_by=None, order_by_descending=False,
                     order_by_nulls_last=False, options=type("WindowMapping", (), {"kind": "groups_to_rows"})())
        nt.p("HStack", ["k", "v", "w", "out"], input=scan, exprs=[PyExprIR(outer, "out")])
    return nt


@pytest.mark.parametrize("where", ["group_by", "select_aggs", "window_in_window", "filter"])
def test_window_outside_select_expressions_stays_on_polars(where):
    nt = _window_elsewhere(where)
    with pytest.raises(PE.Unsupported) as ei:
        PE.translate(nt)
    assert "window outside" in str(ei.value)
    PE.execute_with_polaroid(nt, None)
    assert nt.udf is None  # polars keeps the query


def test_window_after_an_aggregation_input_is_still_translated():
    """The gate holds for the aggregation's input alone: a later expression
    of the same with_columns still takes its window."""
    nt = FakeNT(_table()[0])
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(_table()[0]), projection=None, selection=None)
    mapping = type("WindowMapping", (), {"kind": "groups_to_rows"})()
    # (v * w).sum().over(k), then v.mean().over(k)
    a = nt.e("Agg", name="sum", arguments=[nt.bin(nt.col("v"), "Multiply", nt.col("w"))], options=None)
    w1 = nt.e("Window", function=a, partition_by=[nt.col("k")], order_by=None, order_by_descending=False,
              order_by_nulls_last=False, options=mapping)
    w2 = nt.e("Window", function=_agg("mean", "v")(nt), partition_by=[nt.col("k")], order_by=None,
              order_by_descending=False, order_by_nulls_last=False, options=mapping)
    nt.p("HStack", ["k", "v", "w", "a", "b"], input=scan, exprs=[PyExprIR(w1, "a"), PyExprIR(w2, "b")])
    plan = PE.translate(nt)
    assert [e.args[0].kind for e in plan[2]] == ["over", "over"]


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


def test_segment_starts_argument_checks(N):
    L = N.lib()
    out, srt = N.Column(), C.c_int32(7)
    keys = (N.Column * 2)(_host_col(N, N.I64, 4), _host_col(N, N.I32, 4))
    assert L.plgpu_segment_starts(None, 1, C.byref(out), C.byref(srt), None) == N.ERR_INVALID
    assert L.plgpu_segment_starts(keys, 1, None, C.byref(srt), None) == N.ERR_INVALID
    assert L.plgpu_segment_starts(keys, 1, C.byref(out), None, None) == N.ERR_INVALID
    assert L.plgpu_segment_starts(keys, 0, C.byref(out), C.byref(srt), None) == N.ERR_INVALID
    assert L.plgpu_segment_starts(keys, 9, C.byref(out), C.byref(srt), None) == N.ERR_INVALID
    bad = (N.Column * 1)(_host_col(N, N.STR, 4))
    assert L.plgpu_segment_starts(bad, 1, C.byref(out), C.byref(srt), None) == N.ERR_SCHEMA
    uneven = (N.Column * 2)(_host_col(N, N.I64, 4), _host_col(N, N.I64, 5))
    assert L.plgpu_segment_starts(uneven, 2, C.byref(out), C.byref(srt), None) == N.ERR_SHAPE
    assert L.plgpu_last_error()


def test_rolling_segmented_argument_checks(N):
    L = N.lib()
    out = N.Column()
    v, seg = _host_col(N, N.F64, 8), _host_col(N, N.BOOL, 8)
    SUM, VAR = N.ROLLING["sum"], N.ROLLING["var"]

    def call(values, starts, kind=SUM, w=3, ms=1):
        return L.plgpu_rolling_segmented(values, starts, kind, w, ms, 0, C.byref(out), None)

    assert call(None, C.byref(seg)) == N.ERR_INVALID
    assert call(C.byref(v), None) == N.ERR_INVALID
    assert L.plgpu_rolling_segmented(C.byref(v), C.byref(seg), SUM, 3, 1, 0, None, None) == N.ERR_INVALID
    assert call(C.byref(_host_col(N, N.STR, 8)), C.byref(seg)) == N.ERR_SCHEMA       # value dtype
    assert call(C.byref(_host_col(N, N.U64, 8)), C.byref(seg)) == N.ERR_SCHEMA
    assert call(C.byref(v), C.byref(_host_col(N, N.I64, 8))) == N.ERR_SCHEMA         # starts not Boolean
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 8, nullable=True))) == N.ERR_SCHEMA
    assert call(C.byref(v), C.byref(_host_col(N, N.BOOL, 9))) == N.ERR_SHAPE         # lengths differ
    assert call(C.byref(v), C.byref(seg), w=3, ms=4) == N.ERR_INVALID                # min_periods > window
    assert call(C.byref(v), C.byref(seg), w=0) == N.ERR_INVALID
    assert call(C.byref(v), C.byref(seg), kind=SUM | (1 << 8)) == N.ERR_INVALID      # ddof outside var / std
    assert call(C.byref(v), C.byref(seg), kind=99) == N.ERR_INVALID
    assert VAR | (1 << 8)  # (ddof with var is valid: it reaches the device, not tested here)
    assert L.plgpu_last_error()


def test_invert_permutation_argument_checks(N):
    L = N.lib()
    out = N.Column()
    assert L.plgpu_invert_permutation(None, C.byref(out), None) == N.ERR_INVALID
    assert L.plgpu_invert_permutation(C.byref(_host_col(N, N.U32, 4)), None, None) == N.ERR_INVALID
    assert L.plgpu_invert_permutation(C.byref(_host_col(N, N.I64, 4)), C.byref(out), None) == N.ERR_SCHEMA
    assert L.plgpu_invert_permutation(C.byref(_host_col(N, N.U32, 4, nullable=True)), C.byref(out), None) \
        == N.ERR_SCHEMA


def test_over_presorted_option_round_trip(N):
    prev = N.set_option("over_presorted", 0)
    assert prev == 1
    v = C.c_int64(-1)
    assert N.lib().plgpu_get_option(b"over_presorted", C.byref(v)) == 0 and v.value == 0
    assert N.set_option("over_presorted", prev) == 0
