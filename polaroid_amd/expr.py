"""Expression DSL mirroring py-polars' `pl.col` / `pl.lit` / Expr API for the
filter -> arithmetic/comparison -> group_by-agg path.

An Expr is lowered to the postfix program of include/polaroid_gpu.h
(`plgpu_instr`), which the native library type-checks and runs per row on
the GPU (reference: polars-expr/src/expressions/{column,literal,binary}.rs).
"""

from __future__ import annotations

import builtins
from typing import Any, Sequence

from . import _native as N

_AGG_KINDS = ("sum", "mean", "min", "max", "count", "len")


class Expr:
    """A node of the expression tree."""

    __slots__ = ("kind", "args", "op", "value", "_name")

    def __init__(self, kind: str, args: Sequence["Expr"] = (), op: str | None = None,
                 value: Any = None, name: str | None = None):
        self.kind = kind          # col | lit | bin | un | agg | alias | len | rolling | cum | lag | fill | ewm | rank | over | ...
        self.args = tuple(args)
        self.op = op
        self.value = value
        self._name = name

    # ---------------------------------------------------------- naming
    def output_name(self) -> str:
        if self.kind == "alias":
            return self.value
        if self.kind == "col":
            return self.value
        if self.kind == "len":
            return "len"
        if self.kind == "lit":
            return "literal"
        if self.kind == "ternary":  # when/then/otherwise is named after its first then()
            return self.args[1].output_name()
        return self.args[0].output_name()

    def meta_root_names(self) -> list[str]:
        if self.kind == "col":
            return [self.value]
        out: list[str] = []
        for a in self.args:
            for n in a.meta_root_names():
                if n not in out:
                    out.append(n)
        if self.kind == "over":  # the function's columns, then the partition keys
            for n in self.value:
                if n not in out:
                    out.append(n)
        return out

    def __repr__(self) -> str:
        if self.kind == "col":
            return f'col("{self.value}")'
        if self.kind == "lit":
            return f"lit({self.value!r})"
        if self.kind == "bin":
            return f"[({self.args[0]!r}) {self.op} ({self.args[1]!r})]"
        if self.kind == "alias":
            return f'{self.args[0]!r}.alias("{self.value}")'
        if self.kind == "len":
            return "len()"
        if self.kind == "rolling":
            return f"{self.args[0]!r}.rolling_{self.op}{self.value}"
        if self.kind == "cum":
            return f"{self.args[0]!r}.cum_{self.op}()"
        if self.kind == "lag":
            return f"{self.args[0]!r}.{self.op}{self.value}"
        if self.kind == "fill":
            if self.op in ("forward", "backward"):
                return f"{self.args[0]!r}.{self.op}_fill(limit={self.value[0]!r})"
            return f"{self.args[0]!r}.fill_null(strategy={self.op!r})"
        if self.kind == "ewm":
            alpha, adjust, min_samples, ignore_nulls = self.value
            return (f"{self.args[0]!r}.ewm_{self.op}(alpha={alpha!r}, adjust={adjust}, min_samples={min_samples}, "
                    f"ignore_nulls={ignore_nulls})")
        if self.kind == "rank":
            return f"{self.args[0]!r}.rank(method={self.op!r}, descending={self.value[0]})"
        if self.kind == "over":
            keys = ", ".join(f'col("{k}")' for k in self.value)
            return f"{self.args[0]!r}.over([{keys}])"
        if self.kind == "ternary":
            return f"when({self.args[0]!r}).then({self.args[1]!r}).otherwise({self.args[2]!r})"
        if self.kind == "cast":
            return f"{self.args[0]!r}.cast({self.value!r}, {self.op})"
        if self.kind == "fill_null":
            return f"{self.args[0]!r}.fill_null({self.args[1]!r})"
        if self.kind == "agg" and self.op == "quantile":
            return f"{self.args[0]!r}.quantile({self.value[0]!r}, interpolation={self.value[1]!r})"
        return f"{self.args[0]!r}.{self.op}()"

    def __bool__(self):
        raise TypeError("the truth value of an Expr is ambiguous")

    # -------------------------------------------------------- operators
    def _bin(self, op: str, other: Any, swap: bool = False) -> "Expr":
        o = _to_expr(other)
        return Expr("bin", (o, self) if swap else (self, o), op=op)

    def __add__(self, o): return self._bin("+", o)
    def __radd__(self, o): return self._bin("+", o, True)
    def __sub__(self, o): return self._bin("-", o)
    def __rsub__(self, o): return self._bin("-", o, True)
    def __mul__(self, o): return self._bin("*", o)
    def __rmul__(self, o): return self._bin("*", o, True)
    def __truediv__(self, o): return self._bin("/", o)
    def __rtruediv__(self, o): return self._bin("/", o, True)
    def __floordiv__(self, o): return self._bin("//", o)
    def __rfloordiv__(self, o): return self._bin("//", o, True)
    def __mod__(self, o): return self._bin("%", o)
    def __rmod__(self, o): return self._bin("%", o, True)
    def __xor__(self, o): return self._bin("^", o)
    def __rxor__(self, o): return self._bin("^", o, True)
    def __gt__(self, o): return self._bin(">", o)
    def __ge__(self, o): return self._bin(">=", o)
    def __lt__(self, o): return self._bin("<", o)
    def __le__(self, o): return self._bin("<=", o)
    def __eq__(self, o): return self._bin("==", o)  # type: ignore[override]
    def __ne__(self, o): return self._bin("!=", o)  # type: ignore[override]
    def __and__(self, o): return self._bin("&", o)
    def __rand__(self, o): return self._bin("&", o, True)
    def __or__(self, o): return self._bin("|", o)
    def __ror__(self, o): return self._bin("|", o, True)
    def __neg__(self): return Expr("un", (self,), op="neg")
    def __abs__(self): return Expr("un", (self,), op="abs")
    def __invert__(self): return Expr("un", (self,), op="not")
    __hash__ = object.__hash__

    def gt(self, o): return self._bin(">", o)
    def ge(self, o): return self._bin(">=", o)
    def lt(self, o): return self._bin("<", o)
    def le(self, o): return self._bin("<=", o)
    def eq(self, o): return self._bin("==", o)
    def ne(self, o): return self._bin("!=", o)
    def eq_missing(self, o): return self._bin("eq_missing", o)
    def ne_missing(self, o): return self._bin("ne_missing", o)
    def add(self, o): return self._bin("+", o)
    def sub(self, o): return self._bin("-", o)
    def mul(self, o): return self._bin("*", o)
    def truediv(self, o): return self._bin("/", o)
    def floordiv(self, o): return self._bin("//", o)
    def mod(self, o): return self._bin("%", o)
    def xor(self, o): return self._bin("^", o)
    def and_(self, o): return self._bin("&", o)
    def or_(self, o): return self._bin("|", o)
    def not_(self): return Expr("un", (self,), op="not")
    def abs(self): return Expr("un", (self,), op="abs")
    def is_null(self): return Expr("un", (self,), op="is_null")
    def is_not_null(self): return Expr("un", (self,), op="is_not_null")
    def is_nan(self): return Expr("un", (self,), op="is_nan")
    def is_finite(self): return Expr("un", (self,), op="is_finite")

    @property
    def str(self) -> "_StrNamespace":
        """String functions (Expr.str): literal pattern tests."""
        return _StrNamespace(self)

    def cast(self, dtype, *, strict: bool = True, wrap_numerical: bool = False) -> "Expr":
        """Expr.cast.  Non-strict: a value that does not fit becomes null;
        wrap_numerical: integers wrap.  A strict cast is taken when it cannot
        fail (widening casts); otherwise it raises (see frame._check_strict)."""
        from .frame import Float64, DataType
        if dtype == "f64":
            dtype = Float64
        if not isinstance(dtype, DataType):
            raise N.InvalidOperationError(f"cast to {dtype!r} is not supported on the GPU executor")
        mode = "wrap" if wrap_numerical else ("strict" if strict else "non-strict")
        return Expr("cast", (self,), op=mode, value=dtype)

    def fill_null(self, value: Any = None, strategy: str | None = None, limit: Any = None) -> "Expr":
        """Expr.fill_null(value) (FunctionExpr::FillNull), or
        fill_null(strategy=..., limit=...) (FunctionExpr::FillNullWithStrategy):
        forward / backward carry the closest non-null row over at most `limit`
        nulls; min / max / mean / zero / one fill with the column's aggregate
        or the constant."""
        _fill_args(value, strategy, limit)
        if value is None and strategy is None:
            raise N.InvalidOperationError("fill_null needs a fill `value` or a `strategy`")
        if value is not None:
            return Expr("fill_null", (self, _to_expr(value)), op="fill_null")
        return _fill(self, strategy, limit)

    def forward_fill(self, limit: Any = None) -> "Expr":
        """Expr.forward_fill: fill_null(strategy="forward", limit=limit)."""
        return _fill(self, "forward", limit)

    def backward_fill(self, limit: Any = None) -> "Expr":
        """Expr.backward_fill: fill_null(strategy="backward", limit=limit)."""
        return _fill(self, "backward", limit)

    def is_in(self, other: Sequence[Any], *, nulls_equal: bool = False) -> "Expr":
        """Expr.is_in over a literal collection: x == v0 | x == v1 | ...
        (BooleanFunction::IsIn); a null x gives null unless nulls_equal."""
        vals = list(other)
        if builtins.len(vals) > 15:
            raise N.InvalidOperationError("is_in takes at most 15 literal values on the GPU executor")
        has_null = any(v is None for v in vals)
        vals = [v for v in vals if v is not None]
        if nulls_equal:
            out = self.is_null() if has_null else None
            for v in vals:
                t = self.eq_missing(v)
                out = t if out is None else (out | t)
            return out if out is not None else self.is_null() & lit(False)
        out = None
        for v in vals:
            t = self == v
            out = t if out is None else (out | t)
        return out if out is not None else self.ne(self)  # empty: null for null x, else false

    def is_between(self, lower_bound: Any, upper_bound: Any, closed: str = "both") -> "Expr":
        """Expr.is_between (BooleanFunction::IsBetween): both / left / right / none."""
        if closed not in ("both", "left", "right", "none"):
            raise N.InvalidOperationError(f"invalid closed={closed!r}")
        lo = self >= lower_bound if closed in ("both", "left") else self > lower_bound
        hi = self <= upper_bound if closed in ("both", "right") else self < upper_bound
        return lo & hi

    def alias(self, name: str) -> "Expr":
        return Expr("alias", (self,), value=name)

    # ----------------------------------------------------- aggregations
    def _agg(self, op: str, value: Any = None) -> "Expr":
        if _has_over(self):
            raise N.InvalidOperationError(
                f"{self!r}.{op}(): a window expression (over) inside an aggregation's input is not supported "
                "on the GPU executor")
        if _has_scan(self):
            raise N.InvalidOperationError(
                f"{self!r}.{op}(): a cumulative, lag, fill, ewm or rank function (cum_* / shift / diff / forward_fill / "
                "backward_fill / fill_null(strategy=...) / ewm_mean / rank) inside an aggregation's input is not supported "
                "on the GPU executor: it gives one value per row, in row order")
        return Expr("agg", (self,), op=op, value=value)

    def sum(self): return self._agg("sum")
    def mean(self): return self._agg("mean")
    def min(self): return self._agg("min")
    def max(self): return self._agg("max")
    def count(self): return self._agg("count")
    def len(self): return self._agg("len")
    def std(self, ddof: int = 1): return self._agg("std", int(ddof))
    def var(self, ddof: int = 1): return self._agg("var", int(ddof))
    def first(self): return self._agg("first")
    def last(self): return self._agg("last")

    def median(self) -> "Expr":
        """Expr.median: quantile(0.5, "linear") (polars-core/src/chunked_array/ops/aggregate/quantile.rs:168)."""
        return self._agg("median", (0.5, "linear"))

    def quantile(self, quantile: Any, interpolation: str = "nearest") -> "Expr":
        """Expr.quantile with a literal `quantile` in [0, 1]: nearest / higher /
        lower / midpoint / linear / equiprobable (quantile.rs:106
        generic_quantile).  Float32 stays Float32, every other numeric dtype
        gives Float64."""
        return self._agg("quantile", (_quantile_q(quantile), _quantile_method(interpolation)))

    # ------------------------------------------------- window / ordering
    def rolling_sum(self, window_size: int, weights=None, *, min_samples: int | None = None,
                    center: bool = False) -> "Expr":
        """Fixed-window sum (Expr.rolling_sum)."""
        return _rolling(self, "sum", window_size, weights, min_samples, center)

    def rolling_mean(self, window_size: int, weights=None, *, min_samples: int | None = None,
                     center: bool = False) -> "Expr":
        """Fixed-window mean (Expr.rolling_mean)."""
        return _rolling(self, "mean", window_size, weights, min_samples, center)

    def rolling_min(self, window_size: int, weights=None, *, min_samples: int | None = None,
                    center: bool = False) -> "Expr":
        """Fixed-window minimum (Expr.rolling_min; a NaN in the window propagates)."""
        return _rolling(self, "min", window_size, weights, min_samples, center)

    def rolling_max(self, window_size: int, weights=None, *, min_samples: int | None = None,
                    center: bool = False) -> "Expr":
        """Fixed-window maximum (Expr.rolling_max; a NaN in the window propagates)."""
        return _rolling(self, "max", window_size, weights, min_samples, center)

    def rolling_var(self, window_size: int, weights=None, *, min_samples: int | None = None,
                    center: bool = False, ddof: int = 1) -> "Expr":
        """Fixed-window variance (Expr.rolling_var; a non-finite value gives NaN)."""
        return _rolling(self, "var", window_size, weights, min_samples, center, ddof)

    def rolling_std(self, window_size: int, weights=None, *, min_samples: int | None = None,
                    center: bool = False, ddof: int = 1) -> "Expr":
        """Fixed-window standard deviation (Expr.rolling_std)."""
        return _rolling(self, "std", window_size, weights, min_samples, center, ddof)

    # ------------------------------------------------- cumulative / lag
    def cum_sum(self, *, reverse: bool = False) -> "Expr":
        """Running sum (Expr.cum_sum): Float64 sums are exact and rounded once."""
        return _cum(self, "sum", reverse)

    def cum_min(self, *, reverse: bool = False) -> "Expr":
        """Running minimum (Expr.cum_min; a NaN is skipped once a value has been seen)."""
        return _cum(self, "min", reverse)

    def cum_max(self, *, reverse: bool = False) -> "Expr":
        """Running maximum (Expr.cum_max)."""
        return _cum(self, "max", reverse)

    def cum_count(self, *, reverse: bool = False) -> "Expr":
        """Running count of non-null rows (Expr.cum_count), UInt32."""
        return _cum(self, "count", reverse)

    def cum_prod(self, *, reverse: bool = False) -> "Expr":
        raise N.InvalidOperationError(
            "cum_prod is not supported on the GPU executor (a running product has no exact fixed-point form)")

    def pct_change(self, n: Any = 1) -> "Expr":
        raise N.InvalidOperationError(
            "pct_change is not supported on the GPU executor (it needs forward_fill); "
            "`x / x.shift(n) - 1` covers the null-free case")

    def shift(self, n: Any = 1, *, fill_value: Any = None) -> "Expr":
        """Expr.shift with a literal `n` and an optional literal `fill_value`."""
        _lag_input(self, "shift")
        return Expr("lag", (self,), op="shift", value=(_lag_n(n, "shift"), _lag_fill(fill_value)))

    def diff(self, n: Any = 1, null_behavior: str = "ignore") -> "Expr":
        """Expr.diff: x - x.shift(n) (null_behavior "ignore")."""
        _lag_input(self, "diff")
        if null_behavior != "ignore":
            raise N.InvalidOperationError(
                f"diff(null_behavior={null_behavior!r}) is not supported on the GPU executor: dropping the leading "
                "nulls changes the length of the column")
        return Expr("lag", (self,), op="diff", value=(_lag_n(n, "diff"),))

    def ewm_mean(self, *, com: float | None = None, span: float | None = None, half_life: float | None = None,
                 alpha: float | None = None, adjust: bool = True, min_samples: int = 1,
                 ignore_nulls: bool = False) -> "Expr":
        """Exponentially weighted mean (Expr.ewm_mean; polars-compute/src/ewm/
        mean.rs:52): Float32 stays Float32, every other numeric dtype gives
        Float64."""
        a = _prepare_alpha(com, span, half_life, alpha)
        _lag_input(self, "ewm_mean")
        return Expr("ewm", (self,), op="mean", value=(a, bool(adjust), _ewm_min_samples(min_samples),
                                                      bool(ignore_nulls)))

    def rank(self, method: str = "average", *, descending: bool = False, seed: int | None = None) -> "Expr":
        """Expr.rank (polars-ops/src/series/ops/rank.rs:68): average / min /
        max / dense / ordinal; nulls stay null and are not counted.  UInt32,
        Float64 for "average"."""
        _rank_method(method)
        _lag_input(self, "rank")
        return Expr("rank", (self,), op=method, value=(bool(descending),))

    def ewm_std(self, *args: Any, **kwargs: Any) -> "Expr":
        raise N.InvalidOperationError(
            "ewm_std is not built on the GPU executor (only ewm_mean is; the variance carries a different state)")

    def ewm_var(self, *args: Any, **kwargs: Any) -> "Expr":
        raise N.InvalidOperationError(
            "ewm_var is not built on the GPU executor (only ewm_mean is; the variance carries a different state)")

    def ewm_mean_by(self, *args: Any, **kwargs: Any) -> "Expr":
        raise N.InvalidOperationError(
            "ewm_mean_by is not built on the GPU executor (only ewm_mean is; time-based decay carries a "
            "different state)")

    def over(self, partition_by: Any, *more_exprs: Any, order_by: Any = None,
             mapping_strategy: str = "group_to_rows") -> "Expr":
        """Expr.over: evaluate this expression on every group of the partition
        keys, each result back at its row (polars-expr/src/expressions/
        window.rs:356 WindowExpr::evaluate with WindowMapping::GroupsToRows).
        Takes `<elementwise>.rolling_*(...)`, the aggregations sum / mean /
        min / max / count / len / first / last / std / var / median / quantile of an elementwise
        expression (or pl.len()), and `<elementwise>.cum_*()` / `.shift(...)` /
        `.diff(...)` / `.forward_fill(...)` / `.backward_fill(...)` /
        `.fill_null(strategy=...)` / `.ewm_mean(...)` / `.rank(...)`, over
        plain key columns."""
        keys: list[str] = []
        items = [partition_by, *more_exprs]
        while items:
            it = items.pop(0)
            if isinstance(it, (list, tuple)):
                items = list(it) + items
            elif isinstance(it, str):
                keys.append(it)
            elif isinstance(it, Expr) and it.kind == "col":
                keys.append(it.value)
            elif isinstance(it, Expr):
                raise N.InvalidOperationError(
                    f"over({it!r}): computed partition keys are not supported on the GPU executor "
                    "(partition by plain columns)")
            else:
                raise N.InvalidOperationError(f"cannot interpret {it!r} as a partition key")
        if not keys or builtins.len(keys) > N.MAX_KEYS:
            raise N.InvalidOperationError("over() partitions by 1..8 plain key columns")
        if builtins.len(set(keys)) != builtins.len(keys):
            raise N.DuplicateError("over(): partition keys must be distinct columns")
        if order_by is not None:
            raise N.InvalidOperationError("over(order_by=...) is not supported on the GPU executor")
        if mapping_strategy != "group_to_rows":
            raise N.InvalidOperationError(
                f"over(mapping_strategy={mapping_strategy!r}) is not supported on the GPU executor "
                "(only 'group_to_rows')")
        f = self
        while f.kind == "alias":
            f = f.args[0]
        if f.kind == "rolling" or f.kind in _SCAN_KINDS:
            ok = _is_elementwise(f.args[0])
        elif f.kind == "agg":
            ok = f.op in _OVER_AGGS and _is_elementwise(f.args[0])
        else:
            ok = f.kind == "len"
        if not ok:
            raise N.InvalidOperationError(
                f"{self!r}.over(...): the GPU executor evaluates over groups only rolling_* functions and the "
                f"aggregations {', '.join(_OVER_AGGS)} (or len()) of an elementwise expression, "
                "and cum_sum / cum_min / cum_max / cum_count / shift / diff / forward_fill / backward_fill / "
                "fill_null(strategy=...) / ewm_mean / rank of an elementwise expression")
        if f.kind == "rank" and builtins.len(keys) >= N.MAX_KEYS:
            raise N.InvalidOperationError(
                f"{self!r}.over(...): rank over {builtins.len(keys)} partition keys is not supported on the GPU "
                f"executor: the sort takes {N.MAX_KEYS} columns and the ranked value is one of them, so rank "
                f"partitions by at most {N.MAX_KEYS - 1} keys")
        return Expr("over", (self,), op="over", value=tuple(keys))

    def sort(self, *, descending: bool = False, nulls_last: bool = False) -> "Expr":
        return Expr("sort", (self,), op="sort", value=(bool(descending), bool(nulls_last)))

    def arg_sort(self, *, descending: bool = False, nulls_last: bool = False) -> "Expr":
        return Expr("sort", (self,), op="arg_sort", value=(bool(descending), bool(nulls_last)))


def _rolling(e: Expr, kind: str, window_size: int, weights, min_samples, center, ddof: int = 0) -> Expr:
    if weights is not None:
        raise N.InvalidOperationError("weighted rolling windows are not supported on the GPU executor")
    if not isinstance(window_size, int) or window_size < 1:
        raise N.InvalidOperationError("`window_size` must be a positive integer")
    ms = window_size if min_samples is None else int(min_samples)
    if ms > window_size:
        raise N.InvalidOperationError("`min_samples` should be <= `window_size`")
    if not 0 <= int(ddof) <= 255:
        raise N.InvalidOperationError("`ddof` must be in 0..255")
    return Expr("rolling", (e,), op=kind, value=(window_size, ms, bool(center), int(ddof)))


def _is_rowwise(e: Expr) -> bool:
    """Elementwise expressions and rolling / cumulative / lag / fill / ewm / rank functions of
    them: one value per row, in row order."""
    if e.kind == "over":
        return True
    return e.kind in _ELEMENTWISE + ("rolling",) + _SCAN_KINDS and builtins.all(_is_rowwise(a) for a in e.args)


def _lag_input(e: Expr, what: str) -> None:
    if not _is_rowwise(e):
        raise N.InvalidOperationError(
            f"{e!r}.{what}(...): the input must be an elementwise expression (not an aggregation or a sort)")


def _cum(e: Expr, kind: str, reverse) -> Expr:
    if reverse:
        raise N.InvalidOperationError(f"cum_{kind}(reverse=True) is not supported on the GPU executor")
    _lag_input(e, f"cum_{kind}")
    return Expr("cum", (e,), op=kind, value=(False,))


def _lag_n(n: Any, what: str):
    """A literal `n`: any integer type (operator.index), or for shift a
    literal null, which shifts every row out (an all-null column)."""
    import operator

    if isinstance(n, Expr) and n.kind == "lit":
        n = n.value
    if n is None:
        if what != "shift":
            raise N.InvalidOperationError(f"{what}(n=None): `n` must be an integer")
        return None
    if isinstance(n, Expr):
        raise N.InvalidOperationError(
            f"{what}(n={n!r}): a computed `n` is not supported on the GPU executor (pass an integer)")
    try:
        if isinstance(n, bool):
            raise TypeError
        return operator.index(n)
    except TypeError:
        raise N.InvalidOperationError(f"{what}(n={n!r}): `n` must be an integer") from None


def _lag_fill(v: Any):
    if isinstance(v, Expr):
        if v.kind != "lit":
            raise N.InvalidOperationError(
                f"shift(fill_value={v!r}): a computed `fill_value` is not supported on the GPU executor "
                "(pass a scalar or lit)")
        v = v.value
    return v


_FILL_STRATEGIES = ("forward", "backward", "min", "max", "mean", "zero", "one")


def _fill_args(value: Any, strategy: Any, limit: Any) -> None:
    """The argument checks of py-polars' Expr.fill_null (expr.py:2916-2924)."""
    if value is not None and strategy is not None:
        raise ValueError("cannot specify both `value` and `strategy`")
    if strategy not in ("forward", "backward") and limit is not None:
        raise ValueError("can only specify `limit` when strategy is set to 'backward' or 'forward'")
    if strategy is not None and strategy not in _FILL_STRATEGIES:
        raise ValueError(f"invalid fill_null strategy {strategy!r}: expected one of {', '.join(_FILL_STRATEGIES)}")


def _fill_limit(limit: Any):
    """A literal `limit`: None or a non-negative integer (the reference's
    limit is an unsigned IdxSize)."""
    import operator

    if isinstance(limit, Expr) and limit.kind == "lit":
        limit = limit.value
    if limit is None:
        return None
    if isinstance(limit, Expr):
        raise N.InvalidOperationError(
            f"fill limit={limit!r}: a computed `limit` is not supported on the GPU executor (pass an integer)")
    try:
        if isinstance(limit, bool):
            raise TypeError
        limit = operator.index(limit)
    except TypeError:
        raise N.InvalidOperationError(f"fill limit={limit!r}: `limit` must be a non-negative integer") from None
    if limit < 0:
        raise N.InvalidOperationError(f"fill limit={limit}: `limit` must be a non-negative integer (it is unsigned)")
    return limit


def _fill(e: Expr, strategy: str, limit: Any) -> Expr:
    _fill_args(None, strategy, limit)
    _lag_input(e, "fill_null" if strategy not in ("forward", "backward") else f"{strategy}_fill")
    return Expr("fill", (e,), op=strategy, value=(_fill_limit(limit),))


def _has_scan(e: Expr) -> bool:
    return e.kind in _SCAN_KINDS or builtins.any(_has_scan(a) for a in e.args)


def _prepare_alpha(com: Any = None, span: Any = None, half_life: Any = None, alpha: Any = None) -> float:
    """The decay of an ewm_* function as its smoothing factor alpha, with the
    checks and messages of py-polars' _prepare_alpha (expr.py:11710)."""
    import math

    given = [v for v in (com, span, half_life, alpha) if v is not None]
    if builtins.len(given) > 1:
        raise ValueError("parameters `com`, `span`, `half_life`, and `alpha` are mutually exclusive")
    if not given:
        raise ValueError("one of `com`, `span`, `half_life`, or `alpha` must be set")
    if com is not None:
        if not com >= 0.0:
            raise ValueError(f"require `com` >= 0 (found {com!r})")
        return 1.0 / (1.0 + com)
    if span is not None:
        if not span >= 1.0:
            raise ValueError(f"require `span` >= 1 (found {span!r})")
        return 2.0 / (span + 1.0)
    if half_life is not None:
        if not half_life > 0.0:
            raise ValueError(f"require `half_life` > 0 (found {half_life!r})")
        return 1.0 - math.exp(-math.log(2.0) / half_life)
    if not 0 < alpha <= 1:
        raise ValueError(f"require 0 < `alpha` <= 1 (found {alpha!r})")
    return float(alpha)


_QUANTILE_METHODS = ("nearest", "higher", "lower", "midpoint", "linear", "equiprobable")


def _quantile_method(method: Any) -> str:
    if not isinstance(method, builtins.str) or method not in _QUANTILE_METHODS:
        raise ValueError(f"quantile: `interpolation` must be one of {', '.join(map(repr, _QUANTILE_METHODS))}, "
                         f"got {method!r}")
    return method


def _quantile_q(q: Any) -> float:
    """A literal `quantile`: a Python or NumPy real number in [0, 1]."""
    import numbers

    if isinstance(q, Expr) and q.kind == "lit":
        q = q.value
    if isinstance(q, Expr):
        raise N.InvalidOperationError(
            f"quantile({q!r}): a computed `quantile` is not supported on the GPU executor (pass a number)")
    if isinstance(q, bool) or not isinstance(q, numbers.Real):
        raise N.InvalidOperationError(f"quantile({q!r}): `quantile` must be a real number")
    q = float(q)
    if not 0.0 <= q <= 1.0:  # NaN fails both comparisons
        raise N.ComputeError("`quantile` should be between 0.0 and 1.0")
    return q


_RANK_METHODS = ("average", "min", "max", "dense", "ordinal")


def _rank_method(method: Any) -> str:
    """The tie method of rank: "random" is refused by name (it would need the
    reference's RNG stream), anything else unknown is a ValueError."""
    if method == "random":
        raise N.InvalidOperationError(
            "rank(method='random') is not supported on the GPU executor: its tie order comes from the "
            "reference's random number stream (with or without `seed`)")
    if method not in _RANK_METHODS:
        raise ValueError(f"rank: `method` must be one of {', '.join(map(repr, _RANK_METHODS))} (or 'random'), "
                         f"got {method!r}")
    return method


def _ewm_min_samples(v: Any) -> int:
    import operator

    try:
        if isinstance(v, bool):
            raise TypeError
        v = operator.index(v)
    except TypeError:
        raise N.InvalidOperationError(f"ewm_mean(min_samples={v!r}): `min_samples` must be an integer") from None
    if v < 0:
        raise N.InvalidOperationError(f"ewm_mean(min_samples={v}): `min_samples` must be a non-negative integer")
    return v


_OVER_AGGS = ("sum", "mean", "min", "max", "count", "len", "first", "last", "std", "var", "median", "quantile")
# the segmented scans (frame._window_fn; csrc/seg_scan.hpp); rank follows their rules everywhere
_SCAN_KINDS = ("cum", "lag", "fill", "ewm", "rank")
_ELEMENTWISE = ("col", "lit", "bin", "un", "alias", "ternary", "cast", "fill_null", "strfn", "over")


def _has_over(e: Expr) -> bool:
    return e.kind == "over" or builtins.any(_has_over(a) for a in e.args)


def _is_elementwise(e: Expr) -> bool:
    """Row-by-row expressions (an over node counts: it yields one value per row)."""
    if e.kind == "over":
        return True
    return e.kind in _ELEMENTWISE and builtins.all(_is_elementwise(a) for a in e.args)


def _to_expr(v: Any) -> Expr:
    return v if isinstance(v, Expr) else lit(v)


class _Then:
    def __init__(self, branches: list):
        self._branches = branches

    def when(self, cond: Any) -> "_When":
        return _When(self._branches, _to_expr(cond))

    def otherwise(self, value: Any) -> Expr:
        out = _to_expr(value)
        for cond, val in reversed(self._branches):
            out = Expr("ternary", (cond, val, out), op="if_else")
        return out

    # a chain used without otherwise() ends in null, as in polars
    def _finish(self) -> Expr:
        return self.otherwise(None)

    def __getattr__(self, name: str):
        # pl.when(c).then(x).sum() / .alias(...): the chain as an expression
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._finish(), name)


class _When:
    def __init__(self, branches: list, cond: Expr):
        self._branches, self._cond = branches, cond

    def then(self, value: Any) -> _Then:
        return _Then(self._branches + [(self._cond, _to_expr(value))])


def when(condition: Any) -> _When:
    """pl.when(cond).then(a)[.when(c2).then(b)].otherwise(c) -> a ternary
    expression (if_then_else; a null condition takes the otherwise branch)."""
    return _When([], _to_expr(condition))


def col(name: str) -> Expr:
    return Expr("col", value=name)


def lit(value: Any) -> Expr:
    if isinstance(value, Expr):
        return value
    return Expr("lit", value=value)


def len() -> Expr:  # noqa: A001 - mirrors pl.len()
    return Expr("len")


def sum(name: str) -> Expr:  # noqa: A001
    return col(name).sum()


def mean(name: str) -> Expr:
    return col(name).mean()


def min(name: str) -> Expr:  # noqa: A001
    return col(name).min()


def max(name: str) -> Expr:  # noqa: A001
    return col(name).max()


def count(name: str) -> Expr:
    return col(name).count()


def first(name: str) -> Expr:
    return col(name).first()


def last(name: str) -> Expr:
    return col(name).last()


def median(name: str) -> Expr:
    return col(name).median()


def quantile(name: str, quantile: Any, interpolation: str = "nearest") -> Expr:
    return col(name).quantile(quantile, interpolation)


class _StrNamespace:
    """Expr.str: starts_with / ends_with / contains(literal=True), evaluated
    on the GPU as Boolean columns (frame._lower_strings)."""

    def __init__(self, e: Expr):
        self._e = e

    def _fn(self, op: str, pattern) -> Expr:
        if not isinstance(pattern, str):
            raise N.InvalidOperationError(f"str.{op} takes a string literal on the GPU executor")
        return Expr("strfn", (self._e,), op=op, value=pattern)

    def starts_with(self, prefix: str) -> Expr:
        return self._fn("starts_with", prefix)

    def ends_with(self, suffix: str) -> Expr:
        return self._fn("ends_with", suffix)

    def contains(self, pattern: str, *, literal: bool = False, strict: bool = True) -> Expr:
        if not literal and any(ch in pattern for ch in ".^$*+?()[]{}|\\"):
            raise N.InvalidOperationError("regex patterns are not supported on the GPU executor (use literal=True)")
        return self._fn("contains", pattern)


_BIN_OPS = {
    "+": "ADD", "-": "SUB", "*": "MUL", "/": "TRUEDIV", "//": "FLOORDIV", "%": "MOD", "div": "DIVIDE",
    "^": "XOR", "fill_null": "FILL_NULL",
    ">": "GT", ">=": "GE", "<": "LT", "<=": "LE", "==": "EQ", "!=": "NE",
    "eq_missing": "EQ_MISSING", "ne_missing": "NE_MISSING", "&": "AND", "|": "OR",
}
_UN_OPS = {
    "neg": "NEG", "abs": "ABS", "not": "NOT", "is_null": "IS_NULL",
    "is_not_null": "IS_NOT_NULL", "is_nan": "IS_NAN", "is_finite": "IS_FINITE",
    "cast_f64": "CAST_F64",
}


def lower(expr: Expr, col_index: dict[str, int], schema: dict[str, int]) -> list[tuple[int, int, Any]]:
    """Lower an (aggregation-free) Expr to a postfix program.

    Returns a list of (opcode, arg, imm) triples; `imm` is a float for
    LIT_F64 and an int otherwise.
    """
    out: list[tuple[int, int, Any]] = []

    def emit(e: Expr) -> None:
        k = e.kind
        if k == "alias":
            emit(e.args[0])
        elif k == "col":
            if e.value not in col_index:
                raise N.ComputeError(f'unable to find column "{e.value}"')
            out.append((N.OP["COL"], col_index[e.value], 0))
        elif k == "lit":
            v = e.value
            if v is None:
                out.append((N.OP["LIT_NULL"], 0, 0))  # untyped: takes the other operand's type
            elif isinstance(v, bool):
                out.append((N.OP["LIT_BOOL"], 0, int(v)))
            elif isinstance(v, int):
                if not -(2 ** 63) <= v < 2 ** 63:
                    raise N.InvalidOperationError(f"integer literal {v} does not fit Int64")
                out.append((N.OP["LIT_I64"], 0, v))
            elif isinstance(v, float):
                out.append((N.OP["LIT_F64"], 0, float(v)))
            else:
                raise N.InvalidOperationError(f"literal of type {type(v).__name__} is not supported")
        elif k in ("bin", "fill_null"):
            emit(e.args[0])
            emit(e.args[1])
            out.append((N.OP[_BIN_OPS[e.op]], 0, 0))
        elif k == "ternary":
            for a in e.args:
                emit(a)
            out.append((N.OP["IF_ELSE"], 0, 0))
        elif k == "cast":
            emit(e.args[0])
            out.append((N.OP["CAST"], e.value.code, 1 if e.op == "wrap" else 0))
        elif k == "un":
            emit(e.args[0])
            out.append((N.OP[_UN_OPS[e.op]], 0, 0))
        elif k in ("agg", "len"):
            raise N.InvalidOperationError(f"aggregation {e!r} is not allowed in this context")
        else:
            raise N.InvalidOperationError(f"unsupported expression {e!r}")

    emit(expr)
    if not out:
        raise N.InvalidOperationError("empty expression")
    return out


def to_instr_array(prog: list[tuple[int, int, Any]]):
    arr = (N.Instr * builtins.len(prog))()
    for i, (op, arg, imm) in enumerate(prog):
        arr[i].op = op
        arr[i].arg = arg
        if op == N.OP["LIT_F64"]:
            arr[i].imm.f64 = float(imm)
        else:
            arr[i].imm.i64 = int(imm)
    return arr
