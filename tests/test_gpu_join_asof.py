"""GPU: join_asof against the restatements of tests/asof_ref.py.  Every
comparison is exact -- the matched row and its validity for every left row, and
through the frame every gathered cell -- because nothing here rounds.  Expected
values come from asof_ref_bounds, and from asof_ref_scan as well where the case
is small and its left keys ascend (what the scan's running state needs).

Shapes come from the kernels' geometry (N.ASOF_TILE_ROWS left rows per
workgroup, N.ASOF_LDS_VALUES right values staged at most); every shape runs
with option asof_path 0, 1 and 2 and the three agree bit for bit.  The NaN
cases pin this project's TotalOrd rule (NaN greatest and equal to itself), not
the reference's partial_cmp, whose scan stalls at a NaN."""

import ctypes as C
import datetime as dt
import warnings

import numpy as np
import pytest

import polaroid_amd as pl
from asof_ref import asof_ref_bounds, asof_ref_scan
from conftest import load_golden
from polaroid_amd import _native as N
from test_gpu_sliced_inputs import _place, _spec

pytestmark = pytest.mark.gpu

T, L = N.ASOF_TILE_ROWS, N.ASOF_LDS_VALUES
STRATEGIES = ("backward", "forward", "nearest")
SCAN_ROWS = 4000


# ------------------------------------------------------------------ helpers
def c_call(left, right, strategy, allow_eq=True, tol=None, lo=None, hi=None, rows=None):
    """plgpu_join_asof on device Series -> (rows, ok, path)."""
    out, path = N.Column(), C.c_int32(0)
    bits, tf = 0, 0.0
    if tol is not None:
        if left._col.dtype in (N.F32, N.F64):
            tf = float(tol)
        else:
            bits = int(tol) - (1 << 64) if int(tol) >= 1 << 63 else int(tol)
    ref = lambda s: None if s is None else C.byref(s._col)  # noqa: E731
    N.check(N.lib().plgpu_join_asof(ref(left), ref(right), ref(lo), ref(hi), ref(rows), N.ASOF[strategy],
                                    int(allow_eq), int(tol is not None), bits, tf, C.byref(out), C.byref(path), None))
    s = pl.Series._from_native("idx", out)
    assert s.len() == left.len() and s._col.dtype == N.U32
    ok = s.validity_numpy()
    return np.where(ok, s.to_numpy().astype(np.int64), -1), ok, N.ASOF_PATH[path.value]


def expect(left, lv, right, rv, strategy, allow_eq=True, tol=None, sorted_left=True, **by):
    rows, ok = asof_ref_bounds(left, lv, right, rv, strategy, allow_eq, tol, **by)
    if sorted_left and len(left) + len(right) <= SCAN_ROWS:
        r2, o2 = asof_ref_scan(left, lv, right, rv, strategy, allow_eq, tol, **by)
        assert o2.tolist() == ok.tolist() and r2.tolist() == rows.tolist(), "the two readings disagree"
    return rows, ok


def check_paths(plgpu_option, left, lv, right, rv, strategy, allow_eq=True, tol=None, sorted_left=True,
                layout="fresh", tag=None):
    """The C entry point under asof_path 0 / 1 / 2 against the reference."""
    exp_rows, exp_ok = expect(left, lv, right, rv, strategy, allow_eq, tol, sorted_left)
    ls = _place("l", left, lv, *_spec(layout, 0))
    rs = _place("r", right, rv, *_spec(layout, 1))
    for path in (0, 1, 2):
        plgpu_option("asof_path", path)
        rows, ok, took = c_call(ls, rs, strategy, allow_eq, tol)
        what = (tag, strategy, allow_eq, tol, path, layout)
        assert took == ("global" if path == 2 else "staged"), what
        assert ok.tolist() == exp_ok.tolist(), what
        assert rows.tolist() == exp_rows.tolist(), what


def sorted_keys(rng, n, span, dtype=np.int64, lo=0):
    return np.sort(rng.integers(lo, lo + max(span, 1), n)).astype(dtype)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n_left", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_shapes(gpu, plgpu_option, n_left):
    rng = np.random.default_rng(100 + n_left)
    for n_right in (0, 1, 2, 65, L - 1, L, L + 1, 4 * L + 3):
        span = max(2, n_right // 2)  # duplicates on both sides
        left = sorted_keys(rng, n_left, span + 20, lo=-10)
        right = sorted_keys(rng, n_right, span)
        for strategy in STRATEGIES:
            for allow_eq in (True, False):
                check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tag=(n_left, n_right))
        check_paths(plgpu_option, left, None, right, None, "nearest", True, tol=1, tag=(n_left, n_right))


@pytest.mark.parametrize("window", ["one_below", "one_above", "L_minus_1", "exactly_L", "L_plus_1", "whole"])
def test_window_sizes_of_one_tile(gpu, plgpu_option, window):
    """Right keys 0, 1, 2, ...: the tile's window holds the keys in [min, max]
    of the left keys plus one on either side (nearest: two above), so backward
    and forward stage exactly L values at "exactly_L" and nearest at
    "L_minus_1"; one more falls to the search in place."""
    rng = np.random.default_rng(7)
    right = np.arange(3 * L, dtype=np.int64)
    lo, hi = {"one_below": (3 * L + 5, 3 * L + 50), "one_above": (-50, -5), "L_minus_1": (L, 2 * L - 4), "exactly_L": (L, 2 * L - 3),
              "L_plus_1": (L, 2 * L - 2), "whole": (-5, 3 * L + 5)}[window]
    left = np.sort(np.concatenate([[lo, hi], rng.integers(lo, hi + 1, T - 2)])).astype(np.int64)
    for strategy in STRATEGIES:
        for allow_eq in (True, False):
            check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tag=window)
    check_paths(plgpu_option, left, None, right, None, "nearest", True, tol=0, tag=window)


def test_long_run_of_equal_right_keys_across_a_window_end(gpu, plgpu_option):
    """A run of L + 50 equal right keys: backward's last equal and forward's
    first equal lie L + 49 apart, and nearest's upper candidate is the run's
    last row, beyond the window of a tile whose keys lie below the run."""
    run = L + 50
    right = np.concatenate([np.arange(100), np.full(run, 500), np.arange(600, 700)]).astype(np.int64)
    below = np.sort(np.random.default_rng(3).integers(400, 500, T))
    left = np.concatenate([below, np.full(T, 500), np.arange(501, 501 + T) // 8 + 440]).astype(np.int64)
    left = np.sort(left)
    for strategy in STRATEGIES:
        for allow_eq in (True, False):
            check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tag="run")
    rows, ok = asof_ref_bounds(below.astype(np.int64), None, right, None, "nearest")
    assert ok.all() and set(rows[below > 300].tolist()) == {100 + run - 1}  # the yardstick takes the run's last row


def test_run_of_equal_left_keys_across_a_tile_seam(gpu, plgpu_option):
    left = np.sort(np.concatenate([np.arange(T - 10), np.full(25, T + 3), np.arange(2 * T, 3 * T - 15)])).astype(np.int64)
    right = np.arange(0, 3 * T, 3, dtype=np.int64)
    assert left[T - 1] == left[T] == T + 3
    for strategy in STRATEGIES:
        for allow_eq in (True, False):
            check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tag="seam")


# ------------------------------------------------------------------ parameters
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("allow_eq", [True, False])
def test_tolerances(gpu, plgpu_option, strategy, allow_eq):
    rng = np.random.default_rng(11)
    left, right = sorted_keys(rng, T + 77, 600, lo=-30), sorted_keys(rng, 300, 500)
    for tol in (None, 0, 3, -3):
        check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tol, tag="tol")
    fl, fr = (left / 4).astype(np.float64), (right / 4).astype(np.float64)
    for tol in (None, 0.0, 0.5, -0.5):
        check_paths(plgpu_option, fl, None, fr, None, strategy, allow_eq, tol, tag="ftol")


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_integer_extremes(gpu, plgpu_option, strategy):
    i = np.iinfo(np.int64)
    left = np.array([i.min, i.min + 1, -2, 0, 1608129000134000125, i.max - 1, i.max], np.int64)
    right = np.array([i.min, -1, 1608129000134000124, 1608129000134000126, i.max], np.int64)
    for allow_eq in (True, False):
        for tol in (None, 1, i.max, i.min):
            check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tol, tag="i64")
    u = np.array([0, 5, 2**63 - 1, 2**63, 2**63 + 5, 2**64 - 1], np.uint64)
    ur = np.array([1, 2**63 - 2, 2**63 + 4, 2**63 + 4, 2**64 - 2], np.uint64)
    for allow_eq in (True, False):
        for tol in (None, 3, 2**64 - 1):
            check_paths(plgpu_option, u, None, ur, None, strategy, allow_eq, tol, tag="u64")
    for dtype in (np.int32, np.uint32):
        ii = np.iinfo(dtype)
        l32 = np.array([ii.min, ii.min + 1, 7, ii.max], dtype)
        r32 = np.array([ii.min, 6, 8, ii.max - 1, ii.max], dtype)
        for tol in (None, 1, ii.max if dtype is np.uint32 else ii.min):
            check_paths(plgpu_option, l32, None, r32, None, strategy, True, tol, tag=dtype.__name__)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_floats_total_order(gpu, plgpu_option, dtype, strategy):
    """-0.0 equals 0.0; NaN is the greatest value and equals itself (this
    project's TotalOrd rule; the reference's partial_cmp stalls at a NaN)."""
    nan, inf = np.nan, np.inf
    left = np.array([-inf, -1.5, -0.0, 0.0, 0.3, 1.0, 1.5, 2.0, inf, nan, nan], dtype)   # 1.5: a nearest tie
    right = np.array([-inf, -2.0, 0.0, -0.0, 1.0, 2.0, 2.0, inf, nan, nan], dtype)
    for allow_eq in (True, False):
        for tol in (None, 0.0, 0.5, -inf):
            check_paths(plgpu_option, left, None, right, None, strategy, allow_eq, tol, tag="float")
    check_paths(plgpu_option, left[:-2], None, right[:-2], None, strategy, True, tag="no NaN")
    check_paths(plgpu_option, left, None, right[:-2], None, strategy, True, tag="NaN left")
    check_paths(plgpu_option, left[:-2], None, right, None, strategy, False, tag="NaN right")
    if dtype is np.float32:  # |l - r| is rounded in Float32: 1e8 + 0.1 is 1e8 there, and passes a tolerance of 1e8
        l32, r32 = np.array([1e8], dtype), np.array([-0.1], dtype)
        assert asof_ref_bounds(l32, None, r32, None, "backward", tolerance=1e8)[1].tolist() == [True]
        assert asof_ref_bounds(l32.astype(np.float64), None, r32.astype(np.float64), None, "backward",
                               tolerance=1e8)[1].tolist() == [False]
        check_paths(plgpu_option, l32, None, r32, None, strategy, True, tol=1e8, tag="f32 rounding")


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_nulls_at_the_front(gpu, plgpu_option, strategy):
    rng = np.random.default_rng(5)
    left, right = sorted_keys(rng, T + 130, 900, lo=-20), sorted_keys(rng, L + 300, 800)
    lv, rv = np.ones(len(left), bool), np.ones(len(right), bool)
    lv[:70], rv[:131] = False, False
    left[:70], right[:131] = 10**9, -10**9  # what a null slot holds is not a key
    for lvv, rvv in ((lv, None), (None, rv), (lv, rv)):
        for allow_eq in (True, False):
            check_paths(plgpu_option, left, lvv, right, rvv, strategy, allow_eq, tag="nulls")
    none_l, none_r = np.zeros(len(left), bool), np.zeros(len(right), bool)
    check_paths(plgpu_option, left, none_l, right, rv, strategy, tag="all-null left")
    check_paths(plgpu_option, left, lv, right, none_r, strategy, tag="all-null right")


@pytest.mark.parametrize("layout", ["off1", "off3", "off63", "off65", "ptr8", "bitmap_b1", "bitmap_b3_off2"])
def test_sliced_and_misaligned_inputs(gpu, plgpu_option, layout):
    rng = np.random.default_rng(17)
    for dtype in (np.int64, np.float32):
        left, right = sorted_keys(rng, T + 9, 700, dtype), sorted_keys(rng, 2 * L + 7, 900, dtype)
        lv, rv = np.ones(len(left), bool), np.ones(len(right), bool)
        lv[:5], rv[:67] = False, False
        for strategy in STRATEGIES:
            check_paths(plgpu_option, left, lv, right, rv, strategy, True, tol=2, layout=layout, tag=dtype.__name__)
            check_paths(plgpu_option, left, None, right[:L - 5], None, strategy, False, layout=layout, tag="staged")


def test_is_sorted_asc(gpu):
    def flags(v, valid=None, layout="fresh"):
        a, f = C.c_int32(9), C.c_int32(9)
        s = _place("x", v, valid, *_spec(layout, 0))
        N.check(N.lib().plgpu_is_sorted_asc(C.byref(s._col), C.byref(a), C.byref(f), None))
        return a.value, f.value

    n = 3 * T + 7
    up = np.arange(n, dtype=np.int64) // 3
    assert flags(up) == (1, 1)
    for at in (1, T - 1, T, n - 1):  # a descent inside a tile, across a seam, at the end
        bad = up.copy()
        bad[at] = bad[at - 1] - 1
        assert flags(bad) == (0, 1), at
    valid = np.ones(n, bool)
    valid[:T + 5] = False
    junk = up.copy()
    junk[:T + 5] = 10**12  # null slots are not compared
    assert flags(junk, valid) == (1, 1) and flags(junk, valid, "off63") == (1, 1)
    for at in (T + 5 + 1, n - 1):
        late = valid.copy()
        late[at] = False
        assert flags(junk, late) == (1, 0), at
    f = np.array([-np.inf, -0.0, 0.0, -0.0, 1.0, np.inf, np.nan, np.nan], np.float32)
    assert flags(f) == (1, 1) and flags(f[::-1].copy()) == (0, 1)
    assert flags(np.array([np.nan, 1.0])) == (0, 1)
    assert flags(np.array([2**63, 2**63 - 1], np.uint64)) == (0, 1)


# ------------------------------------------------------------------ the C entry point alone
def test_ranges_are_clamped(gpu):
    rng = np.random.default_rng(23)
    n, nr = T + 3, 500
    left, right = sorted_keys(rng, n, 600), sorted_keys(rng, nr, 600)
    lo = rng.integers(0, nr + 1, n).astype(np.uint32)
    hi = rng.integers(0, nr + 1, n).astype(np.uint32)       # half of them reversed
    hi[::7] = 2**32 - 1                                     # far out of bounds
    lo[::11] = 2**31
    exp = {}
    for strategy in STRATEGIES:
        exp_rows, exp_ok = np.full(n, -1, np.int64), np.zeros(n, bool)
        for i in range(n):
            a = min(int(lo[i]), nr)
            b = max(a, min(int(hi[i]), nr))
            r, o = asof_ref_bounds(left[i:i + 1], None, right[a:b], None, strategy)
            if o[0]:
                exp_rows[i], exp_ok[i] = a + r[0], True
        exp[strategy] = (exp_rows, exp_ok)
    for layout in ("fresh", "off1", "off3", "off63", "off65"):
        ls, rs = _place("l", left, None, *_spec(layout, 0)), _place("r", right, None, *_spec(layout, 1))
        los, his = _place("lo", lo, None, *_spec(layout, 2)), _place("hi", hi, None, *_spec(layout, 3))
        for strategy in STRATEGIES:
            rows, ok, took = c_call(ls, rs, strategy, lo=los, hi=his)
            assert took == "ranged"
            exp_rows, exp_ok = exp[strategy]
            assert ok.tolist() == exp_ok.tolist() and rows.tolist() == exp_rows.tolist(), (layout, strategy)
            assert ((rows >= 0) & (rows < nr))[ok].all()


def test_right_rows_map_positions(gpu):
    left = np.array([5, 15, 25], np.int64)
    right = np.array([0, 10, 20], np.int64)
    perm = np.array([7, 3, 9], np.uint32)
    rows, ok, _ = c_call(pl.Series.from_numpy("l", left), pl.Series.from_numpy("r", right), "backward",
                         rows=pl.Series.from_numpy("p", perm))
    assert ok.all() and rows.tolist() == [7, 3, 9]


# ------------------------------------------------------------------ the frame layer
def frame_rows(out, name="rid"):
    """The right row every output row took, read off a row-id payload column."""
    s = out[name]
    ok = s.validity_numpy()
    return np.where(ok, s.to_numpy().astype(np.int64), -1), ok


@pytest.mark.parametrize("case", load_golden("asof_cases.json")["cases"], ids=lambda c: c["name"])
def test_reference_cases_through_the_frame(gpu, case):
    np_t = np.dtype(case["dtype"])
    pl_t = {"int32": pl.Int32, "int64": pl.Int64, "uint64": pl.UInt64, "float32": pl.Float32, "float64": pl.Float64}[
        case["dtype"]]
    for by_t in case.get("by_dtypes", [None]):
        lcols = {"t": pl.Series("t", case["left"], pl_t)}
        rcols = {"t": pl.Series("t", case["right"], pl_t),
                 "rid": pl.Series.from_numpy("rid", np.arange(len(case["right"]), dtype=np.int64))}
        by = None
        if "by_left" in case:
            by = [f"k{j}" for j in range(len(case["by_left"]))]
            for j, (bl, br) in enumerate(zip(case["by_left"], case["by_right"])):
                kt = getattr(pl, by_t.capitalize().replace("Ui", "UI")) if by_t else None
                lcols[by[j]], rcols[by[j]] = pl.Series(by[j], bl, kt), pl.Series(by[j], br, kt)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            out = pl.DataFrame(lcols).join_asof(pl.DataFrame(rcols), on="t", by=by, strategy=case["strategy"],
                                                tolerance=case.get("tolerance"), coalesce=False,
                                                allow_exact_matches=case.get("allow_eq", True))
        rows, ok = frame_rows(out)
        if "expected_rows" in case:
            assert [int(r) if k else None for r, k in zip(rows, ok)] == case["expected_rows"], (case["name"], by_t)
        else:
            right = np.array(case["right"], np_t)
            assert [right[r].item() if k else None for r, k in zip(rows, ok)] == case["expected_values"], case["name"]
            assert out["t_right"].to_list() == case["expected_values"]


def test_frame_output_columns(gpu):
    left = pl.DataFrame({"t": [1, 5, 10], "v": [1.0, 2.0, 3.0], "k": [1, 1, 2]})
    right = pl.DataFrame({"t": [0, 4, 9], "v": [10.0, None, 30.0], "k": [1, 1, 2], "w": ["a", "b", None]})
    out = left.join_asof(right, on="t")
    assert out.columns == ["t", "v", "k", "v_right", "k_right", "w"]          # the right `on` coalesced away
    assert out["v_right"].to_list() == [10.0, None, 30.0] and out["w"].to_list() == ["a", "b", None]
    out = left.join_asof(right, on="t", coalesce=False, suffix="_q")
    assert out.columns == ["t", "v", "k", "t_q", "v_q", "k_q", "w"] and out["t_q"].to_list() == [0, 4, 9]
    out = left.join_asof(right, on="t", by="k")                                # the right `by` column is dropped
    assert out.columns == ["t", "v", "k", "v_right", "w"]
    r2 = pl.DataFrame({"u": [0, 4, 9], "kk": [1, 1, 2], "w": ["a", "b", None]})
    for coalesce in (True, False):                                             # different names: both kept
        out = left.join_asof(r2, left_on="t", right_on=pl.col("u"), by_left="k", by_right="kk", coalesce=coalesce)
        assert out.columns == ["t", "v", "k", "u", "w"] and out["u"].to_list() == [0, 4, 9]
    lazy = left.lazy().join_asof(right.lazy(), on="t", strategy="forward", allow_parallel=False, force_parallel=True)
    info = {}
    assert lazy.collect(info=info)["v_right"].to_list() == [None, 30.0, None] and info["asof_path"] == "staged"


def test_logical_dtypes_and_temporal_tolerances(gpu):
    t0 = dt.datetime(2020, 1, 1, 9, 0, 0)
    sec = lambda *s: [t0 + dt.timedelta(seconds=x) for x in s]  # noqa: E731
    for unit in ("us", "ms", "ns"):
        trades = pl.DataFrame({"time": pl.Series("time", np.array(sec(1, 1, 3, 6), f"M8[{unit}]")),
                               "stock": ["A", "B", "B", "C"]})
        quotes = pl.DataFrame({"time": pl.Series("time", np.array(sec(0, 2, 4, 6), f"M8[{unit}]")),
                               "stock": ["A", "B", "C", "A"], "quote": [100, 300, 501, 102],
                               "d": pl.Series("d", np.array([1, 2, 3, 4], "m8[ms]"))})
        with pytest.warns(UserWarning, match="Sortedness of columns cannot be checked when 'by' groups provided"):
            out = trades.join_asof(quotes, on="time", by="stock", tolerance="2s")
        assert out["quote"].to_list() == [100, None, 300, 501]                 # test_join_asof.py:249
        assert out.schema["time"] == pl.Datetime(unit) and out.schema["d"] == pl.Duration("ms")
        if unit == "us":
            assert out["time"].to_list() == sec(1, 1, 3, 6)
        with warnings.catch_warnings():
            warnings.simplefilter("error", UserWarning)                        # no warning without the check
            out = trades.join_asof(quotes, on="time", by="stock", tolerance=dt.timedelta(seconds=1),
                                   check_sortedness=False)
        assert out["quote"].to_list() == [100, None, 300, None]                # :263
        out = trades.join_asof(quotes, on="time", tolerance="1500ms", coalesce=False)
        assert out["quote"].to_list() == [100, 100, 300, 102] and out.schema["time_right"] == pl.Datetime(unit)
    days = pl.DataFrame({"d": pl.Series("d", np.array([10, 20, 30], np.int32), pl.Date)})
    other = pl.DataFrame({"d": pl.Series("d", np.array([9, 27], np.int32), pl.Date), "x": [1, 2]})
    assert days.join_asof(other, on="d", tolerance="2d")["x"].to_list() == [1, None, None]
    assert days.join_asof(other, on="d", strategy="nearest", tolerance="1w")["x"].to_list() == [1, 2, 2]


@pytest.mark.parametrize("dtype", ["Int8", "Int16", "UInt8", "UInt16"])
def test_small_integer_keys_run_as_int32(gpu, dtype):
    t = getattr(pl, dtype)
    ii = np.iinfo(t.np_dtype)
    left = pl.DataFrame({"t": pl.Series("t", [ii.min, 0 if ii.min else 1, ii.max], t)})
    right = pl.DataFrame({"t": pl.Series("t", [ii.min, ii.max - 1], t), "rid": [0, 1]})
    out = left.join_asof(right, on="t", strategy="nearest", coalesce=False)
    assert out["rid"].to_list() == [0, 1 if ii.min else 0, 1] and out.schema["t_right"] is t
    assert left.join_asof(right, on="t", tolerance=1)["rid"].to_list() == [0, None if ii.min else 0, 1]


def test_sortedness(gpu):
    msg = "argument in operation 'asof_join' is not sorted, please sort the 'expr/series/column' first"
    up = pl.DataFrame({"t": [1, 2, 3], "x": [1, 2, 3]})
    down = pl.DataFrame({"t": [2, 1, 3], "x": [1, 2, 3]})
    late_null = pl.DataFrame({"t": [1, None, 3], "x": [1, 2, 3]})
    first_null = pl.DataFrame({"t": [None, 1, 3], "x": [1, 2, 3]})
    for l, r in ((down, up), (up, down), (late_null, up), (up, late_null)):
        with pytest.raises(pl.InvalidOperationError, match=msg):
            l.join_asof(r, on="t")
    assert first_null.join_asof(first_null, on="t")["x_right"].to_list() == [None, 2, 3]
    with pytest.warns(UserWarning, match="Sortedness of columns cannot be checked"):
        down.join_asof(down, on="t", by="x")
    # an unsorted left is searched row by row: the same rows as the yardstick
    rng = np.random.default_rng(31)
    left = rng.permutation(sorted_keys(rng, 2 * T + 11, 3000))
    right = sorted_keys(rng, 3 * L, 2500)
    for strategy in STRATEGIES:
        exp_rows, exp_ok = expect(left, None, right, None, strategy, sorted_left=False)
        for path in (0, 2):
            prev = N.set_option("asof_path", path)
            try:
                out = pl.DataFrame({"t": pl.Series.from_numpy("t", left)}).join_asof(
                    pl.DataFrame({"t": pl.Series.from_numpy("t", right),
                                  "rid": pl.Series.from_numpy("rid", np.arange(len(right)))}),
                    on="t", strategy=strategy, check_sortedness=False)
            finally:
                N.set_option("asof_path", prev)
            rows, ok = frame_rows(out)
            assert ok.tolist() == exp_ok.tolist() and rows.tolist() == exp_rows.tolist(), (strategy, path)
    # an unsorted right only has to return rows of the right side
    wild = rng.permutation(right)
    for strategy in STRATEGIES:
        for path in (0, 2):
            prev = N.set_option("asof_path", path)
            try:
                rows, ok, _ = c_call(pl.Series.from_numpy("l", np.sort(left)), pl.Series.from_numpy("r", wild), strategy)
            finally:
                N.set_option("asof_path", prev)
            assert ((rows >= 0) & (rows < len(wild)))[ok].all() and (rows[~ok] == -1).all()


def test_refusals(gpu):
    a = pl.DataFrame({"t": [1, 2], "f": [1.0, 2.0], "s": ["a", "b"], "b": [True, False], "k": [1, 1]})
    with pytest.raises(pl.ComputeError, match="mismatching key dtypes in asof-join: `Int64` and `Float64`"):
        a.join_asof(a, left_on="t", right_on="f")
    with pytest.raises(pl.ComputeError, match="mismatching dtypes in 'by' parameter of asof-join: `Int64` and `String`"):
        a.join_asof(a, on="t", by_left="k", by_right="s", check_sortedness=False)
    with pytest.raises(pl.InvalidOperationError, match="asof join with tolerance is only supported on numeric/temporal"):
        a.join_asof(a, on="s", tolerance=1)
    with pytest.raises(pl.InvalidOperationError, match="join_asof on a String key is not supported"):
        a.join_asof(a, on="s")
    with pytest.raises(pl.InvalidOperationError, match="join_asof on a Boolean key is not supported"):
        a.join_asof(a, on="b")
    import pyarrow as pa

    cat = pl.DataFrame({"c": pl.Series.from_arrow("c", pa.array(["x", "y"], pa.string()).dictionary_encode())})
    with pytest.raises(pl.InvalidOperationError, match="join_asof on a Categorical key is not supported"):
        cat.join_asof(cat, on="c")
    with pytest.raises(pl.ComputeError, match='unable to find column "nope"'):
        a.join_asof(a, on="nope")
    with pytest.raises(pl.ComputeError, match='unable to find column "nope"'):
        a.join_asof(a, on="t", by="nope", check_sortedness=False)
    with pytest.raises(pl.ComputeError, match="does not fit the key dtype"):
        a.join_asof(a, on="t", tolerance=2**63)
    with pytest.raises(pl.InvalidOperationError, match="timedelta string language"):
        a.join_asof(a, on="t", tolerance="2s")


# ------------------------------------------------------------------ by groups
def by_frames(left, lv, right, rv, by_l, by_r, kinds):
    """Frames with `on` = t, `by` = k0.., and on the right a row id and a
    nullable payload; kinds[j]: "int" / "int32" / "str" / "cat" of by column j."""
    import pyarrow as pa

    def key(name, vals, kind):
        if kind == "int":
            return pl.Series(name, vals, pl.Int64)
        if kind == "int32":
            return pl.Series(name, vals, pl.Int32)
        strs = [None if v is None else f"s{v}" for v in vals]
        if kind == "str":
            return pl.Series(name, strs, pl.String)
        return pl.Series.from_arrow(name, pa.array(strs, pa.string()).dictionary_encode())

    lcols = [pl.Series.from_numpy("t", left, lv)]
    rcols = [pl.Series.from_numpy("t", right, rv), pl.Series.from_numpy("rid", np.arange(len(right), dtype=np.int64)),
             pl.Series.from_numpy("pay", np.arange(len(right)) * 0.5, np.arange(len(right)) % 5 != 0)]
    for j, kind in enumerate(kinds):
        lcols.append(key(f"k{j}", by_l[j], kind))
        rcols.append(key(f"k{j}", by_r[j], kind))
    return pl.DataFrame(lcols), pl.DataFrame(rcols)


def grouped_sides(rng, n_left, n_right, groups, interleave_right, nulls, ncols=1):
    """Keys ascending inside every group; the left rows interleave the groups
    (time-sorted overall); the right rows arrive grouped in sorted order or
    interleaved."""
    left, right = sorted_keys(rng, n_left, 4 * n_right // max(groups, 1) + 10), sorted_keys(rng, n_right, 4 * n_right // max(groups, 1) + 10)
    gl = rng.integers(0, groups + 1, n_left)          # group `groups` is absent on the right
    gr = rng.integers(0, groups, n_right)
    gr[gr == 1] = 0 if groups > 2 else gr[gr == 1]    # group 1 is absent on the right too, where there are enough
    if groups > 3:
        gl[gl == 2] = 3                               # and group 2 on the left
    if not interleave_right:
        order = np.argsort(gr, kind="stable")
        gr, right = gr[order], right[order]
    lv, rv = np.ones(n_left, bool), np.ones(n_right, bool)
    cols_l = [[int(g) for g in gl]] + [[int(g) % 3 for g in gl] for _ in range(ncols - 1)]
    cols_r = [[int(g) for g in gr]] + [[int(g) % 3 for g in gr] for _ in range(ncols - 1)]
    if nulls:
        lv[rng.random(n_left) < 0.05] = False
        rv[rng.random(n_right) < 0.1] = False         # null `on` values in the middle of groups
        if groups > 4:
            rv[gr == 4] = False                       # a group whose right `on` values are all null
        for c in cols_l:
            for i in rng.integers(0, n_left, max(1, n_left // 20)):
                c[i] = None
        for c in cols_r:
            for i in rng.integers(0, n_right, max(1, n_right // 20)):
                c[i] = None
    return left, lv, right, rv, cols_l, cols_r


@pytest.mark.parametrize("kinds", [("int",), ("int", "int32"), ("str",), ("cat",)], ids=lambda k: "+".join(k))
@pytest.mark.parametrize("interleave_right", [False, True])
def test_by_groups(gpu, kinds, interleave_right):
    rng = np.random.default_rng(41 + len(kinds) + 2 * interleave_right)
    for groups, nulls in ((1, False), (2, True), (100, True), (5000, False)):
        n_left, n_right = (700, 500) if groups < 5000 else (3 * T + 5, 12000)
        left, lv, right, rv, by_l, by_r = grouped_sides(rng, n_left, n_right, groups, interleave_right, nulls,
                                                        len(kinds))
        lf, rf = by_frames(left, lv, right, rv, by_l, by_r, kinds)
        by = [f"k{j}" for j in range(len(kinds))]
        for strategy in STRATEGIES:
            for allow_eq, tol in ((True, None), (False, 3)):
                exp_rows, exp_ok = asof_ref_bounds(left, lv, right, rv, strategy, allow_eq, tol, by_left=by_l,
                                                   by_right=by_r)
                if n_left + n_right <= SCAN_ROWS:
                    r2, o2 = asof_ref_scan(left, lv, right, rv, strategy, allow_eq, tol, by_left=by_l, by_right=by_r)
                    assert o2.tolist() == exp_ok.tolist() and r2.tolist() == exp_rows.tolist()
                info = {}
                out = lf.lazy().join_asof(rf.lazy(), on="t", by=by, strategy=strategy, tolerance=tol,
                                          allow_exact_matches=allow_eq, check_sortedness=False).collect(info=info)
                what = (kinds, interleave_right, groups, strategy, allow_eq, tol)
                assert info["asof_path"] == "ranged", what
                if not nulls and groups > 1 and kinds[0] == "int":  # (string codes do not sort as the integers)
                    assert info["asof_right_sorted"] == (not interleave_right), what
                rows, ok = frame_rows(out)
                assert ok.tolist() == exp_ok.tolist(), what
                assert rows.tolist() == exp_rows.tolist(), what
                assert out.columns == ["t"] + by + ["rid", "pay"]
                pay_ok = out["pay"].validity_numpy()
                assert pay_ok.tolist() == (exp_ok & (exp_rows % 5 != 0)).tolist(), what
                assert out["pay"].to_numpy()[pay_ok].tolist() == (exp_rows[pay_ok] * 0.5).tolist(), what
                assert out["t"].validity_numpy().tolist() == lv.tolist()


def test_by_sorted_right_takes_no_sort_unless_asked(gpu, plgpu_option):
    rng = np.random.default_rng(43)
    left, lv, right, rv, by_l, by_r = grouped_sides(rng, 300, 400, 7, False, False)
    lf, rf = by_frames(left, lv, right, rv, by_l, by_r, ("int",))
    exp_rows, exp_ok = asof_ref_bounds(left, lv, right, rv, "backward", by_left=by_l, by_right=by_r)
    for presorted in (1, 0):
        plgpu_option("over_presorted", presorted)
        info = {}
        out = lf.lazy().join_asof(rf.lazy(), on="t", by="k0", check_sortedness=False).collect(info=info)
        assert info["asof_right_sorted"] == bool(presorted)
        rows, ok = frame_rows(out)
        assert ok.tolist() == exp_ok.tolist() and rows.tolist() == exp_rows.tolist()


def test_by_large(gpu):
    """2^22 x 2^20 rows in 100 groups, against asof_ref_bounds only."""
    rng = np.random.default_rng(47)
    n_left, n_right, groups = 1 << 22, 1 << 20, 100
    left = np.sort(rng.integers(0, 1 << 40, n_left))
    right = np.sort(rng.integers(0, 1 << 40, n_right))
    gl, gr = rng.integers(0, groups, n_left), rng.integers(0, groups, n_right)
    lf = pl.DataFrame([pl.Series.from_numpy("t", left), pl.Series.from_numpy("k", gl)])
    rf = pl.DataFrame([pl.Series.from_numpy("t", right), pl.Series.from_numpy("k", gr),
                       pl.Series.from_numpy("rid", np.arange(n_right, dtype=np.int64))])
    info = {}
    out = lf.lazy().join_asof(rf.lazy(), on="t", by="k", check_sortedness=False).collect(info=info)
    assert info["asof_path"] == "ranged" and info["asof_right_sorted"] is False
    exp_rows, exp_ok = asof_ref_bounds(left, None, right, None, "backward", codes=(gl, gr))
    rows, ok = frame_rows(out)
    assert np.array_equal(ok, exp_ok) and np.array_equal(rows, exp_rows)
