"""CPU: join_asof -- the two restatements of the reference (tests/asof_ref.py)
agree with each other on randomized inputs and reproduce the cases transcribed
from the reference's own tests (tests/golden/asof_cases.json), so the yardstick
of tests/test_gpu_join_asof.py is itself checked; plan construction, explain()
and argument parsing; the refusals that need no data; the tolerance
conversions; and the argument checks of plgpu_join_asof / plgpu_is_sorted_asc,
which run before any device work."""

import ctypes as C
import datetime as dt
import itertools

import numpy as np
import pytest

import polaroid_amd as pl
from asof_ref import asof_ref_bounds, asof_ref_scan
from conftest import load_golden

GOLDEN = load_golden("asof_cases.json")
CASES = GOLDEN["cases"]
STRATEGIES = ("backward", "forward", "nearest")


def case_arrays(case):
    np_t = np.dtype(case["dtype"])

    def side(vals):
        valid = np.array([v is not None for v in vals], bool)
        return np.array([0 if v is None else v for v in vals], dtype=np_t), valid

    (left, lv), (right, rv) = side(case["left"]), side(case["right"])
    return left, lv, right, rv


def check_case(case, rows, ok, what):
    _, _, right, _ = case_arrays(case)
    if "expected_rows" in case:
        got = [int(r) if k else None for r, k in zip(rows, ok)]
        assert got == case["expected_rows"], (case["name"], what, got)
    else:
        got = [right[r].item() if k else None for r, k in zip(rows, ok)]
        assert got == case["expected_values"], (case["name"], what, got)


# ------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_both_readings_reproduce_the_reference_cases(case):
    left, lv, right, rv = case_arrays(case)
    kw = dict(strategy=case["strategy"], allow_eq=case.get("allow_eq", True), tolerance=case.get("tolerance"),
              by_left=case.get("by_left"), by_right=case.get("by_right"))
    for fn in (asof_ref_scan, asof_ref_bounds):
        rows, ok = fn(left, lv, right, rv, **kw)
        check_case(case, rows, ok, fn.__name__)


def test_golden_file_shape():
    names = set()
    for c in CASES:
        assert set(c) >= {"name", "source", "dtype", "strategy", "left", "right"}, c.get("name")
        assert ("expected_rows" in c) != ("expected_values" in c), c["name"]
        assert len(c.get("expected_rows", c.get("expected_values"))) == len(c["left"]), c["name"]
        assert c["name"] not in names
        names.add(c["name"])
        assert ":" in c["source"] and c["strategy"] in STRATEGIES
        assert ("by_left" in c) == ("by_right" in c)
    assert {"rs_backward_1", "nearest_by_tolerance", "large_int_u64_nearest", "nearest_no_exact_6"} <= names
    assert any("Int128" in line for line in GOLDEN["header"])


def random_sides(rng, n_left, n_right, dtype, nulls, groups, dup):
    span = max(2, (n_left + n_right) // dup)
    if np.dtype(dtype).kind == "f":
        pool = (rng.integers(-span, span, 64) / 4).astype(dtype)
        left = np.sort(rng.choice(pool, n_left)) if n_left else np.zeros(0, dtype)
        right = np.sort(rng.choice(pool, n_right)) if n_right else np.zeros(0, dtype)
    else:
        left = np.sort(rng.integers(-span, span, n_left)).astype(dtype)
        right = np.sort(rng.integers(-span, span, n_right)).astype(dtype)
    lv, rv = np.ones(n_left, bool), np.ones(n_right, bool)
    if nulls:  # at the front, where ascending keys with nulls first have them
        lv[:rng.integers(0, n_left + 1) // 3] = False
        rv[:rng.integers(0, n_right + 1) // 3] = False
    by_l = by_r = None
    if groups:
        # every group's rows keep their ascending order; rows of different groups interleave
        by_l = [[int(g) if g >= 0 else None for g in rng.integers(-1 if nulls else 0, groups, n_left)]]
        by_r = [[int(g) if g >= 0 else None for g in rng.integers(-1 if nulls else 0, groups + 1, n_right)]]
        if nulls and n_right:
            rv = rng.random(n_right) > 0.1  # null `on` values anywhere in a group
    return left, lv, right, rv, by_l, by_r


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("allow_eq", [True, False])
def test_the_two_readings_agree_on_random_inputs(strategy, allow_eq):
    rng = np.random.default_rng(20240 + 7 * STRATEGIES.index(strategy) + int(allow_eq))
    shapes = [(0, 0), (0, 5), (5, 0), (1, 1), (40, 30), (300, 200), (64, 900)]
    for (n_left, n_right), dtype, nulls, groups, dup in itertools.product(
            shapes, ("int64", "float32"), (False, True), (0, 1, 5), (1, 8)):
        left, lv, right, rv, by_l, by_r = random_sides(rng, n_left, n_right, dtype, nulls, groups, dup)
        for tol in (None, 0, 2, -2):
            kw = dict(strategy=strategy, allow_eq=allow_eq, tolerance=tol, by_left=by_l, by_right=by_r)
            a, b = asof_ref_scan(left, lv, right, rv, **kw), asof_ref_bounds(left, lv, right, rv, **kw)
            what = (n_left, n_right, dtype, nulls, groups, dup, tol)
            assert a[1].tolist() == b[1].tolist(), what
            assert a[0].tolist() == b[0].tolist(), what


def test_readings_on_extremes_and_total_order():
    imin, imax = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    left = np.array([imin, -1, imax], np.int64)
    right = np.array([imin, 0, imax], np.int64)
    for fn in (asof_ref_scan, asof_ref_bounds):
        rows, ok = fn(left, None, right, None, "nearest", allow_eq=False)
        assert rows.tolist() == [1, 1, 1] and ok.all()     # |-1 - 0| = 1 against 2^63 - 1
        rows, ok = fn(left, None, right, None, "nearest", tolerance=imax)
        assert rows.tolist() == [0, 1, 2]
        rows, ok = fn(np.array([imax], np.int64), None, np.array([imin], np.int64), None, "backward", tolerance=imax)
        assert not ok[0]                                     # the exact difference is 2^64 - 1
        u = np.array([2**63 + 5], np.uint64)
        rows, ok = fn(u, None, np.array([3, 2**63 + 4, 2**64 - 1], np.uint64), None, "nearest")
        assert rows.tolist() == [1]
        # TotalOrd (our rule, not the reference's partial_cmp): NaN is the greatest value and equals itself
        f = np.array([-0.0, 1.0, np.inf, np.nan], np.float64)
        r = np.array([-np.inf, 0.0, np.inf, np.nan, np.nan], np.float64)
        rows, ok = fn(f, None, r, None, "backward")
        assert rows.tolist() == [1, 1, 2, 4] and ok.all()
        rows, ok = fn(f, None, r, None, "forward", allow_eq=False)
        assert rows.tolist() == [2, 2, 3, -1] and ok.tolist() == [True, True, True, False]
        rows, ok = fn(f, None, r, None, "backward", tolerance=1.0)
        assert ok.tolist() == [True, True, False, False]     # inf - inf and NaN - NaN pass no tolerance


def test_nearest_against_the_brute_force_yardstick():
    """test_asof_join_nearest_reference (test_join_asof.py:527): the closest
    right key, ties to the later row; without exact matches equal keys are
    skipped.  Its random draws are replaced by a seeded sweep."""
    rng = np.random.default_rng(527)
    frames = []
    for counts in itertools.product([0, 1, 2], repeat=4):
        keys = sorted(sum(([int(rng.integers(0, 11))] * c for c in counts), []))
        frames.append(np.array(keys, np.int32))
    for allow_eq in (True, False):
        for left, right in itertools.product(frames[::3], frames):
            exp = []
            for l in left:
                cand = [(abs(int(l) - int(r)), -j) for j, r in enumerate(right) if allow_eq or r != l]
                exp.append(-min(cand)[1] if cand else None)
            for fn in (asof_ref_scan, asof_ref_bounds):
                rows, ok = fn(left, None, right, None, "nearest", allow_eq=allow_eq)
                assert [int(r) if k else None for r, k in zip(rows, ok)] == exp, (left, right, allow_eq, fn.__name__)


# ------------------------------------------------------------- construction
def empty_lazy():
    return pl.LazyFrame(("scan", pl.DataFrame()))


def test_plan_node_and_explain():
    a, b = empty_lazy(), empty_lazy()
    q = a.join_asof(b, on="t")
    assert q._node[0] == "join_asof" and q._node[3:] == ("t", "t", None, None, "backward", "_right", None, True, True,
                                                        True)
    q = a.join_asof(b, left_on=pl.col("t"), right_on="u", by="sym", strategy="nearest", tolerance="2h15m",
                    allow_exact_matches=False, coalesce=False, check_sortedness=False, suffix="_q",
                    allow_parallel=False, force_parallel=True)
    assert q._node[3:] == ("t", "u", ("sym",), ("sym",), "nearest", "_q", "2h15m", False, False, False)
    text = q.explain()
    assert text.splitlines()[0] == "ASOF JOIN NEAREST ON t = u BY ['sym'] = ['sym'] TOLERANCE '2h15m'"
    assert text.count("DF []") == 2
    assert a.join_asof(b, on="t").explain().splitlines()[0] == "ASOF JOIN BACKWARD ON t = t"


def test_by_argument_parsing():
    """test_join_asof_by_argument_parsing (test_join_asof.py:1208): any sequence."""
    a, b = empty_lazy(), empty_lazy()
    as_list = a.join_asof(b, on="n", by=["id1", "id2"])._node[5:7]
    assert as_list == a.join_asof(b, on="n", by=("id1", "id2"))._node[5:7] == (("id1", "id2"), ("id1", "id2"))
    assert as_list == a.join_asof(b, on="n", by_left=["id1", "id2"], by_right=("id1", "id2"))._node[5:7]
    assert a.join_asof(b, on="n", by_left="x", by_right="y")._node[5:7] == (("x",), ("y",))


def test_invalid_arguments():
    """test_join_asof_invalid_args (test_join_asof.py:1243) and the plan-time refusals."""
    df = pl.DataFrame()
    with pytest.raises(TypeError, match="expected `on` to be str or Expr, got 'list'"):
        df.join_asof(df, on=["a"])
    with pytest.raises(TypeError, match="expected `left_on` to be str or Expr, got 'list'"):
        df.join_asof(df, left_on=["a"], right_on="a")
    with pytest.raises(TypeError, match="expected `right_on` to be str or Expr, got 'list'"):
        df.join_asof(df, left_on="a", right_on=["a"])
    a, b = empty_lazy(), empty_lazy()
    with pytest.raises(ValueError, match="you should pass the column to join on as an argument"):
        a.join_asof(b)
    with pytest.raises(ValueError, match="you should pass the column to join on as an argument"):
        a.join_asof(b, left_on="t")
    with pytest.raises(pl.InvalidOperationError, match="expected both 'by_left' and 'by_right' to be set in 'asof_join'"):
        a.join_asof(b, on="t", by_left=None, by_right=["k"])
    with pytest.raises(pl.InvalidOperationError, match="expected equal number of columns in 'by_left' and 'by_right'"):
        a.join_asof(b, on="t", by_left=["k", "j"], by_right=["k"])
    with pytest.raises(pl.InvalidOperationError, match="1..8 plain column names"):
        a.join_asof(b, on="t", by=[f"k{i}" for i in range(9)])
    with pytest.raises(pl.InvalidOperationError, match="computed expression is not supported"):
        a.join_asof(b, left_on=pl.col("t") + 1, right_on="t")
    with pytest.raises(ValueError, match="invalid `strategy` argument 'closest'"):
        a.join_asof(b, on="t", strategy="closest")
    with pytest.raises(pl.InvalidOperationError, match="cannot parse the tolerance 'foo'"):
        a.join_asof(b, on="t", tolerance="foo")
    with pytest.raises(pl.ComputeError, match="cannot use month offset"):
        a.join_asof(b, on="t", tolerance="1mo")


def test_duration_strings():
    from polaroid_amd.frame import _duration_ns

    assert _duration_ns("5m") == 300 * 10**9 and _duration_ns("2h15m") == 8100 * 10**9
    assert _duration_ns("1d6h") == 30 * 3600 * 10**9 and _duration_ns("1w") == 7 * 86400 * 10**9
    assert _duration_ns("3ns2us1ms") == 1_002_003 and _duration_ns("-10s") == -10**10 and _duration_ns("0s") == 0
    for bad in ("1mo", "2q", "1y", "3i"):
        with pytest.raises(pl.ComputeError, match="only ns us ms s m h d w"):
            _duration_ns(bad)
    for bad in ("", "s", "1", "1x", "1 s", "1.5s"):
        with pytest.raises(pl.InvalidOperationError, match="cannot parse"):
            _duration_ns(bad)


def key_of(dtype):
    return pl.Series.from_device("t", dtype, 0x1000, 0)  # borrowed and never read


def test_tolerance_conversions():
    from polaroid_amd.frame import _asof_tolerance

    assert _asof_tolerance(None, key_of(pl.Int64)) == (0, 0, 0.0)
    assert _asof_tolerance(3, key_of(pl.Int64)) == (1, 3, 0.0)
    assert _asof_tolerance(-3, key_of(pl.Int32)) == (1, -3, 0.0)
    assert _asof_tolerance(2.9, key_of(pl.Int64)) == (1, 2, 0.0)            # toward zero, as NumCast
    assert _asof_tolerance(0.5, key_of(pl.Float32)) == (1, 0, 0.5)
    assert _asof_tolerance(2, key_of(pl.Float64)) == (1, 0, 2.0)
    assert _asof_tolerance(2**64 - 1, key_of(pl.UInt64)) == (1, -1, 0.0)    # the bits of the UInt64
    assert _asof_tolerance(-2**63, key_of(pl.Int64)) == (1, -2**63, 0.0)
    td = dt.timedelta(days=1, hours=4)
    assert _asof_tolerance(td, key_of(pl.Datetime("us")))[1] == 28 * 3600 * 10**6
    assert _asof_tolerance("1d4h", key_of(pl.Datetime("ms")))[1] == 28 * 3600 * 10**3
    assert _asof_tolerance("1d4h", key_of(pl.Duration("ns")))[1] == 28 * 3600 * 10**9
    assert _asof_tolerance("1d4h", key_of(pl.Date))[1] == 1 and _asof_tolerance("3w", key_of(pl.Date))[1] == 21
    assert _asof_tolerance("1500us", key_of(pl.Datetime("ms")))[1] == 1    # truncated to the unit
    assert _asof_tolerance(7, key_of(pl.Datetime("us")))[1] == 7           # a number is in the key's unit
    # a value that does not fit the key's physical type raises instead of wrapping
    for tol, dtype in ((2**31, pl.Int32), (-1, pl.UInt32), (2**63, pl.Int64), (2**64, pl.UInt64), (-1, pl.UInt64),
                       (float("inf"), pl.Int64), ("400000000w", pl.Date)):  # 2.8e9 days
        with pytest.raises(pl.ComputeError, match="does not fit the key dtype"):
            _asof_tolerance(tol, key_of(dtype))
    with pytest.raises(pl.InvalidOperationError, match="timedelta string language"):
        _asof_tolerance("2s", key_of(pl.Int64))
    with pytest.raises(pl.InvalidOperationError, match="timedelta string language"):
        _asof_tolerance(td, key_of(pl.Float64))
    with pytest.raises(TypeError, match="must be a number, a timedelta or a duration string"):
        _asof_tolerance([None], key_of(pl.Int64))


def test_constants_mirror_the_kernels():
    import os
    import re

    from conftest import ROOT
    from polaroid_amd import _native as N

    src = open(os.path.join(ROOT, "polaroid_amd", "csrc", "asof.hip")).read()
    threads = int(re.search(r"kAsofThreads = (\d+);", src).group(1))
    per = int(re.search(r"kAsofPer = (\d+);", src).group(1))
    assert N.ASOF_TILE_ROWS == threads * per and N.ASOF_TILE_ROWS % 64 == 0
    assert N.ASOF_LDS_VALUES == int(re.search(r"kAsofLds = (\d+);", src).group(1))
    assert N.ASOF == {"backward": 0, "forward": 1, "nearest": 2}


# ------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def N():
    from polaroid_amd import _native

    _native.lib()
    return _native


def host_col(N, dtype, n, validity=False):
    c = N.Column()
    c.dtype, c.length = dtype, n
    c.values = 0x1000  # never dereferenced: validation fails before any device work
    if validity:
        c.validity = 0x2000
    return c


def call(N, left, right, lo=None, hi=None, rows=None, strategy=0, out=True):
    o, path = N.Column(), C.c_int32(7)
    ref = lambda c: None if c is None else C.byref(c)  # noqa: E731
    rc = N.lib().plgpu_join_asof(ref(left), ref(right), ref(lo), ref(hi), ref(rows), strategy, 1, 0, 0, 0.0,
                                 C.byref(o) if out else None, C.byref(path), None)
    return rc, N.lib().plgpu_last_error().decode()


def test_join_asof_argument_checks_without_gpu(N):
    i64 = lambda n=4, v=False: host_col(N, N.I64, n, v)  # noqa: E731
    u32 = lambda n=4, v=False: host_col(N, N.U32, n, v)  # noqa: E731
    assert call(N, None, i64())[0] == N.ERR_INVALID
    assert call(N, i64(), None)[0] == N.ERR_INVALID
    assert call(N, i64(), i64(), out=False)[0] == N.ERR_INVALID
    for strategy in (-1, 3):
        rc, msg = call(N, i64(), i64(), strategy=strategy)
        assert rc == N.ERR_INVALID and "unknown strategy" in msg
    rc, msg = call(N, i64(), i64(), lo=u32())
    assert rc == N.ERR_INVALID and "lo and hi come together" in msg
    assert call(N, i64(), i64(), hi=u32())[0] == N.ERR_INVALID
    for bad, what in ((host_col(N, N.I64, 4), "UInt32"), (u32(5), "wrong length"), (u32(4, True), "nullable")):
        rc, msg = call(N, i64(), i64(6), lo=bad, hi=u32())
        assert rc == N.ERR_INVALID and "lo" in msg and what in msg
        rc, msg = call(N, i64(), i64(6), lo=u32(), hi=bad)
        assert rc == N.ERR_INVALID and "hi" in msg and what in msg
    for bad, what in ((host_col(N, N.I32, 6), "UInt32"), (u32(4), "wrong length"), (u32(6, True), "nullable")):
        rc, msg = call(N, i64(), i64(6), rows=bad)
        assert rc == N.ERR_INVALID and "right_rows" in msg and what in msg
    rc, msg = call(N, i64(), i64(6, True), lo=u32(), hi=u32())
    assert rc == N.ERR_INVALID and "without a validity buffer" in msg
    for n_right in (2**32 - 1, 2**32, 2**40):
        rc, msg = call(N, i64(), i64(n_right))
        assert rc == N.ERR_INVALID and "2^32 - 1" in msg
    rc, msg = call(N, i64(), host_col(N, N.I32, 4))
    assert rc == N.ERR_SCHEMA and "mismatching key dtypes in asof-join" in msg
    for dtype in (N.BOOL, N.STR, N.I8, N.I16, N.U8, N.U16):
        rc, msg = call(N, host_col(N, dtype, 4), host_col(N, dtype, 4))
        assert rc == N.ERR_SCHEMA and "join_asof keys must be" in msg


def test_is_sorted_argument_checks_without_gpu(N):
    a, f = C.c_int32(7), C.c_int32(7)
    c = host_col(N, N.I64, 4)
    lib = N.lib()
    assert lib.plgpu_is_sorted_asc(None, C.byref(a), C.byref(f), None) == N.ERR_INVALID
    assert lib.plgpu_is_sorted_asc(C.byref(c), None, C.byref(f), None) == N.ERR_INVALID
    assert lib.plgpu_is_sorted_asc(C.byref(c), C.byref(a), None, None) == N.ERR_INVALID
    for dtype in (N.BOOL, N.STR, N.I16):
        c = host_col(N, dtype, 4)
        assert lib.plgpu_is_sorted_asc(C.byref(c), C.byref(a), C.byref(f), None) == N.ERR_SCHEMA
    for n in (0, 1):  # nothing to compare: sorted, and no device work
        c = host_col(N, N.F32, n, True)
        assert lib.plgpu_is_sorted_asc(C.byref(c), C.byref(a), C.byref(f), None) == N.OK
        assert (a.value, f.value) == (1, 1)


def test_asof_path_option_round_trip(N):
    prev = N.set_option("asof_path", 2)
    assert N.get_option("asof_path") == 2
    assert N.set_option("asof_path", prev) == 2
