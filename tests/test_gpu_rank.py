"""GPU: rank (plgpu_rank) at the seams of its three launches -- tile, block and
word edges, both carries, every method and direction, value and null patterns,
segments -- its dtypes, its sliced inputs, and end to end, plain and over groups.

Reference.  tests/rank_ref.py: the reference's rank restated (rank_ref, used up
to a few hundred rows) and its numpy closed form (rank_closed_all /
ranks_from_starts); tests/test_rank.py pins the two to each other and to the
reference's own cases.  Ranks are integers, or halves of integers for
"average": every value, dtype and validity bit is compared exactly, and a null
row's bytes are zero."""

import ctypes as C
import functools

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from polaroid_amd import _native as N
from rank_ref import METHODS, rank_closed_all, rank_ref, ranks_from_starts, sorted_inputs
from test_rank import case_inputs, check_case

pytestmark = pytest.mark.gpu

T = N.CUM_TILE    # rows of one workgroup of the rank kernels: one summary, one carry each way
B = N.CUM_BLOCK   # rows of one pass of a workgroup over its tile
NS = 3 * T + 5
LENGTHS = [0, 1, 2, 63, 64, 65, B - 1, B, B + 1, T - 1, T, T + 1, NS]
_OUT = {m: (np.float64 if m == "average" else np.uint32) for m in METHODS}


def _series(vals, valid, name="x", **kw):
    return pl.Series.from_numpy(name, vals, **kw) if valid is None else pl.Series.from_numpy(name, vals, valid, **kw)


def _mask(valid, n):
    return np.ones(n, bool) if valid is None else valid


def _check(got, exp, ok, method, what, nullable=None):
    """`got` a device Series; `exp` the ranks (0 at null rows), `ok` the
    validity; `nullable`: whether the output has a validity buffer (None: not
    checked)."""
    gv, gok = got.to_numpy(), got.validity_numpy()
    assert got.dtype is (pl.Float64 if method == "average" else pl.UInt32), what
    assert gv.dtype == _OUT[method] and gv.shape == ok.shape, what
    assert np.array_equal(gok, ok), (what, np.flatnonzero(gok != ok)[:8])
    if nullable is not None and len(ok):
        assert bool(got._col.validity) == nullable, what
    bad = np.flatnonzero(gv != np.where(ok, exp, 0))
    assert bad.size == 0, (what, bad[:8], gv[bad[:8]], exp[bad[:8]])


def _check_all(s, vals, valid, desc, what, groups=None):
    """Series._rank of every method against the closed form (and, for short
    columns, against the restated loop)."""
    n = len(vals)
    ok = _mask(valid, n)
    ref = rank_closed_all(vals, ok, desc, groups)
    for m in METHODS:
        exp = ref[m][0]
        if n <= 130 and groups is None:
            assert np.array_equal(exp, rank_ref(vals, ok, m, desc)[0])
        _check(s._rank(m, desc), exp, ok, m, (what, m, desc), valid is not None)


def _value_patterns(n, rng):
    """Int64 columns whose sorted order has the runs named; rows shuffled."""
    def runs(starts):
        st = np.zeros(n, bool)
        st[[r for r in starts if 0 <= r < n]] = True
        return rng.permutation(np.cumsum(st)).astype(np.int64)

    edges = [e + d for e in (64, B, T, 2 * T, 3 * T) for d in (-1, 1)]
    return {
        "distinct": rng.permutation(n).astype(np.int64),
        "all_equal": np.full(n, 7, np.int64),  # one run across every tile and both carries
        "runs_64": rng.permutation(np.arange(n) // 64).astype(np.int64),
        "runs_B": rng.permutation(np.arange(n) // B).astype(np.int64),
        "runs_T": rng.permutation(np.arange(n) // T).astype(np.int64),
        "straddle": runs(edges),               # runs that straddle every edge by one row
        "three": rng.integers(0, 3, n).astype(np.int64),
    }


def _null_patterns(n, rng):
    """{name: validity array, None for no validity buffer}."""
    def nulls(rows):
        v = np.ones(n, bool)
        v[[r for r in rows if 0 <= r < n]] = False
        return v

    return {
        "none": None,
        "all": np.zeros(n, bool),
        "first_row": nulls([0]),
        "last_row": nulls([n - 1]),
        "random": rng.random(n) >= 0.3,
    }


# ---------------------------------------------------------------------- seams
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_patterns_and_nulls(gpu, n, desc):
    rng = np.random.default_rng(n)
    nulls = _null_patterns(n, rng)
    for vname, vals in _value_patterns(n, rng).items():
        for nname, valid in nulls.items():
            _check_all(_series(vals, valid), vals, valid, desc, (n, vname, nname))


def _direct(order, sorted_valid, tie, seg, valid, method, offs=(0, 0, 0, 0, 0)):
    """plgpu_rank on hand-made inputs, each column at its own offset inside a
    hostile parent: row ids outside the column, inverted bits."""
    n = len(order)

    def place(arr, off, junk):
        if off == 0:
            return arr
        return np.concatenate([np.full(off, junk(arr, True), arr.dtype), arr, np.full(67, junk(arr, False), arr.dtype)])

    inv = lambda a, first: (not bool(a[0] if first else a[-1])) if a.size else True  # noqa: E731
    big = lambda a, first: np.uint32(0xFFFFFFF0)  # noqa: E731
    zeros = np.zeros(n, np.int64)
    o_idx, o_sv, o_tie, o_seg, o_val = offs

    def col(name, arr, off, junk, valid_=None):
        pv = place(arr, off, junk)
        pvalid = None if valid_ is None else place(valid_, off, inv)
        s = pl.Series.from_numpy(name, pv) if pvalid is None else pl.Series.from_numpy(name, pv, pvalid)
        return s.slice(off, n) if off else s

    idx = col("idx", order.astype(np.uint32), o_idx, big)
    sv = col("sv", zeros, o_sv, lambda a, f: np.int64(-1), sorted_valid)
    ties = col("tie", tie, o_tie, inv)
    segs = None if seg is None else col("seg", seg, o_seg, inv)
    vals = col("v", zeros, o_val, lambda a, f: np.int64(-1), valid)
    assert int(idx._col.offset) == o_idx and int(ties._col.offset) == o_tie
    out = N.Column()
    N.check(N.lib().plgpu_rank(C.byref(idx._col), C.byref(sv._col), C.byref(ties._col),
                               None if segs is None else C.byref(segs._col), C.byref(vals._col), N.RANK[method],
                               C.byref(out), None))
    return pl.Series._from_native("x", out)


def _segment_layout(rng):
    """Sorted-layout segment starts over NS rows: on, one before and one after
    the tile and block edges, one segment longer than two tiles, segments of
    one row, and a last segment for the cases below."""
    st = np.zeros(NS, bool)
    rows = [0, 5, 6, 7, 64, B - 1, B, B + 1, 2 * B + 1, T - 1, T, T + 1]   # 5, 6: segments of one row
    rows += [3 * T + 3]                                                       # T + 1 .. 3T + 3: longer than two tiles
    st[[r for r in rows if r < NS]] = True
    return st


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
def test_segments_direct_and_over(gpu, desc):
    """Hand-made start bitmaps through the C entry point, and the same groups
    through over(): an all-null segment between two others, a last segment
    whose only tie run ends at n."""
    rng = np.random.default_rng(11)
    seg_sorted = _segment_layout(rng)
    gid_sorted = np.cumsum(seg_sorted) - 1
    perm = rng.permutation(NS)
    groups = np.empty(NS, np.int64)
    groups[perm] = gid_sorted                      # the groups' rows scattered over the column
    vals = rng.integers(0, 50, NS).astype(np.int64)
    valid = rng.random(NS) >= 0.2
    last = gid_sorted[-1]
    vals[groups == last] = 3                       # one run, and it ends at n
    valid[groups == last] = True
    valid[groups == 3] = False                     # all-null segments between others
    valid[groups == gid_sorted[T + 1]] = True      # the long segment: no nulls, its runs cross two tile edges
    valid[groups == gid_sorted[T - 1]] = False
    order, svalid, tie, seg = sorted_inputs(vals, valid, desc, groups)
    assert np.array_equal(seg, seg_sorted)
    ref = rank_closed_all(vals, valid, desc, groups)
    bare = tie & ~seg                              # a segment start is a tie start whatever the caller says
    bare_seg = seg.copy()
    bare_seg[0] = False                            # and row 0 a segment start
    df = pl.DataFrame([_series(groups, None, "k"), _series(vals, valid, "x")])
    for m in METHODS:
        exp = ref[m][0]
        _check(_direct(order, svalid, tie, seg, valid, m), exp, valid, m, ("direct", m, desc))
        _check(_direct(order, svalid, bare, bare_seg, valid, m), exp, valid, m, ("direct, bare starts", m, desc))
        _check(_direct(order, svalid, tie, seg, valid, m, offs=(3, 1, 5, 7, 9)), exp, valid, m, ("direct, sliced", m))
        _check(_direct(order, svalid, tie, seg, valid, m, offs=(4, 64, 66, 63, 2)), exp, valid, m, ("direct, sliced 2", m))
        out = df.select(pl.col("x").rank(m, descending=desc).over("k"))["x"]
        _check(out, exp, valid, m, ("over", m, desc))
    # no segment column: one segment, and row 0 starts it whatever the tie bitmap says
    order, svalid, tie, _ = sorted_inputs(vals, valid, desc)
    ref = rank_closed_all(vals, valid, desc)
    tie[0] = False
    for m in METHODS:
        _check(_direct(order, svalid, tie, None, valid, m, offs=(1, 0, 3, 0, 0)), ref[m][0], valid, m, ("one segment", m))


@pytest.mark.parametrize("n", [0, 1, 2, 65])
def test_direct_small_and_no_validity(gpu, n):
    rng = np.random.default_rng(n)
    vals = rng.integers(0, 3, n).astype(np.int64)
    ok = np.ones(n, bool)
    order, svalid, tie, seg = sorted_inputs(vals, ok)
    ref = rank_closed_all(vals, ok)
    for m in METHODS:
        got = _direct(order, None, tie, None, None, m)
        _check(got, ref[m][0], ok, m, (n, m), nullable=False)
        assert got.null_count() == 0


# --------------------------------------------------------------------- values
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
def test_floats_nan_zero_and_infinities_tie(gpu, desc):
    rng = np.random.default_rng(5)
    pool = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.25, 1e300, 5e-324])
    n = B + 77
    vals = pool[rng.integers(0, len(pool), n)]
    valid = rng.random(n) >= 0.2
    _check_all(_series(vals, valid), vals, valid, desc, "float pool")
    _check_all(_series(vals, None), vals, None, desc, "float pool, no nulls")
    small = np.array([0.0, np.nan, -0.0, 1.0, np.nan, np.inf])
    got = _series(small, None)._rank("min", desc).to_numpy().tolist()
    assert got == ([5, 1, 5, 4, 1, 3] if desc else [1, 5, 1, 3, 5, 4])
    f32 = vals.astype(np.float32)
    _check_all(_series(f32, valid), f32, valid, desc, "Float32")


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.uint8, np.uint16, np.int32, np.uint32, np.int64, np.bool_])
def test_small_dtypes_and_boolean(gpu, dtype):
    rng = np.random.default_rng(9)
    n = B + 3
    if dtype is np.bool_:
        vals = rng.random(n) >= 0.5
    else:
        ii = np.iinfo(dtype)
        vals = rng.integers(max(ii.min, -300), min(ii.max, 300), n, endpoint=True).astype(dtype)
        vals[:4] = [ii.min, ii.max, ii.min, ii.max]
    valid = rng.random(n) >= 0.25
    for desc in (False, True):
        _check_all(_series(vals, valid), vals.astype(np.int64), valid, desc, (np.dtype(dtype).name,))


def test_temporal_columns_rank_on_their_integers(gpu):
    rng = np.random.default_rng(10)
    n = 300
    valid = rng.random(n) >= 0.2
    days = rng.integers(-50, 50, n).astype(np.int32)
    stamps = rng.integers(-10 ** 15, 10 ** 15, n).astype(np.int64)
    stamps[::7] = stamps[0]
    for vals, dt in ((days, pl.Date), (stamps, pl.Datetime("us")), (stamps, pl.Duration("ns"))):
        s = _series(vals, valid, dtype=dt)
        assert s.dtype == dt
        for desc in (False, True):
            _check_all(s, vals, valid, desc, (str(dt),))
        assert s.rank("dense")._logical_dtype() is None


# --------------------------------------------------------------------- slices
def _sliced(vals, valid, off, name="x"):
    """The column as a slice at `off` of a parent whose other rows are hostile
    (as tests/test_gpu_sliced_inputs.py builds them): extreme values that tie
    with nothing, validity bits the inverse of their neighbour's."""
    n = len(vals)
    if vals.dtype.kind == "f":
        junk = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300])
    else:
        ii = np.iinfo(vals.dtype)
        junk = np.array([ii.max, ii.min, ii.max - 1, ii.min + 1], vals.dtype)
    front, back = junk[np.arange(off) % len(junk)].astype(vals.dtype), junk[np.arange(131) % len(junk)].astype(vals.dtype)
    pv = np.concatenate([front, vals, back])
    pvalid = None
    if valid is not None:
        a, b = (not bool(valid[0]), not bool(valid[-1])) if n else (True, True)
        pvalid = np.concatenate([np.full(off, a), valid, np.full(131, b)])
    s = _series(pv, pvalid, name).slice(off, n)
    assert s.len() == n and int(s._col.offset) == off
    return s


@pytest.mark.parametrize("off", [1, 63, 64, 66])
def test_sliced_column(gpu, off):
    rng = np.random.default_rng(off)
    n = T + 70
    ints = rng.integers(0, 40, n).astype(np.int64)
    floats = rng.integers(0, 40, n).astype(np.float64)
    floats[rng.random(n) < 0.05] = np.nan
    valid = rng.random(n) >= 0.3
    for vals in (ints, floats):
        for v in (valid, None):
            for desc in (False, True):
                _check_all(_sliced(vals, v, off), vals, v, desc, (off, vals.dtype.name, v is None))
    # over(): the key sliced too, at another offset
    keys = rng.integers(0, 9, n).astype(np.int64)
    df = pl.DataFrame([_sliced(keys, None, off + 1, "k"), _sliced(ints, valid, off, "x")])
    ref = rank_closed_all(ints, valid, True, keys)
    for m in METHODS:
        _check(df.select(pl.col("x").rank(m, descending=True).over("k"))["x"], ref[m][0], valid, m, ("over", off, m))


# ----------------------------------------------------------------- end to end
def _frame(n=5000, seed=3):
    rng = np.random.default_rng(seed)
    k1 = rng.integers(0, 12, n).astype(np.int64)           # unsorted keys
    k1v = rng.random(n) >= 0.1                              # with nulls: the nulls are one group
    k2 = rng.integers(0, 3, n).astype(np.int32)
    x = rng.integers(0, 30, n).astype(np.int64)
    xv = rng.random(n) >= 0.2
    f = rng.normal(0, 1, n).round(1)
    host = dict(k1=k1, k1v=k1v, k2=k2, x=x, xv=xv, f=f)
    df = pl.DataFrame([_series(k1, k1v, "k1"), _series(k2, None, "k2"), _series(x, xv, "x"), _series(f, None, "f")])
    return df, host


def _gid(*cols):
    """One group id per row from (values, validity) key columns; nulls are a group."""
    keys = [np.where(v, c.astype(np.int64), np.int64(-10 ** 9)) for c, v in cols]
    return np.unique(np.stack(keys, 1), axis=0, return_inverse=True)[1].reshape(-1)


def test_series_select_with_columns_eager_and_lazy(gpu):
    df, h = _frame()
    n = len(h["x"])
    ref = rank_closed_all(h["x"], h["xv"], False)
    refd = rank_closed_all(h["x"], h["xv"], True)
    _check(df["x"].rank(), ref["average"][0], h["xv"], "average", "Series.rank default")
    _check(df["x"].rank("dense", descending=True), refd["dense"][0], h["xv"], "dense", "Series.rank")
    out = df.select(pl.col("x").rank("min").alias("r"), pl.col("x").rank("max", descending=True))
    assert out.columns == ["r", "x"]
    _check(out["r"], ref["min"][0], h["xv"], "min", "select")
    _check(out["x"], refd["max"][0], h["xv"], "max", "select")
    out = df.lazy().with_columns(pl.col("x").rank("ordinal").alias("r")).collect()
    assert out.columns == ["k1", "k2", "x", "f", "r"] and out.height == n
    _check(out["r"], ref["ordinal"][0], h["xv"], "ordinal", "lazy with_columns")
    out = df.lazy().select((pl.col("f") * 2).rank("dense").alias("r")).collect()
    _check(out["r"], rank_closed_all(h["f"] * 2, np.ones(n, bool))["dense"][0], np.ones(n, bool), "dense",
           "rank of an expression")
    out = df.with_columns(pl.col("f").rank().alias("r"))
    _check(out["r"], rank_closed_all(h["f"], np.ones(n, bool))["average"][0], np.ones(n, bool), "average",
           "eager with_columns", nullable=False)


def test_over_one_and_two_keys(gpu):
    df, h = _frame()
    ones = np.ones(len(h["x"]), bool)
    g1 = _gid((h["k1"], h["k1v"]))
    g2 = _gid((h["k1"], h["k1v"]), (h["k2"], ones))
    for desc in (False, True):
        r1, r2 = rank_closed_all(h["x"], h["xv"], desc, g1), rank_closed_all(h["x"], h["xv"], desc, g2)
        for m in METHODS:
            out = df.select(pl.col("x").rank(m, descending=desc).over("k1").alias("a"),
                            pl.col("x").rank(m, descending=desc).over("k1", "k2").alias("b"))
            _check(out["a"], r1[m][0], h["xv"], m, ("over k1", m, desc))
            _check(out["b"], r2[m][0], h["xv"], m, ("over k1, k2", m, desc))
    # two rank().over() on the same keys in one select, lazily
    out = df.lazy().select(pl.col("x").rank("dense", descending=True).over("k1").alias("a"),
                           pl.col("f").rank("ordinal").over("k1").alias("b")).collect()
    _check(out["a"], rank_closed_all(h["x"], h["xv"], True, g1)["dense"][0], h["xv"], "dense", "two overs, a")
    _check(out["b"], rank_closed_all(h["f"], ones, False, g1)["ordinal"][0], ones, "ordinal", "two overs, b",
           nullable=False)


def test_over_categorical_key(gpu):
    import pyarrow as pa

    rng = np.random.default_rng(4)
    n = 3000
    code = rng.integers(0, 5, n)
    names = np.array(["aa", "b", "cccc", "d", "ee"])[code].tolist()
    x = rng.integers(0, 20, n).astype(np.int64)
    xv = rng.random(n) >= 0.2
    df = pl.DataFrame([pl.Series.from_arrow("c", pa.array(names, pa.string()).dictionary_encode()),
                       _series(x, xv, "x")])
    assert df["c"]._cat_codes() is not None
    ref = rank_closed_all(x, xv, False, code)
    for m in METHODS:
        _check(df.with_columns(pl.col("x").rank(m).over("c").alias("r"))["r"], ref[m][0], xv, m, ("categorical", m))


def test_rank_below_the_top_of_an_expression(gpu):
    df, h = _frame(2048)  # (a power of two: rank / n is exact however the division is lowered)
    n = len(h["x"])
    r = rank_closed_all(h["x"], h["xv"], True)["ordinal"][0]
    out = df.select((pl.col("x").rank("ordinal", descending=True) <= 3).alias("top3"))["top3"]
    assert out.dtype is pl.Boolean
    assert np.array_equal(out.validity_numpy(), h["xv"])
    assert np.array_equal(out.to_numpy()[h["xv"]].astype(bool), (r <= 3)[h["xv"]])
    assert int(out.to_numpy()[h["xv"]].astype(bool).sum()) == 3
    g1 = _gid((h["k1"], h["k1v"]))
    rg = rank_closed_all(h["x"], h["xv"], False, g1)["min"][0]
    out = df.select((pl.col("x").rank("min").over("k1") * 2 + 1).alias("y"))["y"]
    assert np.array_equal(out.validity_numpy(), h["xv"])
    assert np.array_equal(out.to_numpy()[h["xv"]].astype(np.int64), (rg.astype(np.int64) * 2 + 1)[h["xv"]])
    pct = df.select((pl.col("f").rank() / n).alias("p"))["p"].to_numpy()
    assert np.array_equal(pct, rank_closed_all(h["f"], np.ones(n, bool))["average"][0] / n)


@pytest.mark.parametrize("case", load_golden("rank_cases.json")["cases"], ids=lambda c: c["name"])
def test_golden_cases(gpu, case):
    vals, valid, _, _ = case_inputs(case)
    s = _series(vals, valid if not valid.all() or not len(valid) else None, "value")  # (no key has this name)
    e = pl.col("value").rank(case["method"], descending=case["descending"])
    cols = [s]
    if "keys" in case:
        (kname, key), = case["keys"].items()
        cols.append(pl.Series(kname, key, dtype=pl.Int64))
        e = e.over(kname)
    else:
        got = s.rank(case["method"], descending=case["descending"])
        check_case(case, got.to_numpy(), got.validity_numpy(), "Series.rank")
    out = pl.DataFrame(cols).select(e)["value"]
    assert out.dtype is getattr(pl, case["expected_dtype"])
    check_case(case, out.to_numpy(), out.validity_numpy(), "select")
    assert out.to_list() == case["expected"]


# ------------------------------------------------------------- the large case
N_BIG = (N.CUM_TOTALS_THREADS + 3) * T   # the totals launch folds more than one tile per thread


@functools.lru_cache(maxsize=1)
def _big():
    """Runs and segments at random, generated in the sorted layout (no host
    sort): a segment longer than many tiles, a run longer than many tiles, and
    whole last runs of some segments null."""
    rng = np.random.default_rng(2024)
    n = N_BIG
    seg = rng.random(n) < 1e-4
    seg[0] = True
    seg[5 * T + 3:40 * T + 11] = False            # one segment across 35 tiles
    tie = (rng.random(n) < 0.3) | seg
    tie[50 * T + 1:90 * T - 1] = False            # one run across 40 tiles (no segment start inside it)
    seg[50 * T + 1:90 * T - 1] = False
    starts = np.flatnonzero(tie)
    run = np.cumsum(tie) - 1
    nxt = np.append(starts[1:], n)
    last_run = np.append(seg, True)[nxt]          # the run ends its segment
    null_run = last_run & (rng.random(starts.size) < 0.3) & ~seg[starts]   # (never a segment's only run... or all of it)
    svalid = ~null_run[run]
    order = rng.permutation(n).astype(np.uint32)
    valid = np.empty(n, bool)
    valid[order] = svalid
    cols = (pl.Series.from_numpy("idx", order), pl.Series.from_numpy("sv", np.zeros(n, np.int8), svalid),
            pl.Series.from_numpy("tie", tie), pl.Series.from_numpy("seg", seg),
            pl.Series.from_numpy("v", np.zeros(n, np.int8), valid))
    return order.astype(np.int64), svalid, tie, seg, valid, cols


@pytest.mark.parametrize("method", METHODS)
def test_many_tiles_per_totals_thread(gpu, method):
    order, svalid, tie, seg, valid, (c_idx, c_sv, c_tie, c_seg, c_v) = _big()
    assert len(order) // T > N.CUM_TOTALS_THREADS
    out = N.Column()
    N.check(N.lib().plgpu_rank(C.byref(c_idx._col), C.byref(c_sv._col), C.byref(c_tie._col), C.byref(c_seg._col),
                               C.byref(c_v._col), N.RANK[method], C.byref(out), None))
    got = pl.Series._from_native("x", out)
    exp = ranks_from_starts(order, svalid, tie, seg, (method,))[method]
    _check(got, exp, valid, method, ("big", method))
