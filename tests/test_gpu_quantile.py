"""GPU: median / quantile (plgpu_segment_quantile) at the seams of its four
launches -- word, block and tile edges of the bitmaps, the ballot word and the
workgroup edge of the per-segment launch, more tiles than the totals launch has
threads -- its methods, dtypes, null patterns and sliced inputs, and end to
end: Series, select, group_by().agg(), over() and the shorthands.

Reference.  tests/quantile_ref.py: the reference's generic_quantile restated
(quantile_ref, used on short inputs) and its numpy closed form
(quantile_closed); tests/test_quantile.py pins the two to each other and to the
reference's own cases.  The arithmetic is the reference's own, so every
comparison is exact: the same validity bits, values equal under == (NaN where
the reference is NaN), the dtype, and a null row's bytes zero."""

import ctypes as C
import functools

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from polaroid_amd import _native as N
from quantile_ref import METHODS, quantile_closed, quantile_ref, segment_bounds, sorted_layout
from test_quantile import case_inputs

pytestmark = pytest.mark.gpu

T = N.CUM_TILE    # rows of one workgroup of the bitmap launches: one count, one first ordinal each
B = N.CUM_BLOCK
NS = 3 * T + 5
LENGTHS = [0, 1, 2, 63, 64, 65, B - 1, B, B + 1, T - 1, T, T + 1, NS]
QS = [0.0, 0.24, 0.5, 0.9, 1.0]
PAIRS = [(q, m) for m in METHODS for q in QS]      # 30 pairs: calls of 8, 8, 8 and 6
# one call of 8 with every method and every q, for the lengths of several tiles
PAIRS8 = [(0.0, "nearest"), (0.24, "higher"), (0.5, "lower"), (0.9, "midpoint"), (1.0, "linear"),
          (0.24, "equiprobable"), (0.5, "nearest"), (0.24, "linear")]


def _series(vals, valid, name="x", **kw):
    return pl.Series.from_numpy(name, vals, **kw) if valid is None else pl.Series.from_numpy(name, vals, valid, **kw)


def _junk(dtype):
    if np.dtype(dtype).kind == "f":
        return np.array([np.nan, np.inf, -np.inf, 1e300, -1e300], dtype)
    if np.dtype(dtype).kind == "b":
        return None
    ii = np.iinfo(dtype)
    return np.array([ii.max, ii.min, ii.max - 1, ii.min + 1], dtype)


def _sliced(vals, valid, off, name="x"):
    """The column as a slice at `off` of a parent whose other rows are hostile
    (as tests/test_gpu_sliced_inputs.py builds them): extreme values, validity
    and Boolean bits the inverse of their neighbour's."""
    n = len(vals)
    if off == 0:
        return _series(vals, valid, name)
    if vals.dtype == np.bool_:
        a, b = (not bool(vals[0]), not bool(vals[-1])) if n else (True, True)
        pv = np.concatenate([np.full(off, a), vals, np.full(131, b)])
    else:
        junk = _junk(vals.dtype)
        pv = np.concatenate([junk[np.arange(off) % len(junk)], vals, junk[np.arange(131) % len(junk)]]).astype(vals.dtype)
    pvalid = None
    if valid is not None:
        a, b = (not bool(valid[0]), not bool(valid[-1])) if n else (True, True)
        pvalid = np.concatenate([np.full(off, a), valid, np.full(131, b)])
    s = _series(pv, pvalid, name).slice(off, n)
    assert s.len() == n and int(s._col.offset) == off
    return s


def _call(sv, seg, pairs):
    """plgpu_segment_quantile on device columns; `seg` None: one segment."""
    nq = len(pairs)
    outs = (N.Column * nq)()
    N.check(N.lib().plgpu_segment_quantile(
        C.byref(sv._col), None if seg is None else C.byref(seg._col), (C.c_double * nq)(*[q for q, _ in pairs]),
        (C.c_int32 * nq)(*[N.QUANTILE[m] for _, m in pairs]), nq, outs, None))
    return [pl.Series._from_native("x", outs[i]) for i in range(nq)]


def _direct(vals, valid, seg, pairs, offs=(0, 0)):
    """The entry point on a hand-made sorted layout (no sort involved), each
    column at its own offset inside a hostile parent."""
    sv = _sliced(vals, valid, offs[0], "sv")
    sg = None if seg is None else _sliced(np.asarray(seg, bool), None, offs[1], "seg")
    out = []
    for at in range(0, len(pairs), N.QUANTILE_MAX):
        out += _call(sv, sg, pairs[at:at + N.QUANTILE_MAX])
    return out


def _check(got, exp, ok, what, nullable=None, dtype=pl.Float64):
    gv, gok = got.to_numpy(), got.validity_numpy()
    assert got.dtype is dtype, what
    assert gv.dtype == dtype.np_dtype and gv.shape == ok.shape, (what, gv.shape, ok.shape)
    assert np.array_equal(gok, ok), (what, np.flatnonzero(gok != ok)[:8])
    if nullable is not None and len(ok):
        assert bool(got._col.validity) == nullable, what
    exp = np.asarray(exp, gv.dtype)
    bad = np.flatnonzero(ok & ~((gv == exp) | (np.isnan(gv) & np.isnan(exp))))
    assert bad.size == 0, (what, bad[:8], gv[bad[:8]], exp[bad[:8]])
    raw = gv.view(np.uint64 if gv.dtype == np.float64 else np.uint32)
    assert not raw[~ok].any(), (what, "a null row's bytes are not zero")


def _check_pairs(vals, valid, seg, pairs, what, offs=(0, 0), literal=False):
    got = _direct(vals, valid, seg, pairs, offs)
    for (q, m), g in zip(pairs, got):
        exp, ok = quantile_closed(vals, valid, seg, q, m)
        if literal:
            e2, ok2 = quantile_ref(vals, valid, seg, q, m)
            assert np.array_equal(ok, ok2) and np.array_equal(exp, e2, equal_nan=True)
        _check(g, exp, ok, (what, q, m), nullable=not ok.all())


def _fill_segments(seg, n, rng, nn_of, dtype=np.int64, pool=None):
    """Values ascending within every segment (TotalOrd), its last len - nn rows
    null and holding junk; nn_of(start, end) is the segment's non-null count."""
    starts, ends = segment_bounds(n, seg)
    if pool is None:
        vals = rng.integers(-1000, 1000, n).astype(dtype)
    else:
        vals = pool[rng.integers(0, len(pool), n)]
    gid = np.repeat(np.arange(len(starts)), ends - starts)
    valid = np.ones(n, bool)
    for s, e in zip(starts.tolist(), ends.tolist()):
        valid[s + max(0, min(e - s, int(nn_of(s, e)))):e] = False
    sv, sok, sseg = sorted_layout(vals, valid, gid)
    junk = _junk(sv.dtype)
    sv = sv.copy()
    sv[~sok] = junk[np.arange(int((~sok).sum())) % len(junk)]
    return sv, sok


def _layouts(n, rng):
    """{name: segment starts, None for no column}."""
    def at(rows):
        st = np.zeros(n, bool)
        st[[r for r in rows if 0 <= r < n]] = True
        return st

    near = [e + d for e in (64, B, T) for d in (-1, 0, 1)]
    return {
        "one": None,
        "one_bare": np.zeros(n, bool),            # row 0 starts a segment whatever its bit says
        "each": np.ones(n, bool),                 # G = n
        # segments of 1 and 2 rows next to long ones, starts around the edges, T + 1 .. 3T + 3 longer than two tiles
        "edges": at([0, 1, 3, 4] + near + [2 * B + 1, 3 * T + 3]),
        "edges2": at([0] + [e + d for e in (128, 2 * B, 2 * T, 3 * T) for d in (-1, 0, 1)]),
        "random": rng.random(n) < 0.05,
    }


def _null_patterns(n, seg, rng):
    """{name: nn_of(start, end), None for no validity buffer}."""
    starts, _ = segment_bounds(n, seg)
    order = {int(s): g for g, s in enumerate(starts.tolist())}

    def word_edge(s, e):  # the null run begins exactly on a word edge, where the segment holds one
        w = (s // 64 + 1) * 64
        return w - s if w < e else e - s

    return {
        "none": None,
        "one_value": lambda s, e: 1,
        # an all-null segment between two others, and as the last one
        "some_empty": lambda s, e: 0 if order[s] % 3 == 1 or order[s] == len(starts) - 1 else rng.integers(1, e - s + 1),
        "all_null": lambda s, e: 0,
        "word_edge": word_edge,
        "random": lambda s, e: rng.integers(0, e - s + 1),
    }


# ---------------------------------------------------------------------- seams
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_layouts_and_nulls(gpu, n):
    rng = np.random.default_rng(n)
    for lname, seg in _layouts(n, rng).items():
        for nname, nn_of in _null_patterns(n, seg, rng).items():
            if nn_of is None:
                vals, valid = _fill_segments(seg, n, rng, lambda s, e: e - s)[0], None
            else:
                vals, valid = _fill_segments(seg, n, rng, nn_of)
            _check_pairs(vals, valid, seg, PAIRS if n <= B + 1 else PAIRS8, (n, lname, nname), literal=n <= 130)


def test_empty_columns(gpu):
    empty = np.zeros(0, np.int64)
    for pairs in ([(0.5, "linear")], PAIRS[:3]):
        for g in _direct(empty, None, None, pairs):              # the plain reduction: one null row
            _check(g, np.zeros(1), np.zeros(1, bool), "empty, one segment", nullable=True)
        for g in _direct(empty, None, np.zeros(0, bool), pairs):  # no segments
            _check(g, np.zeros(0), np.zeros(0, bool), "empty, no segments")
            assert g.len() == 0


@pytest.mark.parametrize("groups", [1, 63, 64, 65, 255, 256, 257])
def test_group_counts(gpu, groups):
    """The ballot word and the workgroup edge of the per-segment launch."""
    rng = np.random.default_rng(groups)
    lens = rng.integers(1, 6, groups)
    n = int(lens.sum())
    seg = np.zeros(n, bool)
    seg[np.concatenate([[0], np.cumsum(lens)[:-1]])] = True
    for nname, nn_of in _null_patterns(n, seg, rng).items():
        if nn_of is None:
            vals, valid = _fill_segments(seg, n, rng, lambda s, e: e - s)[0], None
        else:
            vals, valid = _fill_segments(seg, n, rng, nn_of)
        _check_pairs(vals, valid, seg, PAIRS, (groups, nname), literal=True)
    # a validity buffer on the input, no segment empty: the outputs carry none
    vals, valid = _fill_segments(seg, n, rng, lambda s, e: max(1, e - s - 1))
    for g in _direct(vals, valid, seg, PAIRS[:8]):
        assert g.len() == groups and not g._col.validity and g.null_count() == 0


def test_one_call_of_three_equals_three_calls(gpu):
    rng = np.random.default_rng(3)
    n = B + 77
    seg = rng.random(n) < 0.02
    vals, valid = _fill_segments(seg, n, rng, lambda s, e: rng.integers(0, e - s + 1))
    pairs = [(0.25, "linear"), (0.5, "nearest"), (0.75, "midpoint")]
    sv, sg = _series(vals, valid), _series(seg, None)
    three = _call(sv, sg, pairs)
    for p, a in zip(pairs, three):
        (b,) = _call(sv, sg, [p])
        assert np.array_equal(a.validity_numpy(), b.validity_numpy())
        assert np.array_equal(a.to_numpy().view(np.uint64), b.to_numpy().view(np.uint64)), p
    eight = _call(sv, sg, pairs + [(0.0, "equiprobable"), (1.0, "higher"), (0.9, "lower"), (0.5, "linear"), (0.24, "nearest")])
    assert len(eight) == 8
    for a, b in zip(three, eight):
        assert np.array_equal(a.to_numpy().view(np.uint64), b.to_numpy().view(np.uint64))


# --------------------------------------------------------------------- values
@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64])
def test_integer_dtypes_and_extremes(gpu, dtype):
    rng = np.random.default_rng(7)
    n = B + 3
    seg = rng.random(n) < 0.03
    ii = np.iinfo(dtype)
    pool = np.concatenate([np.array([ii.min, ii.max, ii.min + 1, ii.max - 1, 0, 1], dtype),
                           rng.integers(ii.min, ii.max, 40, dtype=dtype, endpoint=True)])
    if dtype is np.int64:   # above 2^53 a neighbour rounds to the same double
        pool = np.concatenate([pool, np.array([2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, -(2 ** 53) - 1, 2 ** 62 + 1], dtype)])
    for valid_of in (None, lambda s, e: rng.integers(0, e - s + 1)):
        vals, valid = _fill_segments(seg, n, rng, valid_of or (lambda s, e: e - s), dtype, pool)
        _check_pairs(vals, None if valid_of is None else valid, seg, PAIRS, (np.dtype(dtype).name, valid_of is None))
        vals, valid = _fill_segments(None, n, rng, valid_of or (lambda s, e: e - s), dtype, pool)
        _check_pairs(vals, None if valid_of is None else valid, None, PAIRS, (np.dtype(dtype).name, "one segment"))


def test_floats_nan_zero_and_infinities(gpu):
    """NaN is the greatest value and a value; -inf / inf neighbours give NaN
    under midpoint and linear; lower == upper is the IEEE comparison."""
    rng = np.random.default_rng(5)
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.25, 1e300, 5e-324])
    n = B + 77
    seg = rng.random(n) < 0.1
    for valid_of in (None, lambda s, e: rng.integers(0, e - s + 1)):
        vals, valid = _fill_segments(seg, n, rng, valid_of or (lambda s, e: e - s), np.float64, pool)
        _check_pairs(vals, None if valid_of is None else valid, seg, PAIRS, ("float pool", valid_of is None))
    two = np.array([-np.inf, np.inf])
    for m in ("midpoint", "linear"):
        (g,) = _direct(two, None, None, [(0.5, m)])
        assert np.isnan(g.to_numpy()[0]) and g.null_count() == 0
    (g,) = _direct(np.array([1.0, np.nan]), None, None, [(1.0, "nearest")])
    assert np.isnan(g.to_numpy()[0])
    (g,) = _direct(np.array([-0.0, 0.0]), None, None, [(0.5, "linear")])
    assert g.to_numpy()[0] == 0.0


# --------------------------------------------------------------------- slices
@pytest.mark.parametrize("off", [1, 63, 64, 66])
def test_sliced_inputs(gpu, off):
    rng = np.random.default_rng(off)
    n = T + 70
    seg = rng.random(n) < 0.01
    seg[[63, 64, 65]] = True
    pool = np.array([np.nan, np.inf, -np.inf, 0.0, 1.5, -2.25, 7.0])
    for dtype, pl_ in ((np.int64, None), (np.float64, pool), (np.int32, None)):
        for nn_of in (None, lambda s, e: rng.integers(0, e - s + 1)):
            vals, valid = _fill_segments(seg, n, rng, nn_of or (lambda s, e: e - s), dtype, pl_)
            valid = None if nn_of is None else valid
            for offs in ((off, 0), (0, off), (off, off + 1)):
                _check_pairs(vals, valid, seg, PAIRS[::4], (off, np.dtype(dtype).name, nn_of is None, offs), offs)
            vals, valid = _fill_segments(None, n, rng, nn_of or (lambda s, e: e - s), dtype, pl_)
            _check_pairs(vals, None if nn_of is None else valid, None, PAIRS[::4], (off, "one segment"), (off, 0))


# ------------------------------------------------------------ argument checks
def test_argument_checks(gpu):
    vals = _series(np.arange(10, dtype=np.int64), None)
    seg = _series(np.zeros(10, bool), None)

    def rc(sv, sg, qs, ms, nq=None):
        nq = len(qs) if nq is None else nq
        k = max(1, len(qs))
        outs = (N.Column * 9)()
        return N.lib().plgpu_segment_quantile(C.byref(sv._col), None if sg is None else C.byref(sg._col),
                                              (C.c_double * k)(*qs), (C.c_int32 * k)(*ms), nq, outs, None)

    (ok,) = _call(vals, seg, [(0.5, "linear")])          # the same arguments, accepted
    assert ok.to_list() == [4.5]
    assert rc(vals, seg, [], [], 0) == N.ERR_INVALID
    assert rc(vals, seg, [0.5] * 9, [5] * 9) == N.ERR_INVALID
    assert b"between 1 and 8" in N.lib().plgpu_last_error()
    for q in (1.5, -0.01, float("nan")):
        assert rc(vals, seg, [0.5, q], [5, 5]) == N.ERR_INVALID
        assert b"should be between 0.0 and 1.0" in N.lib().plgpu_last_error()
    for m in (0, 7, -1):
        assert rc(vals, None, [0.5], [m]) == N.ERR_INVALID
        assert b"unknown quantile method" in N.lib().plgpu_last_error()
    assert rc(seg, None, [0.5], [5]) == N.ERR_INVALID                       # Boolean values
    assert rc(_series(np.arange(10, dtype=np.float32), None), None, [0.5], [5]) == N.ERR_INVALID
    assert rc(vals, _series(np.zeros(9, bool), None), [0.5], [5]) == N.ERR_INVALID
    assert b"equal lengths" in N.lib().plgpu_last_error()
    nullable = _series(np.zeros(10, bool), np.arange(10) != 3)
    assert nullable._col.validity and rc(vals, nullable, [0.5], [5]) == N.ERR_INVALID
    assert rc(vals, vals, [0.5], [5]) == N.ERR_INVALID                      # starts that are not Boolean
    assert b"null-free Boolean" in N.lib().plgpu_last_error()


# ------------------------------------------------------------- the large case
N_BIG = (N.CUM_TOTALS_THREADS + 3) * T   # the totals launch folds more than one tile per thread


@functools.lru_cache(maxsize=1)
def _big():
    """Generated in the sorted layout (no host sort): values ascending over the
    whole column, so ascending in every segment; segments at random, one across
    35 tiles; the tails of some segments, and all of some, null."""
    rng = np.random.default_rng(2024)
    n = N_BIG
    seg = rng.random(n) < 1e-3
    seg[0] = True
    seg[5 * T + 3:40 * T + 11] = False
    vals = np.cumsum(rng.integers(0, 3, n, dtype=np.int32), dtype=np.int32)
    starts, ends = segment_bounds(n, seg)
    nn = np.minimum((rng.random(len(starts)) * 1.3 * (ends - starts + 1)).astype(np.int64), ends - starts)
    nn[rng.random(len(starts)) < 0.1] = 0
    nn[-1] = 0
    first_null = starts + nn
    valid = np.arange(n) < np.repeat(first_null, ends - starts)
    vals[~valid] = np.iinfo(np.int32).min
    return vals, valid, seg, _series(vals, valid), _series(seg, None)


def test_many_tiles_per_totals_thread(gpu):
    vals, valid, seg, c_vals, c_seg = _big()
    assert len(vals) // T > N.CUM_TOTALS_THREADS
    pairs = [(0.5, "linear"), (0.24, "nearest"), (0.9, "higher"), (0.0, "lower"), (1.0, "midpoint"),
             (0.5, "equiprobable"), (0.24, "linear"), (0.9, "midpoint")]
    got = _call(c_vals, c_seg, pairs)
    for (q, m), g in zip(pairs, got):
        exp, ok = quantile_closed(vals, valid, seg, q, m)
        _check(g, exp, ok, ("big", q, m), nullable=True)


# ----------------------------------------------------------------- end to end
def _frame(n=5000, seed=3):
    rng = np.random.default_rng(seed)
    k1 = rng.integers(0, 12, n).astype(np.int64)           # unsorted keys
    k1v = rng.random(n) >= 0.1                              # with nulls: the nulls are one group
    k2 = rng.integers(0, 3, n).astype(np.int32)
    x = rng.integers(0, 30, n).astype(np.int64)
    xv = rng.random(n) >= 0.2
    f = rng.normal(0, 1, n).round(1)
    fv = rng.random(n) >= 0.1
    xv[k1 == 7] = False                                     # a group without a value of x
    host = dict(k1=k1, k1v=k1v, k2=k2, x=x, xv=xv, f=f, fv=fv, ones=np.ones(n, bool))
    df = pl.DataFrame([_series(k1, k1v, "k1"), _series(k2, None, "k2"), _series(x, xv, "x"), _series(f, fv, "f")])
    return df, host


def _gid(*cols):
    """One group id per row from (values, validity) key columns, numbered by
    first occurrence (the group-by's maintain_order=True order); nulls are a group."""
    first: dict = {}
    rows = zip(*[[v if ok else None for v, ok in zip(c.tolist(), okc.tolist())] for c, okc in cols])
    return np.array([first.setdefault(r, len(first)) for r in rows], np.int64)


def _ref(vals, valid, gid, q, method):
    sv, sok, seg = sorted_layout(vals, valid, gid)
    return quantile_closed(sv, sok, seg, q, method)


def _same_keys(out, base, names):
    for nm in names:
        assert np.array_equal(out[nm].validity_numpy(), base[nm].validity_numpy()), nm
        assert out[nm].to_list() == base[nm].to_list(), nm


def test_series_and_select(gpu):
    df, h = _frame()
    exp, ok = _ref(h["x"], h["xv"], None, 0.5, "linear")
    assert df["x"].median() == exp[0] and isinstance(df["x"].median(), float)
    for q, m in PAIRS:
        exp, ok = _ref(h["f"], h["fv"], None, q, m)
        assert df["f"].quantile(q, m) == exp[0], (q, m)
    assert df["x"].quantile(0.25) == _ref(h["x"], h["xv"], None, 0.25, "nearest")[0][0]
    assert _series(np.zeros(4, np.int64), np.zeros(4, bool)).median() is None
    assert _series(np.zeros(0, np.float64), None).quantile(0.5) is None
    out = df.select(pl.col("x").quantile(0.25, "linear").alias("q1"), pl.col("x").median().alias("q2"),
                    pl.col("x").quantile(0.75, "linear").alias("q3"), pl.col("x").sum().alias("s"), pl.len(),
                    pl.median("f"), pl.quantile("k2", 0.9, "higher"))
    assert out.columns == ["q1", "q2", "q3", "s", "len", "f", "k2"] and out.height == 1
    for nm, c, q, m in (("q1", "x", 0.25, "linear"), ("q2", "x", 0.5, "linear"), ("q3", "x", 0.75, "linear"),
                        ("f", "f", 0.5, "linear")):
        exp, ok = _ref(h[c], h[c + "v"], None, q, m)
        _check(out[nm], exp, ok, nm, nullable=False)
    _check(out["k2"], *_ref(h["k2"], h["ones"], None, 0.9, "higher"), "k2")
    assert out["s"].to_list() == [int(h["x"][h["xv"]].sum())] and out["len"].to_list() == [len(h["x"])]
    # a filter below applies
    keep = h["k2"] > 0
    out = df.lazy().filter(pl.col("k2") > 0).select(pl.col("x").median(), pl.col("f").quantile(0.9, "midpoint"),
                                                    pl.col("x").count().alias("n")).collect()
    _check(out["x"], *_ref(h["x"][keep], h["xv"][keep], None, 0.5, "linear"), "filtered median")
    _check(out["f"], *_ref(h["f"][keep], h["fv"][keep], None, 0.9, "midpoint"), "filtered quantile")
    assert out["n"].to_list() == [int((keep & h["xv"]).sum())]


def test_group_by_keys_order_and_mixes(gpu):
    df, h = _frame()
    g1 = _gid((h["k1"], h["k1v"]))
    g2 = _gid((h["k1"], h["k1v"]), (h["k2"], h["ones"]))
    for keys, gid in ((["k1"], g1), (["k1", "k2"], g2), (["k2"], _gid((h["k2"], h["ones"])))):
        base = df.group_by(keys, maintain_order=True).agg(pl.len())
        aggs = [pl.col("x").median().alias("med"), pl.col("x").quantile(0.24, "nearest").alias("qn"),
                pl.col("f").quantile(0.9, "linear").alias("fl"), pl.col("f").mean().alias("fm"),
                pl.col("f").std().alias("fs"), pl.len()]
        for lazy in (False, True):
            info: dict = {}
            if lazy:
                out = df.lazy().group_by(keys, maintain_order=True).agg(aggs).collect(info=info)
                assert info["quantile_sorts"] == 2
            else:
                out = df.group_by(keys, maintain_order=True).agg(aggs)
            assert out.columns == keys + ["med", "qn", "fl", "fm", "fs", "len"]
            _same_keys(out, base, keys)                 # the rows and the row order of the existing group-by
            assert out["len"].to_list() == base["len"].to_list()
            _check(out["med"], *_ref(h["x"], h["xv"], gid, 0.5, "linear"), (keys, "med"))
            _check(out["qn"], *_ref(h["x"], h["xv"], gid, 0.24, "nearest"), (keys, "qn"))
            _check(out["fl"], *_ref(h["f"], h["fv"], gid, 0.9, "linear"), (keys, "fl"))
            plain = df.group_by(keys, maintain_order=True).agg(pl.col("f").mean().alias("fm"), pl.col("f").std().alias("fs"),
                                                               pl.len())
            assert out["fm"].to_list() == plain["fm"].to_list() and out["fs"].to_list() == plain["fs"].to_list()
        if keys == ["k1"]:
            assert not out["med"].validity_numpy().all()   # the group without a value is null
    # maintain_order=False: any order, the same for every column
    out = df.group_by("k1").agg(pl.col("x").median().alias("med"), pl.col("x").count().alias("n"))
    exp, ok = _ref(h["x"], h["xv"], g1, 0.5, "linear")
    base = df.group_by("k1", maintain_order=True).agg(pl.col("x").count().alias("n"))
    want = {k: (e if o else None, c) for k, e, o, c in zip(base["k1"].to_list(), exp.tolist(), ok.tolist(), base["n"].to_list())}
    got = {k: (m, c) for k, m, c in zip(out["k1"].to_list(), out["med"].to_list(), out["n"].to_list())}
    assert got == want


def test_quantiles_of_one_input_share_one_sort(gpu):
    df, h = _frame()
    g1 = _gid((h["k1"], h["k1v"]))
    info: dict = {}
    out = df.lazy().group_by("k1", maintain_order=True).agg(
        pl.col("x").quantile(0.25, "linear").alias("a"), pl.col("x").median().alias("b"),
        pl.col("x").quantile(0.75, "linear").alias("c")).collect(info=info)
    assert info["quantile_sorts"] == 1
    for nm, q in (("a", 0.25), ("b", 0.5), ("c", 0.75)):
        _check(out[nm], *_ref(h["x"], h["xv"], g1, q, "linear"), nm)
    info = {}
    df.lazy().group_by("k1").agg(pl.col("x").median().alias("a"), pl.col("f").median().alias("b"),
                                 pl.col("x").quantile(0.1).alias("c")).collect(info=info)
    assert info["quantile_sorts"] == 2
    info = {}
    df.lazy().select(pl.col("x").median().alias("a"), pl.col("x").quantile(0.9).alias("b")).collect(info=info)
    assert info["quantile_sorts"] == 1
    # a quantile of an expression
    info = {}
    out = df.lazy().group_by("k1", maintain_order=True).agg(
        (pl.col("x") * 2).median().alias("m"), (pl.col("x") * 2).quantile(0.9, "higher").alias("q")).collect(info=info)
    assert info["quantile_sorts"] == 1
    _check(out["m"], *_ref(h["x"] * 2, h["xv"], g1, 0.5, "linear"), "expression median")
    _check(out["q"], *_ref(h["x"] * 2, h["xv"], g1, 0.9, "higher"), "expression quantile")


def test_string_and_categorical_keys(gpu):
    import pyarrow as pa

    rng = np.random.default_rng(4)
    n = 3000
    code = rng.integers(0, 5, n)
    names = np.array(["aa", "b", "a key longer than seven bytes", "d", "ee"])[code]
    kv = rng.random(n) >= 0.1
    x = rng.integers(0, 20, n).astype(np.int64)
    xv = rng.random(n) >= 0.2
    gid = _gid((code, kv))
    strings = [s if ok else None for s, ok in zip(names.tolist(), kv.tolist())]
    for key in (pl.Series.from_arrow("c", pa.array(strings, pa.large_string())),
                pl.Series.from_arrow("c", pa.array(strings, pa.string()).dictionary_encode())):
        df = pl.DataFrame([key, _series(x, xv, "x")])
        base = df.group_by("c", maintain_order=True).agg(pl.len())
        out = df.group_by("c", maintain_order=True).agg(pl.col("x").median().alias("m"),
                                                         pl.col("x").quantile(0.9, "lower").alias("q"))
        assert out["c"].to_list() == base["c"].to_list() and out["c"].dtype == base["c"].dtype
        _check(out["m"], *_ref(x, xv, gid, 0.5, "linear"), "string key median")
        _check(out["q"], *_ref(x, xv, gid, 0.9, "lower"), "string key quantile")
    exp, ok = _ref(x, xv, gid, 0.5, "linear")       # the Categorical key, over()
    got = df.with_columns(pl.col("x").median().over("c").alias("m"))["m"]
    _check(got, exp[gid], ok[gid], "categorical over")


def test_float32_and_small_integers(gpu):
    rng = np.random.default_rng(9)
    n = B + 3
    k = rng.integers(0, 9, n).astype(np.int64)
    valid = rng.random(n) >= 0.25
    gid = _gid((k, np.ones(n, bool)))
    f32 = rng.normal(0, 1, n).astype(np.float32)
    f32[rng.random(n) < 0.02] = np.nan
    df = pl.DataFrame([_series(k, None, "k"), _series(f32, valid, "f")])
    for q, m in ((0.5, "linear"), (0.24, "midpoint"), (0.9, "nearest")):
        exp, ok = _ref(f32.astype(np.float64), valid, gid, q, m)    # computed in f64, rounded once
        out = df.group_by("k", maintain_order=True).agg(pl.col("f").quantile(q, m))
        _check(out["f"], exp.astype(np.float32), ok, ("Float32", q, m), dtype=pl.Float32)
        one, _ = _ref(f32.astype(np.float64), valid, None, q, m)
        got = df.select(pl.col("f").quantile(q, m))["f"]
        _check(got, one.astype(np.float32), np.ones(1, bool), ("Float32 select", q, m), dtype=pl.Float32)
    assert isinstance(df["f"].median(), float)
    for dtype in (np.int8, np.int16, np.uint8, np.uint16, np.int32, np.uint32):
        ii = np.iinfo(dtype)
        vals = rng.integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
        df = pl.DataFrame([_series(k, None, "k"), _series(vals, valid, "v")])
        out = df.group_by("k", maintain_order=True).agg(pl.col("v").median().alias("m"), pl.col("v").quantile(1.0).alias("q"))
        _check(out["m"], *_ref(vals, valid, gid, 0.5, "linear"), (np.dtype(dtype).name, "median"))
        _check(out["q"], *_ref(vals, valid, gid, 1.0, "nearest"), (np.dtype(dtype).name, "max"))


def test_over_one_and_two_keys(gpu):
    df, h = _frame()
    g1 = _gid((h["k1"], h["k1v"]))
    g2 = _gid((h["k1"], h["k1v"]), (h["k2"], h["ones"]))
    e1, o1 = _ref(h["x"], h["xv"], g1, 0.5, "linear")
    e2, o2 = _ref(h["f"], h["fv"], g2, 0.24, "linear")
    exprs = [pl.col("x").median().over("k1").alias("a"), pl.col("f").quantile(0.24, "linear").over("k1", "k2").alias("b")]
    for out in (df.select(exprs), df.lazy().select(exprs).collect(), df.with_columns(exprs),
                df.lazy().with_columns(exprs).collect()):
        assert out.height == len(g1)
        _check(out["a"], e1[g1], o1[g1], "over k1")
        _check(out["b"], e2[g2], o2[g2], "over k1, k2")
    # below the top of an expression
    out = df.select((pl.col("x") - pl.col("x").median().over("k1")).alias("d"))["d"]
    ok = h["xv"] & o1[g1]
    assert out.dtype is pl.Float64 and np.array_equal(out.validity_numpy(), ok)
    assert np.array_equal(out.to_numpy()[ok], (h["x"] - e1[g1])[ok])


def test_shorthands(gpu):
    df, h = _frame()
    num = pl.DataFrame([df["k2"], df["x"], df["f"]])
    gid = _gid((h["k2"], h["ones"]))
    for lazy in (False, True):
        src = num.lazy() if lazy else num
        fin = (lambda r: r.collect()) if lazy else (lambda r: r)
        out = fin(src.group_by("k2", maintain_order=True).median())
        assert out.columns == ["k2", "x", "f"]
        _check(out["x"], *_ref(h["x"], h["xv"], gid, 0.5, "linear"), "GroupBy.median x")
        _check(out["f"], *_ref(h["f"], h["fv"], gid, 0.5, "linear"), "GroupBy.median f")
        out = fin(src.group_by("k2", maintain_order=True).quantile(0.24, "higher"))
        _check(out["x"], *_ref(h["x"], h["xv"], gid, 0.24, "higher"), "GroupBy.quantile x")
        _check(out["f"], *_ref(h["f"], h["fv"], gid, 0.24, "higher"), "GroupBy.quantile f")
        out = fin(src.median())
        assert out.columns == ["k2", "x", "f"] and out.height == 1
        _check(out["x"], *_ref(h["x"], h["xv"], None, 0.5, "linear"), "DataFrame.median")
        out = fin(src.quantile(0.9))
        _check(out["f"], *_ref(h["f"], h["fv"], None, 0.9, "nearest"), "DataFrame.quantile")
        _check(out["k2"], *_ref(h["k2"], h["ones"], None, 0.9, "nearest"), "DataFrame.quantile k2")
    words = pl.DataFrame([df["k2"], pl.Series("s", ["a"] * df.height)])
    with pytest.raises(pl.InvalidOperationError, match="median / quantile of a String column"):
        words.group_by("k2").median()
    with pytest.raises(pl.InvalidOperationError, match="median / quantile of a String column"):
        words.quantile(0.5)


def test_sliced_frame(gpu):
    rng = np.random.default_rng(12)
    n = B + 70
    k = rng.integers(0, 9, n).astype(np.int64)
    x = rng.integers(-40, 40, n).astype(np.int64)
    xv = rng.random(n) >= 0.3
    gid = _gid((k, np.ones(n, bool)))
    for off in (1, 64):
        df = pl.DataFrame([_sliced(k, None, off + 1, "k"), _sliced(x, xv, off, "x")])
        out = df.group_by("k", maintain_order=True).agg(pl.col("x").median().alias("m"), pl.col("x").quantile(0.9).alias("q"))
        _check(out["m"], *_ref(x, xv, gid, 0.5, "linear"), ("sliced", off))
        _check(out["q"], *_ref(x, xv, gid, 0.9, "nearest"), ("sliced", off))
        assert df["x"].median() == _ref(x, xv, None, 0.5, "linear")[0][0]
        e, o = _ref(x, xv, gid, 0.5, "linear")
        _check(df.select(pl.col("x").median().over("k"))["x"], e[gid], o[gid], ("sliced over", off))


@pytest.mark.parametrize("case", load_golden("quantile_cases.json")["cases"], ids=lambda c: c["name"])
def test_golden_cases(gpu, case):
    vals, valid, gid, q, method, ev, eok = case_inputs(case)
    s = _series(vals, None if valid.all() else valid, "value")
    e = pl.col("value").median() if case.get("median") else pl.col("value").quantile(q, method)
    if "keys" not in case:
        assert (s.median() if case.get("median") else s.quantile(q, method)) == ev[0]
        out = pl.DataFrame([s]).select(e)["value"]
        _check(out, ev, eok, "select")
        return
    (kname, key), = case["keys"].items()
    kcol = pl.Series(kname, key) if isinstance(key[0], str) else pl.Series(kname, key, dtype=pl.Int64)
    df = pl.DataFrame([kcol, s])
    out = df.group_by(kname, maintain_order=True).agg(e)
    assert out[kname].to_list() == list(dict.fromkeys(key))
    _check(out["value"], ev, eok, "group_by")
    if case.get("median"):
        _check(df.group_by(kname, maintain_order=True).median()["value"], ev, eok, "GroupBy.median")
    else:
        _check(df.group_by(kname, maintain_order=True).quantile(q, method)["value"], ev, eok, "GroupBy.quantile")
    _check(df.select(e.over(kname))["value"], ev[gid], eok[gid], "over")


def test_refused_dtypes(gpu):
    import pyarrow as pa

    n = 8
    k = pl.Series("k", [1, 1, 2, 2, 3, 3, 4, 4], dtype=pl.Int64)
    cases = [
        (pl.Series("v", ["a"] * n), "median / quantile of a String column is not supported"),
        (pl.Series.from_arrow("v", pa.array(["a"] * n, pa.string()).dictionary_encode()),
         "is not supported on the GPU executor \\(it takes numeric columns\\)"),
        (_series(np.ones(n, bool), None, "v"), "median / quantile of a Boolean column is not supported"),
        (_series(np.arange(n, dtype=np.uint64), None, "v"), "UInt64 is not among them"),
        (_series(np.arange(n, dtype=np.int32), None, "v", dtype=pl.Date), "Date, Datetime, Duration and Time medians are a follow-up"),
        (_series(np.arange(n, dtype=np.int64), None, "v", dtype=pl.Datetime("us")), "medians are a follow-up"),
        (_series(np.arange(n, dtype=np.int64), None, "v", dtype=pl.Duration("ns")), "medians are a follow-up"),
    ]
    for s, msg in cases:
        df = pl.DataFrame([k, s])
        with pytest.raises(pl.InvalidOperationError, match=msg):
            s.median()
        with pytest.raises(pl.InvalidOperationError, match=msg):
            df.select(pl.col("v").quantile(0.5))
        with pytest.raises(pl.InvalidOperationError, match=msg):
            df.group_by("k").agg(pl.col("v").median())
        with pytest.raises(pl.InvalidOperationError, match=msg):
            df.select(pl.col("v").median().over("k"))
