"""GPU: window expressions over groups -- the segmented rolling kernels
(plgpu_rolling_segmented) at their seams, plgpu_segment_starts,
plgpu_invert_permutation, and Expr.over end to end.

Bars.  Rolling: values and validity bit-exact against the existing oracle
applied to each segment / group alone (O.rolling mode ROLLING_EXACT,
O.rolling_var mode ROLLING_EXACT; integer sums and min / max their reference
mode -- for min / max, as tests/test_gpu_sort_rolling.py, -0.0 and 0.0 compare
equal since the reference's choice follows its scan order), written back to
the rows' positions.  Aggregations: bit-exact against O.group_by_agg_multi
(SUM_EXACT) mapped back per row; var / std bit-identical to what
group_by(keys).agg(...) itself returns for the row's group, and that within
the 1e-12 of the exact rational variance that tests/test_gpu_var_std.py sets
for every group-by variance path.
"""

import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from oracle import oracle as O
from polaroid_amd import _native as N
from polaroid_amd.frame import _segment_starts

pytestmark = pytest.mark.gpu

NSEAM = 8269  # 4 workgroups of 4 x 512-output wave blocks, plus a ragged tail (not a multiple of 64)


# ------------------------------------------------------------------ helpers
def _segmented(v, valid, starts, kind, w, ms, center, ddof=0, seg_series=None):
    """plgpu_rolling_segmented through the native binding -> (values, valid)."""
    s = pl.Series.from_numpy("x", v, valid)
    seg = seg_series if seg_series is not None else pl.Series.from_numpy("seg", starts)
    out = N.Column()
    code = N.ROLLING[kind] | (ddof << 8)
    N.check(N.lib().plgpu_rolling_segmented(C.byref(s._col), C.byref(seg._col), code, w, ms, int(center),
                                            C.byref(out), None))
    r = pl.Series._from_native("x", out)
    return r.to_numpy(), r.validity_numpy()


def _plain(v, valid, kind, w, ms, center, ddof=0):
    s = pl.Series.from_numpy("x", v, valid)
    out = N.Column()
    N.check(N.lib().plgpu_rolling(C.byref(s._col), N.ROLLING[kind] | (ddof << 8), w, ms, int(center),
                                  C.byref(out), None))
    r = pl.Series._from_native("x", out)
    return r.to_numpy(), r.validity_numpy()


def _oracle_one(v, valid, kind, w, ms, center, ddof):
    hc = O.HostCol(np.ascontiguousarray(v), None if valid is None else np.ascontiguousarray(valid))
    if kind in ("var", "std"):
        return O.rolling_var(hc, w, ms, center, ddof, kind == "std", O.ROLLING_EXACT)
    isint = v.dtype.kind in "iu"
    if kind in ("min", "max") or (isint and kind == "sum"):
        return O.rolling(hc, kind, w, ms, center, O.ROLLING_REFERENCE)
    return O.rolling(hc, kind, w, ms, center, O.ROLLING_EXACT)


def _expected_by_rows(v, valid, row_sets, kind, w, ms, center, ddof=0):
    """The oracle on each row set (a segment or a group, rows in order) alone,
    written back to those rows."""
    n = v.shape[0]
    isint = v.dtype.kind in "iu" and kind in ("sum", "min", "max")
    ev = np.zeros(n, np.int64 if isint else np.float64)
    eok = np.zeros(n, bool)
    for rows in row_sets:
        x, ok = _oracle_one(v[rows], None if valid is None else valid[rows], kind, w, ms, center, ddof)
        ev[rows], eok[rows] = x, ok
    return ev, eok


def _segments(starts):
    b = np.flatnonzero(starts)
    assert starts.shape[0] == 0 or b[0] == 0
    ends = np.append(b[1:], starts.shape[0])
    return [np.arange(a, e) for a, e in zip(b, ends)]


def _same(gv, gok, ev, eok, kind, what):
    assert np.array_equal(gok, eok), (what, np.flatnonzero(gok != eok)[:8])
    g, e = gv[gok], ev[eok]
    if e.dtype.kind in "iu":
        assert np.array_equal(g.astype(np.int64), e), what
        return
    assert np.array_equal(np.isnan(g), np.isnan(e)), what
    m = ~np.isnan(e)
    if kind in ("min", "max"):
        assert np.array_equal(g[m], e[m]), what
    else:
        bad = np.flatnonzero(g[m].view(np.int64) != e[m].view(np.int64))
        assert bad.size == 0, (what, bad[:8], g[m][bad[:4]], e[m][bad[:4]])


def _seam_starts(n, w, rng):
    """Segment starts at the wave-block, workgroup and column seams, one
    stretch of 1500 rows without a start (interior blocks keep the
    specialised scan), one stretch with a start every 1-6 rows (segments
    shorter than the window and than min_samples)."""
    st = np.zeros(n, bool)
    for r in (0, 1, 2, 63, 64, 65, 511, 512, 513, 512 + w - 1, 512 + w, 2048 - w + 1, 2047, 2048, 2049, n - 1):
        if 0 <= r < n:
            st[r] = True
    # rows 2050 .. 3549: no start
    r = 4200
    while r < 4800:
        st[r] = True
        r += int(rng.integers(1, 7))
    for r in (3550, 3583, 3584, 4100, 5000, 5119, 5120, 5121, 6143, 6144, 6700, 7168, 8191, 8192, 8200):
        st[r] = True
    assert not st[2050:3550].any()
    return st


def _data(form, n, rng):
    if form == "prices":     # a few binades, null-free: the int64 form, the hot / rest split
        return rng.uniform(100, 150, n) * np.exp(0.02 * rng.standard_normal(n)), None
    if form == "specials":   # 3 % nulls, NaN and +-inf
        v = rng.standard_normal(n) * 10
        v[rng.random(n) < 0.01] = np.nan
        v[rng.random(n) < 0.01] = np.inf
        v[rng.random(n) < 0.01] = -np.inf
        return v, rng.random(n) > 0.03
    if form == "wide128":    # ~40 binades, mixed signs: the 128-bit form
        return rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n)), None
    v = rng.uniform(-1, 1, n)  # "huge": beyond 128 bits, the exact per-output path
    v[::31] = 1e200
    v[1::31] = -1e200
    v[3::31] = -0.0
    return v, None


# --------------------------------------------------------- golden fixtures
_DT = {"String": pl.String, "Int64": pl.Int64, "Int32": pl.Int32, "Float64": pl.Float64}


def _golden_expr(spec):
    if "len" in spec:
        e = pl.len()
    else:
        e = pl.col(spec["col"])
        if "agg" in spec:
            e = getattr(e, spec["agg"])()
    if "over" in spec:
        e = e.over(spec["over"]) if spec.get("as_list", True) else e.over(*spec["over"])
    if "minus" in spec:
        e = pl.col(spec["col"]) - _golden_expr(spec["minus"])
    return e


@pytest.mark.parametrize("lazy", [False, True])
def test_over_golden(gpu, lazy):
    for case in load_golden("over_cases.json")["cases"]:
        df = pl.DataFrame([pl.Series(k, v, _DT[case["dtypes"][k]]) for k, v in case["frame"].items()])
        exprs = [_golden_expr(s) for s in case["exprs"]]
        src = df.lazy() if lazy else df
        out = getattr(src, case["op"])(*exprs)
        out = out.collect() if lazy else out
        if "expected" in case:
            assert out.columns == list(case["expected"]), case["name"]
            for k, exp in case["expected"].items():
                assert out[k].to_list() == exp, (case["name"], k, out[k].to_list())
        for k, exp in case.get("isclose_first", {}).items():
            got = out[k].to_list()[0]
            assert abs(got - exp) <= 1e-8 + 1e-5 * abs(exp), (case["name"], got)  # np.isclose's defaults


# ------------------------------------------- the segmented kernel's seams
@pytest.mark.parametrize("w", [1, 2, 20, 64])
@pytest.mark.parametrize("form", ["prices", "specials", "wide128", "huge"])
def test_segmented_wave_kernel_seams(gpu, plgpu_option, form, w):
    rng = np.random.default_rng(w * 11 + len(form))
    v, valid = _data(form, NSEAM, rng)
    starts = _seam_starts(NSEAM, w, rng)
    segs = _segments(starts)
    seg = pl.Series.from_numpy("seg", starts)
    plgpu_option("ktime", 1)
    N.ktime_read()
    for kind in ("sum", "mean", "var", "std"):
        ddof = 1 if kind in ("var", "std") else 0
        for center in (False, True):
            for ms in sorted({1, w}):
                gv, gok = _segmented(v, valid, starts, kind, w, ms, center, ddof, seg)
                ev, eok = _expected_by_rows(v, valid, segs, kind, w, ms, center, ddof)
                _same(gv, gok, ev, eok, kind, (form, kind, w, ms, center))
    kt = N.ktime_read()
    assert kt.get("rl_wave_seg_kernel", (0, 0))[1] > 0 and kt.get("rl_wave_var_seg_kernel", (0, 0))[1] > 0, kt
    assert "rl_wave_kernel" not in kt and "rl_wave_var_kernel" not in kt, kt


@pytest.mark.parametrize("dt", [np.int64, np.int32])
def test_segmented_integer_sums(gpu, dt):
    rng = np.random.default_rng(5)
    v = rng.integers(np.iinfo(dt).min // 2, np.iinfo(dt).max // 2, NSEAM).astype(dt)
    for valid in (None, rng.random(NSEAM) > 0.05):
        for w in (2, 20, 64):
            starts = _seam_starts(NSEAM, w, rng)
            segs = _segments(starts)
            for kind, ms, center in (("sum", 1, False), ("sum", w, True), ("mean", 1, True)):
                gv, gok = _segmented(v, valid, starts, kind, w, ms, center)
                if kind == "sum":
                    assert gv.dtype == dt
                ev, eok = _expected_by_rows(v, valid, segs, kind, w, ms, center)
                _same(gv, gok, ev, eok, kind, (dt, kind, w, ms, center))


@pytest.mark.parametrize("w", [65, 1100, 3100])
def test_segmented_wide_windows(gpu, w):
    """w > 64: the two LDS tile sizes and the direct kernel (sum / mean), the
    direct variance kernel at w = 65."""
    rng = np.random.default_rng(w)
    starts = _seam_starts(NSEAM, min(w, 400), rng)
    segs = _segments(starts)
    for form in ("prices", "specials"):
        v, valid = _data(form, NSEAM, rng)
        for kind in ("sum", "mean") + (("var",) if w == 65 else ()):
            for ms, center in ((1, False), (w, False), (max(1, w // 3), True)):
                ddof = 1 if kind == "var" else 0
                gv, gok = _segmented(v, valid, starts, kind, w, ms, center, ddof)
                ev, eok = _expected_by_rows(v, valid, segs, kind, w, ms, center, ddof)
                _same(gv, gok, ev, eok, kind, (form, kind, w, ms, center))


@pytest.mark.parametrize("w", [3, 64, 65, 300])
@pytest.mark.parametrize("kind", ["min", "max"])
def test_segmented_min_max(gpu, kind, w):
    rng = np.random.default_rng(w + len(kind))
    starts = _seam_starts(NSEAM, min(w, 400), rng)
    segs = _segments(starts)
    x = rng.standard_normal(NSEAM) * 100
    x[rng.random(NSEAM) < 0.01] = np.nan
    x[rng.random(NSEAM) < 0.01] = np.inf
    x[rng.random(NSEAM) < 0.01] = -0.0
    nulls = rng.random(NSEAM) > 0.05
    for v in (x, rng.integers(-2**40, 2**40, NSEAM).astype(np.int64),
              rng.integers(-2**31, 2**31, NSEAM).astype(np.int32)):
        for valid, ms, center in ((None, w, False), (nulls, 1, True), (nulls, max(1, w // 2), False)):
            gv, gok = _segmented(v, valid, starts, kind, w, ms, center)
            assert gv.dtype == v.dtype
            ev, eok = _expected_by_rows(v, valid, segs, kind, w, ms, center)
            _same(gv, gok, ev, eok, kind, (v.dtype, kind, w, ms, center))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_segmented_small_columns(gpu, n):
    rng = np.random.default_rng(n)
    v = rng.uniform(1, 2, n)
    valid = rng.random(n) > 0.2
    starts = rng.random(n) < 0.2
    if n:
        starts[0] = True
    segs = _segments(starts) if n else []
    for kind, w in (("sum", 3), ("mean", 20), ("var", 4), ("std", 64), ("min", 3), ("max", 70), ("sum", 70),
                    ("var", 70)):
        ddof = 1 if kind in ("var", "std") else 0
        for vd in (None, valid):
            gv, gok = _segmented(v, vd, starts, kind, w, 1, True, ddof)
            assert gv.shape[0] == n
            ev, eok = _expected_by_rows(v, vd, segs, kind, w, 1, True, ddof)
            _same(gv, gok, ev, eok, kind, (n, kind, w))


def test_segmented_takes_a_sliced_start_column(gpu):
    """A start column with an Arrow offset (not word-aligned) is re-packed."""
    rng = np.random.default_rng(77)
    n, off = 3000, 13
    v = rng.uniform(100, 150, n)
    full = rng.random(n + off + 5) < 0.01
    full[off] = True
    starts = full[off:off + n]
    seg = pl.Series.from_numpy("seg", full).slice(off, n)
    for kind, w in (("mean", 20), ("max", 5), ("sum", 100)):
        gv, gok = _segmented(v, None, starts, kind, w, 1, False, 0, seg)
        ev, eok = _expected_by_rows(v, None, _segments(starts), kind, w, 1, False)
        _same(gv, gok, ev, eok, kind, (kind, w))


@pytest.mark.parametrize("kind", ["sum", "mean", "min", "max", "var", "std"])
def test_no_boundary_means_no_difference(gpu, kind):
    """Only bit 0 set: plgpu_rolling_segmented equals plgpu_rolling bit for bit."""
    rng = np.random.default_rng(len(kind))
    starts = np.zeros(NSEAM, bool)
    starts[0] = True
    ddof = 1 if kind in ("var", "std") else 0
    for form in ("prices", "specials"):
        v, valid = _data(form, NSEAM, rng)
        for ms, center in ((20, False), (1, True)):
            gv, gok = _segmented(v, valid, starts, kind, 20, ms, center, ddof)
            pv, pok = _plain(v, valid, kind, 20, ms, center, ddof)
            assert np.array_equal(gok, pok)
            assert np.array_equal(gv.view(np.uint64), pv.view(np.uint64)), (kind, form, ms, center)


# ------------------------------------------- segment starts / permutation
def test_segment_starts_equality_and_order(gpu, plgpu_option):
    nan2 = np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0]
    f = np.array([-0.0, 0.0, 1.0, 1.0, np.nan, nan2, np.nan], np.float64)
    st, srt = _segment_starts([pl.Series.from_numpy("f", f)])
    assert st.to_numpy().tolist() == [True, False, True, False, True, False, False] and srt  # TotalEq, NaN last
    i = np.array([5, 5, 7, 7, 7, 9], np.int64)
    iv = np.array([0, 0, 1, 1, 1, 1], bool)
    st, srt = _segment_starts([pl.Series.from_numpy("i", i, iv)])
    assert st.to_numpy().tolist() == [True, False, True, False, False, True] and srt  # null == null, nulls first
    st, srt = _segment_starts([pl.Series.from_numpy("i", i, iv[::-1].copy())])
    assert st.to_numpy().tolist() == [True, False, True, False, True, False] and not srt  # a null after a value
    a = np.array([1, 1, 1, 2, 2, 1], np.int64)
    b = np.array([3, 3, 4, 1, 1, 1], np.int32)
    st, srt = _segment_starts([pl.Series.from_numpy("a", a), pl.Series.from_numpy("b", b)])
    assert st.to_numpy().tolist() == [True, False, True, True, False, True] and not srt
    st, srt = _segment_starts([pl.Series.from_numpy("a", a[:5]), pl.Series.from_numpy("b", b[:5])])
    assert srt
    plgpu_option("over_presorted", 0)  # the option is the caller's: the pass reports what it finds
    st, srt = _segment_starts([pl.Series.from_numpy("a", a[:5])])
    assert st.to_numpy().tolist() == [True, False, False, True, False] and srt
    rng = np.random.default_rng(1)
    n = 100_003
    k = np.sort(rng.integers(0, 50, n)).astype(np.int64)
    plgpu_option("over_presorted", 1)
    st, srt = _segment_starts([pl.Series.from_numpy("k", k)])
    assert srt and np.array_equal(st.to_numpy(), np.append(True, k[1:] != k[:-1]))
    assert st.null_count() == 0 and st.dtype is pl.Boolean


def test_invert_permutation(gpu):
    rng = np.random.default_rng(2)
    n = 100_003
    perm = rng.permutation(n).astype(np.uint32)
    src = pl.Series.from_numpy("p", perm)  # (held: its device buffer lives as long as the Series)
    out = N.Column()
    N.check(N.lib().plgpu_invert_permutation(C.byref(src._col), C.byref(out), None))
    inv = pl.Series._from_native("inv", out)
    assert inv.dtype is pl.UInt32 and inv.null_count() == 0
    assert np.array_equal(inv.to_numpy().astype(np.int64), np.argsort(perm))


# ------------------------------------------------------- over, end to end
NOVER = 20_000


def _groups(rng):
    """37 group sizes summing to NOVER: groups of 1 row, of more than 2048."""
    fixed = [1, 1, 2, 5, 2600, 3100, 64, 65, 511, 513]
    rest = rng.multinomial(NOVER - sum(fixed) - 27, np.ones(27) / 27) + 1
    sizes = np.array(fixed + rest.tolist())
    assert sizes.size == 37 and sizes.sum() == NOVER and sizes.min() == 1 and sizes.max() > 2048
    return sizes[rng.permutation(37)]


def _key_frames(kind, gid):
    """Key columns for group ids 0..36 in sorted (ascending, nulls first)
    order of the ids: {name: (values, valid)}."""
    if kind == "i64":
        return {"k": ((gid * 1000 - 7000).astype(np.int64), None)}
    if kind == "pair":
        return {"k": ((gid // 5).astype(np.int64), None), "j": ((gid % 5 - 2).astype(np.int32), None)}
    if kind == "nullable":
        return {"k": (np.where(gid == 0, 123, gid * 3).astype(np.int64), gid != 0)}
    # a short-string code is (length << 56) | bytes, little-endian: equal lengths order by the last
    # byte first, so the digits go in reverse for the codes to ascend with the group id
    return {"k": (np.array([f"{g % 10}{g // 10}s" for g in gid], dtype=object), None)}


def _frame(keys, cols):
    ser = []
    for nm, (v, m) in keys.items():
        ser.append(pl.Series(nm, v.tolist()) if v.dtype == object else pl.Series.from_numpy(nm, v, m))
    for nm, (v, m) in cols.items():
        ser.append(pl.Series.from_numpy(nm, v, m))
    return pl.DataFrame(ser)


def _interleave(gid, rng):
    """A shuffle that keeps every group's rows in their relative order:
    pos[r] = the shuffled position of sorted-layout row r."""
    labels = rng.permutation(gid)
    pos = np.empty(gid.shape[0], np.int64)
    for g in np.unique(gid):
        pos[np.flatnonzero(gid == g)] = np.flatnonzero(labels == g)
    return pos


def _take(cols, order):
    return {nm: (v[order], None if m is None else m[order]) for nm, (v, m) in cols.items()}


_ROLLS = [("mean", 20, 1, False, 0), ("sum", 20, 20, False, 0), ("std", 5, 2, True, 1), ("var", 64, 1, False, 0),
          ("min", 3, 1, False, 0), ("max", 100, 1, True, 0), ("mean", 300, 5, False, 0)]


@pytest.mark.parametrize("kkind", ["i64", "pair", "nullable", "string"])
def test_over_rolling_end_to_end(gpu, plgpu_option, kkind):
    rng = np.random.default_rng(len(kkind))
    gid = np.repeat(np.arange(37), _groups(rng))
    close = rng.uniform(100, 150, NOVER) * np.exp(0.02 * rng.standard_normal(NOVER))
    cvalid = rng.random(NOVER) > 0.03
    keys = _key_frames(kkind, gid)
    cols = {"close": (close, cvalid)}
    row_sets = [np.flatnonzero(gid == g) for g in range(37)]
    pos = _interleave(gid, rng)
    order = np.argsort(pos)  # shuffled row -> sorted-layout row
    exprs = []
    for i, (kd, w, ms, c, dd) in enumerate(_ROLLS):
        kw = {"ddof": dd} if kd in ("var", "std") else {}
        roll = getattr(pl.col("close"), "rolling_" + kd)(w, min_samples=ms, center=c, **kw)
        exprs.append(roll.over(list(keys)).alias(f"r{i}"))
    plgpu_option("ktime", 1)
    df_sorted = _frame(keys, cols)
    N.ktime_read()
    out_sorted = df_sorted.select(*exprs)
    kt = N.ktime_read()
    assert not [k for k in kt if k.startswith("srt_")] and "invert_perm_kernel" not in kt, kt
    assert kt["seg_starts_kernel"][1] == 1, kt  # one pass for the seven expressions over the same keys
    df_shuf = _frame(_take(keys, order), _take(cols, order))
    N.ktime_read()
    out_shuf = df_shuf.with_columns(*exprs)
    kt = N.ktime_read()
    assert [k for k in kt if k.startswith("srt_")], kt
    # one sort for the seven expressions: the rows as they stand, then the sorted rows
    assert kt["invert_perm_kernel"][1] == 1 and kt["seg_starts_kernel"][1] == 2, kt
    assert out_shuf.columns == list(keys) + ["close"] + [f"r{i}" for i in range(len(_ROLLS))]
    plgpu_option("over_presorted", 0)
    N.ktime_read()
    out_forced = df_sorted.select(*exprs)
    kt = N.ktime_read()
    assert [k for k in kt if k.startswith("srt_")], kt
    for i, (kd, w, ms, c, dd) in enumerate(_ROLLS):
        ev, eok = _expected_by_rows(close, cvalid, row_sets, kd, w, ms, c, dd)
        a = out_sorted[f"r{i}"]
        _same(a.to_numpy(), a.validity_numpy(), ev, eok, kd, (kkind, "sorted", kd, w))
        b = out_shuf[f"r{i}"]
        _same(b.to_numpy()[pos], b.validity_numpy()[pos], ev, eok, kd, (kkind, "shuffled", kd, w))
        f = out_forced[f"r{i}"]
        assert np.array_equal(f.validity_numpy(), a.validity_numpy())
        assert np.array_equal(f.to_numpy().view(np.uint64), a.to_numpy().view(np.uint64)), (kkind, "forced", kd)


def test_over_rolling_of_an_expression_and_integers(gpu):
    rng = np.random.default_rng(9)
    n = 5000
    k = np.sort(rng.integers(0, 9, n)).astype(np.int64)
    a = rng.uniform(1, 2, n)
    b = rng.integers(-50, 50, n).astype(np.int64)
    df = pl.DataFrame({"k": pl.Series.from_numpy("k", k), "a": pl.Series.from_numpy("a", a),
                       "b": pl.Series.from_numpy("b", b)})
    out = df.select((pl.col("a") * 3.0).rolling_sum(7, min_samples=1).over("k").alias("x"),
                    pl.col("b").rolling_sum(4).over(pl.col("k")),
                    (pl.col("a") - pl.col("a").rolling_mean(5, min_samples=1).over("k")).alias("d"))
    rows = [np.flatnonzero(k == g) for g in np.unique(k)]
    ev, eok = _expected_by_rows(a * 3.0, None, rows, "sum", 7, 1, False)
    _same(out["x"].to_numpy(), out["x"].validity_numpy(), ev, eok, "sum", "expr")
    ev, eok = _expected_by_rows(b, None, rows, "sum", 4, 4, False)
    assert out["b"].dtype is pl.Int64
    _same(out["b"].to_numpy(), out["b"].validity_numpy(), ev, eok, "sum", "int")
    ev, eok = _expected_by_rows(a, None, rows, "mean", 5, 1, False)
    assert eok.all() and np.array_equal(out["d"].to_numpy().view(np.uint64), (a - ev).view(np.uint64))


def test_over_refusals_at_collect(gpu):
    df = pl.DataFrame({"s": pl.Series("s", ["a-string-longer-than-seven", "b"]), "x": [1.0, 2.0]})
    with pytest.raises(pl.InvalidOperationError, match="longer than 7 bytes"):
        df.select(pl.col("x").rolling_sum(2).over("s"))
    with pytest.raises(pl.ComputeError):
        df.select(pl.col("x").rolling_sum(2).over("nope"))
    with pytest.raises(pl.ComputeError):
        df.select(pl.col("x").sum().over("nope"))


# ------------------------------------------------ aggregations over groups
def _dense_ids(keys):
    """Group id per row, groups numbered by first occurrence (O._row_words tuples)."""
    enc = np.concatenate([O._row_words(v, m) for v, m in keys], axis=1)
    _, first, inv = np.unique(enc, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], np.int64)
    rank[np.argsort(first)] = np.arange(first.shape[0])
    return rank[inv.reshape(-1)]


def _exact_var(vals, ddof):
    fv = [Fraction(float(v)) for v in vals]
    n = len(fv)
    return float((n * sum(v * v for v in fv) - sum(fv) ** 2) / (n * (n - ddof)))


@pytest.mark.parametrize("kkind", ["i64", "pair", "nullable", "string"])
def test_over_aggregations(gpu, kkind):
    rng = np.random.default_rng(3 + len(kkind))
    n = NOVER
    gid = rng.permutation(np.repeat(np.arange(37), _groups(rng)))
    keys = _key_frames(kkind, gid)
    close = rng.uniform(100, 150, n)
    cvalid = rng.random(n) > 0.1
    cvalid[gid == 5] = False  # an all-null group: sum 0, mean / min / max null
    volume = rng.integers(1, 10_000, n).astype(np.int64)
    df = _frame(keys, {"close": (close, cvalid), "volume": (volume, None)})
    kl = list(keys)
    names = ["sum", "mean", "min", "max", "count", "len", "first", "last"]
    exprs = [getattr(pl.col("close"), nm)().over(kl).alias(nm) for nm in names]
    exprs += [pl.col("volume").sum().over(kl).alias("vsum"), pl.len().over(kl).alias("n"),
              (pl.col("close") * pl.col("volume")).sum().over(kl).alias("notional"),
              pl.col("close").std(1).over(kl).alias("std1"), pl.col("close").var(0).over(kl).alias("var0"),
              (pl.col("close") - pl.col("close").mean().over(kl)).alias("demeaned")]
    out = df.with_columns(*exprs)
    assert out.height == n and out.columns[:len(kl) + 2] == kl + ["close", "volume"]
    okeys = list(keys.values())
    if kkind == "string":  # the oracle groups the strings by their dense codes
        okeys = [(np.unique(keys["k"][0].astype(str), return_inverse=True)[1].reshape(-1).astype(np.int64), None)]
    ids = _dense_ids(okeys)
    prod = close * volume.astype(np.float64)
    hcols = [O.HostCol(close, cvalid), O.HostCol(volume), O.HostCol(prod, cvalid)]
    aggs = [(nm, 0) for nm in names] + [("sum", 1), ("len", 0), ("sum", 2)]
    _, outs = O.group_by_agg_multi(okeys, hcols, [], aggs, n, O.SUM_EXACT)
    for nm, (ev, eok) in zip(names + ["vsum", "n", "notional"], outs):
        g = out[nm]
        gv, gok = g.to_numpy(), g.validity_numpy()
        assert np.array_equal(gok, eok[ids]), nm
        e = ev[ids][gok]
        if e.dtype.kind == "f":
            assert np.array_equal(gv[gok].view(np.uint64), e.view(np.uint64)), nm
        else:
            assert np.array_equal(gv[gok].astype(np.int64), e.astype(np.int64)), nm
    assert out["n"].dtype is pl.UInt32 and out["vsum"].dtype is pl.Int64
    # demeaned = close - mean.over, elementwise on the materialised window column
    mean = out["mean"].to_numpy()
    ok = out["demeaned"].validity_numpy()
    assert np.array_equal(ok, cvalid & out["mean"].validity_numpy())
    assert np.array_equal(out["demeaned"].to_numpy()[ok].view(np.uint64), (close - mean)[ok].view(np.uint64))
    # var / std: what group_by itself returns for the row's group, and that
    # within test_gpu_var_std.py's 1e-12 of the exact rational variance
    gb = df.group_by(*kl, maintain_order=True).agg(pl.col("close").std(1).alias("std1"),
                                                   pl.col("close").var(0).alias("var0"))
    for nm, ddof, root in (("std1", 1, True), ("var0", 0, False)):
        gv, gok = gb[nm].to_numpy(), gb[nm].validity_numpy()
        a = out[nm]
        assert np.array_equal(a.validity_numpy(), gok[ids]), nm
        m = a.validity_numpy()
        assert np.array_equal(a.to_numpy()[m].view(np.uint64), gv[ids][m].view(np.uint64)), nm
        for g in range(37):
            vals = close[(ids == g) & cvalid]
            if len(vals) <= ddof:
                assert not gok[g]
                continue
            exact = _exact_var(vals, ddof)
            assert math.isclose(gv[g], math.sqrt(exact) if root else exact, rel_tol=1e-12), (nm, g)
