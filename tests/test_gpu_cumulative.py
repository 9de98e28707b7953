"""GPU: cumulative and lag expressions -- the three-launch segmented scans
(plgpu_cumulative) and the lag kernel (plgpu_lag) at their seams, the Float64
number formats, the two bit identities with rolling_sum and sum().over, and
cum_* / shift / diff end to end, plain and over groups.

Bars.  Integer sums, min / max, counts, shift and diff: equal to numpy per
segment (cumsum wrapping at the dtype's width, minimum / maximum.accumulate
with NaN skipped once a value has been seen, numpy's own subtraction); -0.0
and 0.0 compare equal for min / max.  Float64 sums: bit-equal to float() of
the running fractions.Fraction sum (the correctly rounded exact sum, +0.0 for
a zero sum), NaN / +-inf by the rules of DESIGN.md "Cumulative and lag
expressions"; and within i * 2^-53 * sum|x_j| + ulp/2 of the reference's
sequential f64 fold (the fold's own error bound)."""

import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from polaroid_amd import _native as N
from polaroid_amd import polars_engine as PE

pytestmark = pytest.mark.gpu

T = N.CUM_TILE    # rows of one workgroup: one summary, one carry
B = N.CUM_BLOCK   # rows of one of the scans a workgroup runs one after the other
NS = 3 * T + 37


# ------------------------------------------------------------------ helpers
def _placements(n):
    """Segment-start layouts: {name: Boolean array}."""
    def at(rows):
        st = np.zeros(n, bool)
        st[[r for r in rows if 0 <= r < n]] = True
        return st

    return {
        "row0": at([0]),
        "tile_first": at([0, T, 2 * T, 3 * T]),
        "tile_last": at([0, T - 1, 2 * T - 1, 3 * T - 1]),
        "wave_word": at([0, 63, 64, 65, 127, 128, 129, T + 63, T + 64, 2 * T + 1, 3 * T + 36]),
        "span2": at([0, T - 5, 3 * T + 3]),  # one segment covers two whole tiles
        "block_seams": at([0, B - 1, B, B + 1, 3 * B, 5 * B - 1, T + 2 * B, T + 7 * B - 1, 2 * T + B + 3]),
        "every": np.ones(n, bool),
    }


def _seg_info(starts):
    """(first row of each row's segment) for starts with row 0 set."""
    st = starts.copy()
    if st.size:
        st[0] = True
    first = np.flatnonzero(st)
    return first[np.cumsum(st) - 1] if st.size else np.zeros(0, np.int64)


def _since_start(ind, first):
    """Inclusive running count of `ind` within each row's segment."""
    c = np.cumsum(ind.astype(np.int64))
    before = np.where(first > 0, c[np.maximum(first - 1, 0)], 0)
    return c - before


def _cum(s, kind, seg=None):
    out = N.Column()
    N.check(N.lib().plgpu_cumulative(C.byref(s._col), None if seg is None else C.byref(seg._col), N.CUM[kind],
                                     C.byref(out), None))
    r = pl.Series._from_native("x", out)
    return r.to_numpy(), r.validity_numpy()


def _lag(s, op, n, seg=None, fill=None):
    out = N.Column()
    N.check(N.lib().plgpu_lag(C.byref(s._col), None if seg is None else C.byref(seg._col), N.LAG[op], n,
                              int(fill is not None), 0 if fill is None else fill, C.byref(out), None))
    r = pl.Series._from_native("x", out)
    return r.to_numpy(), r.validity_numpy()


class _ExactSums:
    """Running exact sums of a Float64 column (finite, non-null values)."""

    def __init__(self, v, valid):
        ok = valid & np.isfinite(v)
        self.prefix = [Fraction(0)]
        for x, k in zip(v.tolist(), ok.tolist()):
            self.prefix.append(self.prefix[-1] + (Fraction(x) if k else 0))
        self.nan = valid & np.isnan(v)
        self.pinf = valid & (v == np.inf)
        self.ninf = valid & (v == -np.inf)

    def expected(self, first):
        n = first.shape[0]
        out = np.zeros(n)
        nan, pinf, ninf = (_since_start(a, first) > 0 for a in (self.nan, self.pinf, self.ninf))
        for i in range(n):
            if nan[i] or (pinf[i] and ninf[i]):
                out[i] = np.nan
            elif pinf[i] or ninf[i]:
                out[i] = np.inf if pinf[i] else -np.inf
            else:
                q = self.prefix[i + 1] - self.prefix[first[i]]
                try:
                    out[i] = float(q)
                except OverflowError:
                    out[i] = np.inf if q > 0 else -np.inf
        return out


def _ref(v, valid, first, kind, exact=None):
    """Expected (values, validity) of one cumulative kind."""
    if kind == "count":
        return _since_start(valid, first).astype(np.uint32), np.ones(v.shape[0], bool)
    if kind == "sum" and v.dtype.kind == "f":
        return (exact or _ExactSums(v, valid)).expected(first), valid
    if kind == "sum":
        with np.errstate(over="ignore"):
            c = np.cumsum(np.where(valid, v, 0).astype(v.dtype), dtype=v.dtype)
            before = np.where(first > 0, c[np.maximum(first - 1, 0)], 0).astype(v.dtype)
            return c - before, valid
    # min / max: per segment, null and NaN skipped; NaN until a value has been seen
    acc = np.minimum.accumulate if kind == "min" else np.maximum.accumulate
    skip = ~valid | (np.isnan(v) if v.dtype.kind == "f" else False)
    if v.dtype.kind == "f":
        ident = np.inf if kind == "min" else -np.inf
    else:
        ident = np.iinfo(v.dtype).max if kind == "min" else np.iinfo(v.dtype).min
    x = np.where(skip, v.dtype.type(ident), v)
    out = np.empty_like(v)
    bounds = np.flatnonzero(np.append(first[1:] != first[:-1], True)) + 1 if v.size else []
    a = 0
    for b in bounds:
        out[a:b] = acc(x[a:b])
        a = b
    if v.dtype.kind == "f":
        out = np.where(_since_start(~skip, first) > 0, out, np.nan)
    return out, valid


def _assert_same(gv, gok, ev, eok, what, bits=False):
    assert np.array_equal(gok, eok), (what, np.flatnonzero(gok != eok)[:8])
    g, e = gv[eok], ev[eok]
    if e.dtype.kind in "iu":
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, np.flatnonzero(g != e)[:8])
        return
    assert np.array_equal(np.isnan(g), np.isnan(e)), (what, np.flatnonzero(np.isnan(g) != np.isnan(e))[:8])
    m = ~np.isnan(e)
    if bits:
        bad = np.flatnonzero(g[m].view(np.uint64) != e[m].view(np.uint64))
        assert bad.size == 0, (what, bad[:8], g[m][bad[:4]], e[m][bad[:4]])
    else:
        assert np.array_equal(g[m], e[m]), (what, np.flatnonzero(g[m] != e[m])[:8])


def _values(dt, n, rng):
    if dt == "f64":
        v = rng.standard_normal(n) * np.exp2(rng.integers(-8, 8, n))
        v[rng.random(n) < 0.02] = np.nan
        return v
    if dt == "i64":
        v = rng.integers(-2**62, 2**62, n, dtype=np.int64)  # sums wrap
        v[5], v[6] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
        return v
    v = rng.integers(-2**30, 2**30, n).astype(np.int32)
    v[5], v[6] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    return v


# ------------------------------------------------------------------- seams
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("dt", ["i64", "i32", "f64"])
@pytest.mark.parametrize("kind", ["sum", "min", "max", "count"])
def test_scan_seams(gpu, kind, dt, nullable):
    rng = np.random.default_rng(len(kind) * 7 + len(dt) + nullable)
    v = _values(dt, NS, rng)
    if kind == "sum" and dt == "f64":
        v = np.where(np.isnan(v), 0.5, v)
        v[[100, T + 3, 2 * T + 700]] = [np.nan, np.inf, -np.inf]
    valid = rng.random(NS) > 0.05 if nullable else np.ones(NS, bool)
    s = pl.Series.from_numpy("x", v, valid if nullable else None)
    exact = _ExactSums(v, valid) if (kind == "sum" and dt == "f64") else None
    bits = kind == "sum"
    pv, pok = _cum(s, kind)
    ev, eok = _ref(v, valid, np.zeros(NS, np.int64), kind, exact)
    _assert_same(pv, pok, ev, eok, (kind, dt, "plain"), bits)
    for name, st in _placements(NS).items():
        gv, gok = _cum(s, kind, pl.Series.from_numpy("seg", st))
        ev, eok = _ref(v, valid, _seg_info(st), kind, exact)
        _assert_same(gv, gok, ev, eok, (kind, dt, name), bits)
        if name == "row0":  # bit 0 only == the NULL-bitmap call, bit for bit
            assert np.array_equal(gok, pok)
            assert gv.tobytes() == pv.tobytes() or np.array_equal(gv[gok].view(np.uint8), pv[pok].view(np.uint8))


@pytest.mark.parametrize("kind, dt", [("sum", "f64"), ("sum", "i64"), ("max", "f64"), ("min", "i32"),
                                      ("count", "f64")])
def test_scan_of_a_sliced_input(gpu, kind, dt):
    """A slice that starts at an odd row: 8-byte values that are not 16-byte
    aligned, validity bits that start inside a byte."""
    rng = np.random.default_rng(11)
    full = _values(dt, NS + 10, rng)
    if kind == "sum" and dt == "f64":
        full = np.where(np.isnan(full), 0.25, full)
    fvalid = rng.random(NS + 10) > 0.1
    s = pl.Series.from_numpy("x", full, fvalid).slice(3, NS)
    v, valid = full[3:3 + NS], fvalid[3:3 + NS]
    bits = kind == "sum"
    for name in ("plain", "wave_word", "tile_last", "block_seams"):
        st = None if name == "plain" else _placements(NS)[name]
        gv, gok = _cum(s, kind, None if st is None else pl.Series.from_numpy("seg", st))
        first = np.zeros(NS, np.int64) if st is None else _seg_info(st)
        ev, eok = _ref(v, valid, first, kind)
        _assert_same(gv, gok, ev, eok, (kind, dt, name, "sliced"), bits)
    # a sliced start column as well (bits repacked from an offset)
    st = _placements(NS)["wave_word"]
    seg = pl.Series.from_numpy("seg", np.concatenate([np.ones(5, bool), st])).slice(5, NS)
    gv, gok = _cum(s, kind, seg)
    ev, eok = _ref(v, valid, _seg_info(st), kind)
    _assert_same(gv, gok, ev, eok, (kind, dt, "sliced starts"), bits)


def test_cast_dtypes_once_each(gpu):
    rng = np.random.default_rng(3)
    n = 700
    valid = rng.random(n) > 0.1
    one = np.zeros(n, np.int64)
    for npdt, name in ((np.int8, "Int8"), (np.int16, "Int16"), (np.uint8, "UInt8"), (np.uint16, "UInt16")):
        v = rng.integers(np.iinfo(npdt).min, np.iinfo(npdt).max, n, endpoint=True).astype(npdt)
        s = pl.Series.from_numpy("x", v, valid)
        r = s.cum_sum()
        assert r.dtype is pl.Int64, name
        _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(v.astype(np.int64), valid, one, "sum"), ("sum", name))
        for kind in ("min", "max"):
            r = getattr(s, "cum_" + kind)()
            assert r.dtype is getattr(pl, name)
            _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(v, valid, one, kind), (kind, name))
    # UInt32 / UInt64 sums wrap at their own width
    v = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    r = pl.Series.from_numpy("x", v, valid).cum_sum()
    assert r.dtype is pl.UInt32
    _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(v, valid, one, "sum"), "sum UInt32")
    r = pl.Series.from_numpy("x", v, valid).cum_max()
    assert r.dtype is pl.UInt32
    _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(v, valid, one, "max"), "max UInt32")
    v = rng.integers(0, 2**64, n, dtype=np.uint64)
    r = pl.Series.from_numpy("x", v, valid).cum_sum()
    assert r.dtype is pl.UInt64
    _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(v, valid, one, "sum"), "sum UInt64")
    # UInt64 min / max order as unsigned: values on both sides of 2^63, 0 and 2^64 - 1
    v[[3, 40, 41]] = [2**63, 0, 2**64 - 1]
    st = np.zeros(n, bool)
    st[[0, 37, 300]] = True
    for kind in ("min", "max"):
        r = getattr(pl.Series.from_numpy("x", v, valid), "cum_" + kind)()
        assert r.dtype is pl.UInt64
        _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(v, valid, one, kind), (kind, "UInt64"))
        gv, gok = _cum(pl.Series.from_numpy("x", v, valid), kind, pl.Series.from_numpy("seg", st))
        _assert_same(gv, gok, *_ref(v, valid, _seg_info(st), kind), (kind, "UInt64 segmented"))
    # Boolean sums count as UInt32
    b = rng.random(n) < 0.4
    r = pl.Series.from_numpy("x", b, valid).cum_sum()
    assert r.dtype is pl.UInt32
    _assert_same(r.to_numpy(), r.validity_numpy(), np.cumsum(b & valid).astype(np.uint32), valid, "sum Boolean")
    # Float32 runs as Float64 and is rounded back
    f = (rng.standard_normal(n) * 100).astype(np.float32)
    r = pl.Series.from_numpy("x", f, valid).cum_sum()
    assert r.dtype is pl.Float32
    ev, _ = _ref(f.astype(np.float64), valid, one, "sum")
    _assert_same(r.to_numpy().astype(np.float64), r.validity_numpy(), ev.astype(np.float32).astype(np.float64),
                 valid, "sum Float32", bits=True)
    r = pl.Series.from_numpy("x", f, valid).cum_min()
    assert r.dtype is pl.Float32
    _assert_same(r.to_numpy(), r.validity_numpy(), *_ref(f, valid, one, "min"), "min Float32")
    # Duration keeps its unit; Datetime min / max keep the dtype
    d = rng.integers(-10**9, 10**9, n).astype("m8[us]")
    r = pl.Series.from_numpy("x", d, valid).cum_sum()
    assert r.dtype == pl.Duration("us")
    ev, _ = _ref(d.view(np.int64), valid, one, "sum")
    assert np.array_equal(r.to_numpy().view(np.int64)[valid], ev[valid])
    t = rng.integers(0, 10**15, n).astype("M8[ns]")
    r = pl.Series.from_numpy("x", t, valid).cum_max()
    assert r.dtype == pl.Datetime("ns")
    ev, _ = _ref(t.view(np.int64), valid, one, "max")
    assert np.array_equal(r.to_numpy().view(np.int64)[valid], ev[valid])
    with pytest.raises(pl.InvalidOperationError):
        pl.Series.from_numpy("x", t, valid).cum_sum()
    with pytest.raises(pl.InvalidOperationError):
        pl.Series.from_numpy("x", b, valid).cum_max()
    with pytest.raises(pl.InvalidOperationError):
        pl.Series("x", ["a", "b"]).cum_min()
    c = pl.Series("x", ["a", None, "b"]).cum_count()
    assert c.dtype is pl.UInt32 and c.to_list() == [1, 1, 2]


# ---------------------------------------------------------- number formats
def _format(form, n, rng):
    if form == "prices":
        return rng.uniform(100, 150, n) * np.exp(0.02 * rng.standard_normal(n))
    if form == "wide40":
        return rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))
    if form == "cancel":  # every even-length prefix cancels to +0.0
        a = rng.standard_normal((n + 1) // 2) * 1e3
        return np.stack([a, -a], 1).reshape(-1)[:n]
    if form == "negzero":
        return np.full(n, -0.0)
    if form == "subnormal":
        v = rng.integers(-2**20, 2**20, n).astype(np.float64) * 5e-324
        v[::97] = 2.0**-1000  # a few normal values next to them
        return v
    if form == "specials":  # NaN, then +inf and -inf at different rows of one segment; the next one clean
        v = rng.standard_normal(n)
        v[[T - 900, T - 600, T - 300]] = [np.inf, -np.inf, np.nan]
        v[[40, 90]] = [np.nan, np.inf]
        return v
    v = rng.uniform(1, 2, n) * 1e300  # "overflow": prefixes past the largest f64 round to inf and come back
    v[[50, 51, 52]] = 1.7e308
    v[[60, 61, 62]] = -1.7e308
    v[[T + 5, T + 6]] = -1.7e308
    v[[T + 9, T + 10]] = 1.7e308
    return v


@pytest.mark.parametrize("form", ["prices", "wide40", "cancel", "negzero", "subnormal", "specials", "overflow"])
def test_float_sum_formats(gpu, form):
    rng = np.random.default_rng(len(form))
    v = _format(form, NS, rng)
    valid = rng.random(NS) > 0.04
    if form in ("overflow", "specials"):
        valid[~np.isfinite(v) | (np.abs(v) > 1e308)] = True
    s = pl.Series.from_numpy("x", v, valid)
    exact = _ExactSums(v, valid)
    st = np.zeros(NS, bool)
    st[[0, T - 1000, T - 100, 2 * T + 17]] = True
    for name, starts in (("plain", None), ("segmented", st)):
        gv, gok = _cum(s, "sum", None if starts is None else pl.Series.from_numpy("seg", starts))
        first = np.zeros(NS, np.int64) if starts is None else _seg_info(starts)
        ev, eok = _ref(v, valid, first, "sum", exact)
        _assert_same(gv, gok, ev, eok, (form, name), bits=True)
        if form in ("cancel", "negzero"):
            z = gv[gok & (ev == 0)]
            assert z.size and not np.signbit(z).any(), form  # a zero sum is +0.0
        if form == "overflow":
            assert np.isinf(gv[gok]).any() and np.isfinite(gv[gok][-1])
        if form == "specials" and starts is not None:
            assert np.isfinite(gv[gok][-1])  # the segment after the non-finite ones is clean again


@pytest.mark.parametrize("form", ["prices", "wide40"])
def test_float_sum_against_the_sequential_fold(gpu, form):
    """|gpu - fold| <= i * 2^-53 * sum|x_j| + ulp(gpu) / 2: the bound of the
    reference's own f64 fold (DESIGN.md float-tolerance table)."""
    rng = np.random.default_rng(5)
    v = _format(form, NS, rng)
    gv, gok = _cum(pl.Series.from_numpy("x", v), "sum")
    assert gok.all()
    fold = np.array(list(itertools.accumulate(v.tolist())))
    sabs = np.cumsum(np.abs(v))
    i = np.arange(1, NS + 1)
    bound = i * 2.0**-53 * sabs + np.spacing(np.abs(gv)) / 2
    worst = np.max(np.abs(gv - fold) / bound)
    print(f"cum_sum vs sequential fold ({form}): worst error / bound = {worst:.3g}")
    assert (np.abs(gv - fold) <= bound).all()


def test_float_sum_span_refusal(gpu):
    v = np.ones(NS)
    v[T + 7] = 2.0**100
    s = pl.Series.from_numpy("x", v)
    with pytest.raises(pl.ComputeError) as ei:
        s.cum_sum()
    assert "span 100 binades" in str(ei.value) and "67" in str(ei.value)
    # exactly at the limit it runs, and the library still works afterwards
    v[T + 7] = 2.0**67
    gv, gok = _cum(pl.Series.from_numpy("x", v), "sum")
    _assert_same(gv, gok, *_ref(v, np.ones(NS, bool), np.zeros(NS, np.int64), "sum"), "span 67", bits=True)
    # zeros, nulls and non-finite values do not count towards the span
    v = np.array([0.0, 1e-300, np.inf, 1e300, 1e-300])
    valid = np.array([True, True, True, False, True])
    gv, gok = _cum(pl.Series.from_numpy("x", v, valid), "sum")
    assert gv[1] == 1e-300 and np.isinf(gv[2]) and np.isinf(gv[4]) and not gok[3]


# --------------------------------------------------------------- identities
def test_identity_with_rolling_sum(gpu):
    """cum_sum() == rolling_sum(n, min_samples=1) at every non-null row."""
    rng = np.random.default_rng(21)
    v = _format("wide40", NS, rng)
    valid = rng.random(NS) > 0.05
    s = pl.Series.from_numpy("x", v, valid)
    c, r = s.cum_sum(), s.rolling_sum(NS, min_samples=1)
    assert np.array_equal(c.validity_numpy(), valid)
    assert r.validity_numpy()[valid].all()
    assert np.array_equal(c.to_numpy()[valid].view(np.uint64), r.to_numpy()[valid].view(np.uint64))


def test_identity_with_sum_over(gpu):
    """The last non-null cum_sum().over(k) of a group == sum().over(k)."""
    rng = np.random.default_rng(22)
    n = 2 * T + 99
    k = rng.integers(0, 9, n).astype(np.int64)
    v = _format("wide40", n, rng)
    valid = rng.random(n) > 0.05
    df = pl.DataFrame([pl.Series.from_numpy("k", k), pl.Series.from_numpy("v", v, valid)])
    out = df.select(pl.col("v").cum_sum().over("k").alias("c"), pl.col("v").sum().over("k").alias("s"))
    c, s = out["c"].to_numpy(), out["s"].to_numpy()
    for g in range(9):
        rows = np.flatnonzero((k == g) & valid)
        assert rows.size
        assert c[rows[-1]].view(np.uint64) == s[rows[-1]].view(np.uint64), g


# ------------------------------------------------ more than one layer of totals
@pytest.mark.parametrize("dt", ["f64", "i64"])
def test_many_tiles(gpu, dt):
    """(1024 + 3) tiles: every thread of the totals scan owns more than one
    tile, and one segment is longer than 1024 tiles.  Integer-valued data in
    +-2^20: every prefix is exact in f64, so np.cumsum is the exact sum."""
    n = (1024 + 3) * T
    rng = np.random.default_rng(31)
    v = rng.integers(-2**20, 2**20, n)
    v = v.astype(np.float64) if dt == "f64" else v.astype(np.int64)
    s = pl.Series.from_numpy("x", v)
    valid = np.ones(n, bool)
    gv, gok = _cum(s, "sum")
    _assert_same(gv, gok, *_ref_exact_int(v, np.zeros(n, np.int64)), (dt, "plain"), bits=True)
    st = np.zeros(n, bool)
    st[[0, 5, T * 3 - 1, T * 1026 + 11, n - 2]] = True  # rows T*3-1 .. T*1026+10: > 1024 tiles
    gv, gok = _cum(s, "sum", pl.Series.from_numpy("seg", st))
    _assert_same(gv, gok, *_ref_exact_int(v, _seg_info(st)), (dt, "sparse"), bits=True)
    gv, gok = _cum(s, "max", pl.Series.from_numpy("seg", st))
    _assert_same(gv, gok, *_ref(v, valid, _seg_info(st), "max"), (dt, "max sparse"))


def _ref_exact_int(v, first):
    c = np.cumsum(v)
    before = np.where(first > 0, c[np.maximum(first - 1, 0)], 0).astype(v.dtype)
    return c - before, np.ones(v.shape[0], bool)


# --------------------------------------------------------- empty and trivial
@pytest.mark.parametrize("kind", ["sum", "min", "max", "count"])
def test_empty_and_trivial(gpu, kind):
    for dt in (np.float64, np.int64, np.int32):
        gv, gok = _cum(pl.Series.from_numpy("x", np.zeros(0, dt)), kind)
        assert gv.shape == (0,) and gok.shape == (0,)
        gv, gok = _cum(pl.Series.from_numpy("x", np.zeros(0, dt)), kind, pl.Series.from_numpy("s", np.zeros(0, bool)))
        assert gv.shape == (0,)
        one = np.array([7], dt)
        for seg in (None, pl.Series.from_numpy("s", np.ones(1, bool))):
            gv, gok = _cum(pl.Series.from_numpy("x", one), kind, seg)
            assert gok.all() and gv[0] == (1 if kind == "count" else 7)
        nul = np.zeros(130, bool)
        gv, gok = _cum(pl.Series.from_numpy("x", np.arange(130).astype(dt), nul), kind)
        if kind == "count":
            assert gok.all() and not gv.any()
        else:
            assert not gok.any()
    for op in ("shift", "diff"):
        gv, gok = _lag(pl.Series.from_numpy("x", np.zeros(0)), op, 1)
        assert gv.shape == (0,)
        gv, gok = _lag(pl.Series.from_numpy("x", np.array([3.0])), op, 1)
        assert not gok.any()
        gv, gok = _lag(pl.Series.from_numpy("x", np.array([3.0])), op, 0)
        assert gok.all() and gv[0] == (3.0 if op == "shift" else 0.0)


# --------------------------------------------------------------------- lag
_LAG_N = [0, 1, 2, 63, 64, 65, -1, -64, NS, NS + 5]


def _lag_values(dt, rng):
    if dt == "f64":
        v = rng.standard_normal(NS)
        v[[10, 11, 300, 301]] = [np.inf, np.inf, -np.inf, np.inf]  # inf - inf
        v[20] = np.frombuffer(np.uint64(0x7FF8_0000_DEAD_BEEF).tobytes(), np.float64)[0]  # a NaN payload
        return v
    if dt == "f32":
        v = rng.standard_normal(NS).astype(np.float32)
        v[[10, 11]] = np.inf
        return v
    if dt == "i64":
        v = rng.integers(-2**62, 2**62, NS, dtype=np.int64)
        v[[30, 31, 32]] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, np.iinfo(np.int64).min]
        return v
    if dt == "i32":
        v = rng.integers(-2**31, 2**31, NS).astype(np.int32)
        v[[30, 31, 32]] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min]
        return v
    return rng.integers(0, 2**32, NS, dtype=np.uint64).astype(np.uint32)


def _lag_ref(v, valid, first, op, n, fill=None):
    N_ = v.shape[0]
    i = np.arange(N_)
    src = i - n
    inb = (src >= 0) & (src < N_)
    sc = np.clip(src, 0, N_ - 1)
    inb &= first[sc] == first
    if op == "shift":
        ev = np.where(inb, v[sc], v.dtype.type(0) if fill is None else fill).astype(v.dtype)
        eok = np.where(inb, valid[sc], fill is not None)
        return ev, eok
    with np.errstate(over="ignore", invalid="ignore"):
        return (v - v[sc]).astype(v.dtype), inb & valid & valid[sc]


def _bits_of(x, dtype):
    u = np.array([x], dtype=dtype).view(np.uint64 if np.dtype(dtype).itemsize == 8 else np.uint32)[0]
    u = int(u)
    return u - (1 << 64) if u >= 1 << 63 else u


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32", "i64", "i32", "u32"])
def test_lag_kernel(gpu, dt, nullable):
    rng = np.random.default_rng(len(dt) + 40 + nullable)
    v = _lag_values(dt, rng)
    valid = rng.random(NS) > 0.07 if nullable else np.ones(NS, bool)
    s = pl.Series.from_numpy("x", v, valid if nullable else None)
    fill = v.dtype.type(7)
    layouts = [("plain", None, np.zeros(NS, np.int64))]
    for name, st in _placements(NS).items():
        layouts.append((name, pl.Series.from_numpy("seg", st), _seg_info(st)))
    for name, seg, first in layouts:
        for n in _LAG_N:
            gv, gok = _lag(s, "shift", n, seg)
            ev, eok = _lag_ref(v, valid, first, "shift", n)
            assert np.array_equal(gok, eok), (dt, name, n, "shift validity")
            assert gv[eok].tobytes() == ev[eok].tobytes(), (dt, name, n, "shift")  # bits: NaN payloads travel
            gv, gok = _lag(s, "shift", n, seg, _bits_of(fill, v.dtype))
            ev, eok = _lag_ref(v, valid, first, "shift", n, fill)
            assert np.array_equal(gok, eok), (dt, name, n, "fill validity")
            assert gv[eok].tobytes() == ev[eok].tobytes(), (dt, name, n, "fill")
            if dt == "u32":
                continue  # unsigned differences run as Int64 (below)
            gv, gok = _lag(s, "diff", n, seg)
            ev, eok = _lag_ref(v, valid, first, "diff", n)
            assert np.array_equal(gok, eok), (dt, name, n, "diff validity")
            g, e = gv[eok], ev[eok]
            if v.dtype.kind == "f":
                assert np.array_equal(np.isnan(g), np.isnan(e)), (dt, name, n)
                g, e = g[~np.isnan(e)], e[~np.isnan(e)]
            assert g.tobytes() == e.tobytes(), (dt, name, n, "diff")


def test_lag_of_a_sliced_input(gpu):
    rng = np.random.default_rng(50)
    full = rng.standard_normal(NS + 9)
    fvalid = rng.random(NS + 9) > 0.1
    s = pl.Series.from_numpy("x", full, fvalid).slice(3, NS)
    v, valid = full[3:3 + NS], fvalid[3:3 + NS]
    st = _placements(NS)["wave_word"]
    for seg, first in ((None, np.zeros(NS, np.int64)), (pl.Series.from_numpy("seg", st), _seg_info(st))):
        for n in (1, -1, 65):
            for op in ("shift", "diff"):
                gv, gok = _lag(s, op, n, seg)
                ev, eok = _lag_ref(v, valid, first, op, n)
                assert np.array_equal(gok, eok) and gv[eok].tobytes() == ev[eok].tobytes(), (op, n)


def test_lag_series_dtypes(gpu):
    rng = np.random.default_rng(51)
    n = 500
    one = np.zeros(n, np.int64)
    valid = rng.random(n) > 0.1
    # diff: UInt8 -> Int16, UInt16 -> Int32, UInt32 / UInt64 -> Int64; Int8 / Int16 wrap
    for npdt, out in ((np.uint8, "Int16"), (np.uint16, "Int32"), (np.uint32, "Int64")):
        v = rng.integers(0, np.iinfo(npdt).max, n, endpoint=True).astype(npdt)
        r = pl.Series.from_numpy("x", v, valid).diff(2)
        assert r.dtype is getattr(pl, out)
        ev, eok = _lag_ref(v.astype(np.int64), valid, one, "diff", 2)
        assert np.array_equal(r.validity_numpy(), eok)
        assert np.array_equal(r.to_numpy()[eok].astype(np.int64), ev[eok])
    v = rng.integers(-128, 127, n, endpoint=True).astype(np.int8)
    r = pl.Series.from_numpy("x", v, valid).diff()
    assert r.dtype is pl.Int8
    ev, eok = _lag_ref(v, valid, one, "diff", 1)
    assert np.array_equal(r.validity_numpy(), eok) and np.array_equal(r.to_numpy()[eok], ev[eok])
    r = pl.Series.from_numpy("x", v, valid).shift(-3, fill_value=5)
    assert r.dtype is pl.Int8
    ev, eok = _lag_ref(v, valid, one, "shift", -3, np.int8(5))
    assert np.array_equal(r.validity_numpy(), eok) and np.array_equal(r.to_numpy()[eok], ev[eok])
    # Datetime -> Duration of the same unit; shift keeps the logical dtype
    t = rng.integers(0, 10**15, n).astype("M8[ns]")
    s = pl.Series.from_numpy("t", t, valid)
    r = s.diff()
    assert r.dtype == pl.Duration("ns")
    ev, eok = _lag_ref(t.view(np.int64), valid, one, "diff", 1)
    assert np.array_equal(r.validity_numpy(), eok) and np.array_equal(r.to_numpy().view(np.int64)[eok], ev[eok])
    assert s.shift(1).dtype == pl.Datetime("ns")
    f = pl.Series.from_numpy("x", np.arange(5.0)).shift(2, fill_value=pl.lit(-1.5))
    assert f.to_list() == [-1.5, -1.5, 0.0, 1.0, 2.0]
    assert pl.Series.from_numpy("x", np.arange(5.0)).shift(np.int64(2)).to_list() == [None, None, 0.0, 1.0, 2.0]
    # a literal null n: every row null, the fill ignored (test_shift.py:124)
    i32 = pl.Series.from_numpy("x", np.array([1, 2, 3], np.int32))
    for r in (i32.shift(None), i32.shift(None, fill_value=1)):
        assert r.dtype is pl.Int32 and r.to_list() == [None, None, None]
    assert pl.Series.from_numpy("x", np.zeros(0)).shift(None).len() == 0
    for bad in (pl.Series("x", [True, False]), pl.Series("x", ["a", "b"])):
        for call in (lambda q: q.shift(1), lambda q: q.diff()):
            with pytest.raises(pl.InvalidOperationError):
                call(bad)
    with pytest.raises(pl.InvalidOperationError):
        pl.Series.from_numpy("x", np.arange(5.0)).diff(1, "drop")


# ------------------------------------------------------------------ golden
def _golden_value(x):
    return {"inf": math.inf, "-inf": -math.inf, "nan": math.nan}.get(x, x) if isinstance(x, str) else x


@pytest.mark.parametrize("case", load_golden("cumulative_cases.json")["cases"], ids=lambda c: c["name"])
def test_golden_cases(gpu, case):
    dt = getattr(pl, case["dtype"])
    vals = [_golden_value(x) for x in case["values"]]
    valid = np.array([x is not None for x in vals])
    arr = np.array([0 if x is None else x for x in vals], dtype=dt.np_dtype)
    s = pl.Series.from_numpy("a", arr, None if valid.all() else valid)
    if case["op"].startswith("cum_"):
        f = getattr(pl.col("a"), case["op"])()
    elif case["op"] == "shift":
        f = pl.col("a").shift(case["n"], fill_value=case.get("fill_value"))
    else:
        f = pl.col("a").diff(case["n"])
    cols = [s]
    if "keys" in case:
        cols.append(pl.Series("k", case["keys"]))
        f = f.over("k")
    out = pl.DataFrame(cols).select(f)["a"]
    assert out.dtype is getattr(pl, case["expected_dtype"]), case["name"]
    exp = [_golden_value(x) for x in case["expected"]]
    got = out.to_list()
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        if e is None or g is None:
            assert g is None and e is None, (case["name"], got)
        elif isinstance(e, float) and math.isnan(e):
            assert math.isnan(g)
        elif isinstance(e, float):
            assert math.isclose(g, e, rel_tol=1e-6), (case["name"], got)  # Float32 cases; 1.3 + 2.4 as written
        else:
            assert g == e, (case["name"], got)


# -------------------------------------------------------------- end to end
def _bars(rng, n, nsym=7):
    sym = np.sort(rng.integers(0, nsym + 1, n)).astype(np.int64)  # symbol 0 stands for the null key
    kvalid = sym != 0
    close = rng.uniform(100, 150, n) * np.exp(0.02 * rng.standard_normal(n))
    high = close * rng.uniform(1.0, 1.02, n)
    volume = rng.integers(1, 10**6, n).astype(np.int64)
    cvalid = rng.random(n) > 0.03
    return sym, kvalid, close, cvalid, high, volume


def _bars_frame(sym, kvalid, close, cvalid, high, volume, order=None):
    o = np.arange(sym.shape[0]) if order is None else order
    return pl.DataFrame([pl.Series.from_numpy("symbol", sym[o], kvalid[o]),
                         pl.Series.from_numpy("close", close[o], cvalid[o]),
                         pl.Series.from_numpy("high", high[o]), pl.Series.from_numpy("volume", volume[o])])


def test_end_to_end_over_symbol(gpu, plgpu_option):
    rng = np.random.default_rng(61)
    n = 2 * T + 51
    sym, kvalid, close, cvalid, high, volume = _bars(rng, n)
    exprs = [(pl.col("close") / pl.col("close").shift(1).over("symbol") - 1).alias("ret"),
             pl.col("volume").cum_sum().over("symbol").alias("vol"),
             pl.col("high").cum_max().over("symbol").alias("hi")]
    # the per-group numpy reference (rows in sorted layout: every group contiguous)
    first = _seg_info(np.append(True, sym[1:] != sym[:-1]))
    prev, pok = _lag_ref(close, cvalid, first, "shift", 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        e_ret, e_rok = close / prev - 1, cvalid & pok
    e_vol, _ = _ref(volume, np.ones(n, bool), first, "sum")
    e_hi, _ = _ref(high, np.ones(n, bool), first, "max")

    def check(out, pos, what):
        r = out["ret"]
        assert np.array_equal(r.validity_numpy()[pos], e_rok), what
        assert np.array_equal(r.to_numpy()[pos][e_rok].view(np.uint64), e_ret[e_rok].view(np.uint64)), what
        assert out["vol"].dtype is pl.Int64 and np.array_equal(out["vol"].to_numpy()[pos], e_vol), what
        assert np.array_equal(out["hi"].to_numpy()[pos], e_hi), what

    plgpu_option("ktime", 1)
    df_sorted = _bars_frame(sym, kvalid, close, cvalid, high, volume)
    N.ktime_read()
    out_sorted = df_sorted.with_columns(*exprs)
    kt = N.ktime_read()
    assert out_sorted.columns == ["symbol", "close", "high", "volume", "ret", "vol", "hi"]
    assert not [k for k in kt if k.startswith("srt_")], kt
    assert kt["seg_starts_kernel"][1] == 1, kt  # the three nodes share the segment cache
    assert kt["lag_seg_kernel"][1] == 1 and kt["cum_apply_kernel"][1] == 2, kt
    check(out_sorted, np.arange(n), "sorted")
    # interleaved: a shuffle that keeps every group's rows in their relative order
    labels = rng.permutation(sym)
    pos = np.empty(n, np.int64)
    for g in np.unique(sym):
        pos[np.flatnonzero(sym == g)] = np.flatnonzero(labels == g)
    order = np.argsort(pos)
    N.ktime_read()
    out_shuf = _bars_frame(sym, kvalid, close, cvalid, high, volume, order).with_columns(*exprs)
    kt = N.ktime_read()
    assert [k for k in kt if k.startswith("srt_")] and kt["invert_perm_kernel"][1] == 1, kt
    check(out_shuf, pos, "interleaved")
    plgpu_option("over_presorted", 0)
    N.ktime_read()
    out_forced = df_sorted.with_columns(*exprs)
    kt = N.ktime_read()
    assert [k for k in kt if k.startswith("srt_")], kt
    for nm in ("ret", "vol", "hi"):
        assert np.array_equal(out_forced[nm].validity_numpy(), out_sorted[nm].validity_numpy())
        ok = out_sorted[nm].validity_numpy()
        assert out_forced[nm].to_numpy()[ok].tobytes() == out_sorted[nm].to_numpy()[ok].tobytes(), nm


def test_end_to_end_keys_and_composition(gpu):
    import pyarrow as pa

    rng = np.random.default_rng(62)
    n = 3000
    sym = rng.integers(0, 5, n).astype(np.int64)
    day = rng.integers(0, 3, n).astype(np.int32)
    x = rng.integers(-1000, 1000, n).astype(np.int64)
    f = rng.standard_normal(n)
    names = np.array(["aapl", "msft", "amd", "nvda", "tsm"], dtype=object)
    cat = pl.Series.from_arrow("cat", pa.array(names[sym].tolist(), pa.string()).dictionary_encode())
    df = pl.DataFrame([pl.Series.from_numpy("symbol", sym), pl.Series.from_numpy("day", day),
                       pl.Series.from_numpy("x", x), pl.Series.from_numpy("f", f), cat])
    out = df.select(pl.col("x").cum_sum().over("symbol", "day").alias("two"),
                    pl.col("x").diff().over("cat").alias("bycat"),
                    pl.col("x").cum_count().over("cat").alias("cnt"),
                    (pl.col("f") - pl.col("f").shift(1)).alias("plain"),
                    pl.col("x").shift(1).cum_sum().alias("composed"),
                    (pl.col("x") * 2).cum_min().alias("expr"))
    e_two = np.zeros(n, np.int64)
    for s_ in range(5):
        for d_ in range(3):
            rows = np.flatnonzero((sym == s_) & (day == d_))
            e_two[rows] = np.cumsum(x[rows])
    assert np.array_equal(out["two"].to_numpy(), e_two)
    e_d, e_dok, e_c = np.zeros(n, np.int64), np.zeros(n, bool), np.zeros(n, np.uint32)
    for s_ in range(5):
        rows = np.flatnonzero(sym == s_)
        e_d[rows[1:]], e_dok[rows[1:]] = np.diff(x[rows]), True
        e_c[rows] = np.arange(1, rows.size + 1)
    assert np.array_equal(out["bycat"].validity_numpy(), e_dok)
    assert np.array_equal(out["bycat"].to_numpy()[e_dok], e_d[e_dok])
    assert out["cnt"].dtype is pl.UInt32 and np.array_equal(out["cnt"].to_numpy(), e_c)
    p = out["plain"]
    assert not p.validity_numpy()[0] and p.validity_numpy()[1:].all()
    assert np.array_equal(p.to_numpy()[1:].view(np.uint64), (f[1:] - f[:-1]).view(np.uint64))
    c = out["composed"]
    assert not c.validity_numpy()[0] and np.array_equal(c.to_numpy()[1:], np.cumsum(x[:-1]))
    assert np.array_equal(out["expr"].to_numpy(), np.minimum.accumulate(x * 2))
    with pytest.raises(pl.InvalidOperationError) as ei:
        df.group_by("symbol").agg(pl.col("x").cum_sum())
    assert "not an aggregation" in str(ei.value)


def test_plugin_window_cum_sum_runs(gpu):
    from test_polars_engine import FakeNT, FakePolarsDF, PyExprIR, _table

    table, k, v, w, vvalid = _table(5000, 4)
    nt = FakeNT(table)
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(table), projection=None, selection=None)
    fn = nt.e("Function", function_data=("cum_sum", False), input=[nt.col("w")], options=None)
    win = nt.e("Window", function=fn, partition_by=[nt.col("k")], order_by=None, order_by_descending=False,
               order_by_nulls_last=False, options=type("WindowMapping", (), {"kind": "groups_to_rows"})())
    sh = nt.e("Function", function_data=("shift_and_fill",), input=[nt.col("v"), nt.lit(1), nt.lit(0.0)],
              options=None)
    nt.p("HStack", ["k", "v", "w", "cw", "pv"], input=scan, exprs=[PyExprIR(win, "cw"), PyExprIR(sh, "pv")])
    PE.execute_with_polaroid(nt, None, to_frame=lambda t: t)
    assert callable(nt.udf)
    out = nt.udf(None, None, None, False)
    assert out.column_names == ["k", "v", "w", "cw", "pv"]
    exp = np.zeros(5000, np.int64)
    for g in np.unique(k):
        rows = np.flatnonzero(k == g)
        exp[rows] = np.cumsum(w[rows])
    assert out.column("cw").to_pylist() == exp.tolist()
    pv = out.column("pv").to_pylist()
    assert pv[0] == 0.0
    assert pv[1:] == [x if ok else None for x, ok in zip(v[:-1].tolist(), vvalid[:-1].tolist())]
