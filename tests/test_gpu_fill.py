"""GPU: forward / backward fill (plgpu_fill) at the seams of its three launches,
the fill_null strategies, and both end to end, plain and over groups.

Reference.  `_ref_idx` restates the index loops of the reference's
fill_forward_gather_limit / fill_backward_gather_limit
(polars-core/src/chunked_array/ops/fill_null.rs:258 / :304), applied per
segment; the expected column is the input gathered by those indices.  Every
comparison is bit for bit: validity first, then the values of the valid rows
viewed as unsigned integers of their width.  There is no tolerance.  For
min / max / mean the expected fill value is this library's own select(agg)
result (int() of it for an integer mean)."""

import ctypes as C

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from polaroid_amd import _native as N
from polaroid_amd import polars_engine as PE

pytestmark = pytest.mark.gpu

T = N.CUM_TILE    # rows of one workgroup of the fill kernels: one summary, one carry
B = N.CUM_BLOCK   # rows of one pass of a workgroup over the values
NS = 3 * T + 5
LENGTHS = [0, 1, 63, 64, 65, B - 1, B, B + 1, T - 1, T, T + 1, NS]
LIMITS = [None, 0, 1, 2, 63, 64, 65, T, T + 1, "n", "n+5"]
_UINT = {4: np.uint32, 8: np.uint64}


# ------------------------------------------------------------------ reference
def _ref_idx(valid, limit, rev):
    """fill_forward_gather_limit / fill_backward_gather_limit: the row every
    row gathers (a limit of None: the column's length)."""
    n = len(valid)
    lim = n if limit is None else limit
    out = list(range(n))
    last, cnt = (n - 1 if rev else 0), 0
    for i in (range(n - 1, -1, -1) if rev else range(n)):
        if valid[i]:
            last, cnt = i, 0
        elif cnt < lim:
            cnt += 1
            out[i] = last
    return out


def _ref(vals, valid, op, limit=None, starts=None):
    """Expected (values, validity) of a forward / backward fill per segment."""
    n = len(valid)
    rev = op == "backward"
    if starts is None or n == 0:
        bounds = [0, n]
    else:
        st = np.asarray(starts).copy()
        st[0] = True
        bounds = np.flatnonzero(st).tolist() + [n]
    vl = np.asarray(valid).tolist()
    idx = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        idx.extend(a + j for j in _ref_idx(vl[a:b], limit, rev))
    idx = np.asarray(idx, dtype=np.int64)
    return vals[idx], np.asarray(valid)[idx]


def _limit(limit, n):
    return {"n": n, "n+5": n + 5}.get(limit, limit) if isinstance(limit, str) else limit


def _fill(s, op, limit=None, seg=None):
    out = N.Column()
    N.check(N.lib().plgpu_fill(C.byref(s._col), None if seg is None else C.byref(seg._col), N.FILL[op],
                               -1 if limit is None else limit, C.byref(out), None))
    r = pl.Series._from_native("x", out)
    return r.to_numpy(), r.validity_numpy()


def _same(got, exp, what):
    gv, gok = got
    ev, eok = exp
    assert gv.shape == ev.shape and np.array_equal(gok, eok), (what, np.flatnonzero(gok != eok)[:8])
    u = _UINT[ev.dtype.itemsize]
    a, b = gv[eok].view(u), ev[eok].view(u)
    assert np.array_equal(a, b), (what, np.flatnonzero(a != b)[:8])


def _values(n, dtype=np.float64, seed=0):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype).kind == "f":
        return rng.standard_normal(n).astype(dtype)
    return rng.integers(-2**31, 2**31 - 1, n).astype(dtype)


def _patterns(n, rng):
    """Null patterns: {name: validity array}."""
    def only(rows):
        v = np.zeros(n, bool)
        v[[r for r in rows if 0 <= r < n]] = True
        return v

    first_null = np.ones(n, bool)
    first_null[:1] = False
    run = np.ones(n, bool)
    run[min(5, n):2 * T + 9] = False  # one null run from tile 0 into tile 2
    return {
        "all_valid": np.ones(n, bool),
        "all_null": np.zeros(n, bool),
        "only_row0": only([0]),
        "only_last": only([n - 1]),
        "first_null": first_null,
        "alternating": np.arange(n) % 2 == 0,
        "alternating_odd": np.arange(n) % 2 == 1,
        "random_50": rng.random(n) >= 0.5,
        "random_99": rng.random(n) >= 0.99,
        "long_run": run,
    }


# ---------------------------------------------------------------------- seams
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_null_patterns(gpu, n):
    rng = np.random.default_rng(n)
    vals = _values(n, seed=n)
    for name, valid in _patterns(n, rng).items():
        s = pl.Series.from_numpy("x", vals, valid)
        for op in ("forward", "backward"):
            for limit in (None, 1):
                _same(_fill(s, op, limit), _ref(vals, valid, op, limit), (n, name, op, limit))


def test_no_validity_buffer_is_returned_as_it_is(gpu, plgpu_option):
    vals = _values(B + 1)
    s = pl.Series.from_numpy("x", vals)
    plgpu_option("ktime", 1)
    N.ktime_read()
    for r in (s.forward_fill(), s.backward_fill(3), s.fill_null(strategy="forward", limit=1)):
        assert int(r._col.values) == int(s._col.values) and not r._col.validity
        assert np.array_equal(r.to_numpy().view(np.uint64), vals.view(np.uint64))
    # the entry point itself copies the values, without a kernel
    gv, gok = _fill(s, "forward")
    assert gok.all() and np.array_equal(gv.view(np.uint64), vals.view(np.uint64))
    assert not [k for k in N.ktime_read() if k.startswith("fill_")]


@pytest.mark.parametrize("limit", LIMITS, ids=[str(x) for x in LIMITS])
def test_limits(gpu, limit):
    n = NS
    lim = _limit(limit, n)
    rng = np.random.default_rng(7)
    vals = _values(n, seed=7)
    pats = _patterns(n, rng)
    cases = {k: pats[k] for k in ("random_50", "random_99", "only_row0", "only_last", "long_run")}
    if lim is not None and 0 < lim < B:
        # null runs of exactly limit and limit + 1 rows that straddle a word, a block and a tile boundary
        for length in (lim, lim + 1):
            v = np.ones(n, bool)
            for seam in (3 * 64, 9 * 64, B, 3 * B, T, 2 * T):
                at = seam - (length + 1) // 2
                v[at:at + length] = False
            cases[f"runs_of_{length}_at_seams"] = v
    for name, valid in cases.items():
        s = pl.Series.from_numpy("x", vals, valid)
        for op in ("forward", "backward"):
            _same(_fill(s, op, lim), _ref(vals, valid, op, lim), (name, op, lim))


def _placements(n, rng):
    def at(rows):
        st = np.zeros(n, bool)
        st[[r for r in rows if 0 <= r < n]] = True
        return st

    return {
        "word_seams": at([0, 63, 64, 65, 127, 128, 129, T + 63, T + 64, 2 * T + 1, n - 1]),
        "block_seams": at([0, B - 1, B, B + 1, 3 * B, 5 * B - 1, T + 2 * B, T + 7 * B - 1, 2 * T + B + 3]),
        "tile_seams": at([0, T - 1, T, T + 1, 2 * T - 1, 2 * T, 3 * T, 3 * T + 1]),
        "random_1pct": np.append(True, rng.random(n - 1) < 0.01),
    }


@pytest.mark.parametrize("place", ["word_seams", "block_seams", "tile_seams", "random_1pct"])
def test_segments(gpu, place):
    n = NS
    rng = np.random.default_rng(11)
    vals = _values(n, seed=11)
    starts = _placements(n, rng)[place]
    seg = pl.Series.from_numpy("seg", starts)
    pats = _patterns(n, rng)
    for name in ("random_50", "random_99", "only_row0", "only_last", "all_null", "long_run"):
        valid = pats[name]
        s = pl.Series.from_numpy("x", vals, valid)
        for op in ("forward", "backward"):
            for limit in (None, 2, T + 1):
                _same(_fill(s, op, limit, seg), _ref(vals, valid, op, limit, starts), (place, name, op, limit))


def test_segment_identities(gpu):
    n = NS
    rng = np.random.default_rng(12)
    vals = _values(n, seed=12)
    valid = rng.random(n) >= 0.6
    s = pl.Series.from_numpy("x", vals, valid)
    row0 = np.zeros(n, bool)
    row0[0] = True
    every = np.ones(n, bool)
    for op in ("forward", "backward"):
        for limit in (None, 3):
            plain = _fill(s, op, limit)
            got = _fill(s, op, limit, pl.Series.from_numpy("seg", row0))
            assert np.array_equal(got[1], plain[1])
            assert got[0].tobytes() == plain[0].tobytes()  # bit 0 only: the NULL-bitmap call, every byte
            _same(_fill(s, op, limit, pl.Series.from_numpy("seg", every)), (vals, valid), (op, limit, "every"))


@pytest.mark.parametrize("at", [5, 63, 64, B - 1, B, T - 1, T, 2 * T + 1])
def test_nulls_next_to_a_start_stay_null(gpu, at):
    """A start directly after a valid row, followed by nulls: they belong to the
    new segment and stay null; the mirror image for backward."""
    n = NS
    vals = _values(n, seed=13)
    valid = np.zeros(n, bool)
    valid[at - 1] = True                    # forward: the valid row ends a segment
    starts = np.zeros(n, bool)
    starts[[0, at]] = True
    s, seg = pl.Series.from_numpy("x", vals, valid), pl.Series.from_numpy("seg", starts)
    gv, gok = _fill(s, "forward", None, seg)
    assert gok.sum() == 1 and gok[at - 1]
    _same((gv, gok), _ref(vals, valid, "forward", None, starts), at)
    valid = np.zeros(n, bool)
    valid[at] = True                        # backward: the valid row starts a segment
    s = pl.Series.from_numpy("x", vals, valid)
    gv, gok = _fill(s, "backward", None, seg)
    assert gok.sum() == 1 and gok[at]
    _same((gv, gok), _ref(vals, valid, "backward", None, starts), at)
    # and within one segment they are filled
    starts2 = np.zeros(n, bool)
    starts2[0] = True
    seg2 = pl.Series.from_numpy("seg", starts2)
    assert _fill(s, "backward", None, seg2)[1][:at + 1].all()


@pytest.mark.parametrize("off", [1, 3, 63, 65, 9])
@pytest.mark.parametrize("np_dtype", [np.float64, np.int32])
def test_slices(gpu, off, np_dtype):
    """A row offset: the validity and the start bits begin inside a word, and
    the values are not 16-byte aligned."""
    n = 2 * T + 77
    rng = np.random.default_rng(off)
    vals = _values(n + off, np_dtype, seed=off)
    valid = rng.random(n + off) >= 0.7
    starts = rng.random(n + off) < 0.01
    s = pl.Series.from_numpy("x", vals, valid).slice(off, n)
    seg = pl.Series.from_numpy("seg", starts).slice(off, n)
    st = starts[off:].copy()
    st[0] = True
    for op in ("forward", "backward"):
        for limit in (None, 4):
            _same(_fill(s, op, limit), _ref(vals[off:], valid[off:], op, limit), (off, op, limit))
            _same(_fill(s, op, limit, seg), _ref(vals[off:], valid[off:], op, limit, st), (off, op, limit, "seg"))


def test_bitmaps_at_odd_addresses(gpu):
    """Borrowed bitmaps that are not 8-byte aligned and not padded to a word."""
    n = T + 77
    rng = np.random.default_rng(17)
    vals = _values(n, seed=17)
    valid = rng.random(n) >= 0.6
    starts = np.append(True, rng.random(n - 1) < 0.01)
    base = pl.Series.from_numpy("x", vals)

    def odd(mask):
        bits = np.packbits(mask, bitorder="little")
        buf = N.DeviceBuffer(bits.nbytes + 1)
        N.check(N.lib().plgpu_memcpy_h2d(C.c_void_p(buf.ptr + 1), bits.ctypes.data_as(C.c_void_p), bits.nbytes, None))
        return buf

    vbuf, sbuf = odd(valid), odd(starts)
    s = pl.Series.from_device("x", pl.Float64, int(base._col.values), n, validity_ptr=vbuf.ptr + 1,
                              keepalive=(base, vbuf))
    seg = pl.Series.from_device("seg", pl.Boolean, sbuf.ptr + 1, n, keepalive=sbuf)
    for op in ("forward", "backward"):
        _same(_fill(s, op, 3), _ref(vals, valid, op, 3), op)
        _same(_fill(s, op, None, seg), _ref(vals, valid, op, None, starts), (op, "seg"))


def test_many_tiles(gpu):
    """More tiles than the totals launch has threads.  (Limit None: the index
    loop's result is the running maximum / minimum of the valid row indices,
    taken here with numpy at this size.)"""
    n = 1025 * T + 3
    rng = np.random.default_rng(5)
    vals = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    valid = rng.random(n) < 1.0 / 40000  # runs that cross several tiles
    valid[3] = True
    s = pl.Series.from_numpy("x", vals, valid)
    rows = np.arange(n, dtype=np.int64)
    j = np.maximum.accumulate(np.where(valid, rows, -1))
    gv, gok = _fill(s, "forward")
    assert np.array_equal(gok, j >= 0) and np.array_equal(gv[gok], vals[j[gok]])
    j = np.minimum.accumulate(np.where(valid, rows, n)[::-1])[::-1]
    gv, gok = _fill(s, "backward")
    assert np.array_equal(gok, j < n) and np.array_equal(gv[gok], vals[j[gok]])


# --------------------------------------------------------------------- dtypes
_DTYPES = [pl.Int8, pl.Int16, pl.Int32, pl.Int64, pl.UInt8, pl.UInt16, pl.UInt32, pl.UInt64, pl.Float32, pl.Float64,
           pl.Date, pl.Datetime("ns"), pl.Datetime("ms"), pl.Duration("us")]


@pytest.mark.parametrize("dt", _DTYPES, ids=[str(d).split("(")[0] + str(i) for i, d in enumerate(_DTYPES)])
def test_every_dtype_once(gpu, dt):
    n = B + 1
    rng = np.random.default_rng(21)
    npd = np.dtype(dt.np_dtype)
    if npd.kind == "f":
        vals = rng.standard_normal(n).astype(npd)
    else:
        info = np.iinfo(npd)
        vals = rng.integers(info.min, info.max, n, dtype=npd, endpoint=True)
    valid = rng.random(n) >= 0.5
    s = pl.Series.from_numpy("x", vals, valid, dtype=dt)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[npd.itemsize]
    for r, op, limit in ((s.forward_fill(), "forward", None), (s.backward_fill(2), "backward", 2),
                         (s.fill_null(strategy="forward", limit=1), "forward", 1)):
        assert r.dtype == dt and r.name == "x", (r.dtype, dt)
        ev, eok = _ref(vals, valid, op, limit)
        assert np.array_equal(r.validity_numpy(), eok)
        assert np.array_equal(r.to_numpy().view(u)[eok], ev.view(u)[eok])


def test_bits_are_moved(gpu):
    bits = np.array([0x7FF8000000000123, 0, 0, 0x8000000000000000, 0, 0xFFF0000000000001, 0, 0x7FF0000000000000],
                    np.uint64)
    valid = np.array([1, 0, 0, 1, 0, 1, 0, 1], bool)
    s = pl.Series.from_numpy("x", bits.view(np.float64), valid)
    f = s.forward_fill().to_numpy().view(np.uint64)
    assert f.tolist() == [bits[0], bits[0], bits[0], bits[3], bits[3], bits[5], bits[5], bits[7]]
    b = s.backward_fill().to_numpy().view(np.uint64)
    assert b.tolist() == [bits[0], bits[3], bits[3], bits[3], bits[5], bits[5], bits[7], bits[7]]
    b32 = np.array([0x7FC00123, 0, 0x80000000, 0], np.uint32)
    s32 = pl.Series.from_numpy("x", b32.view(np.float32), np.array([1, 0, 1, 0], bool))
    r = s32.forward_fill()
    assert r.dtype is pl.Float32 and r.to_numpy().view(np.uint32).tolist() == [b32[0], b32[0], b32[2], b32[2]]


def test_categorical_and_refusals(gpu):
    import pyarrow as pa

    words = ["b", None, None, "a", None, "c", None]
    cat = pl.Series.from_arrow("cat", pa.array(words, pa.string()).dictionary_encode())
    dictionary = cat._cat_codes()[0]
    f = cat.forward_fill(1)
    assert f._cat_codes() is not None and f._cat_codes()[0] is dictionary
    assert f.to_list() == ["b", "b", None, "a", "a", "c", "c"]
    b = pl.DataFrame([cat]).select(pl.col("cat").backward_fill())["cat"]
    assert b._cat_codes() is not None and b.to_list() == ["b", "a", "a", "a", "c", "c", None]
    for bad in (pl.Series("x", [True, None, False]), pl.Series("x", ["a", None, "b"])):
        for call in (lambda q: q.forward_fill(), lambda q: q.backward_fill(1),
                     lambda q: q.fill_null(strategy="min"), lambda q: q.fill_null(strategy="zero")):
            with pytest.raises(pl.InvalidOperationError) as ei:
                call(bad)
            assert "not supported" in str(ei.value)
    x = pl.Series("x", [1.0, None])
    with pytest.raises(pl.InvalidOperationError):
        x.forward_fill(-1)
    with pytest.raises(ValueError):
        x.fill_null(1.0, strategy="forward")
    with pytest.raises(ValueError):
        x.fill_null(strategy="max", limit=1)
    with pytest.raises(ValueError):
        x.fill_null(strategy="nearest")
    with pytest.raises(pl.InvalidOperationError):
        x.fill_null()
    with pytest.raises(pl.InvalidOperationError):
        pl.Series.from_numpy("t", np.array([1, 2], np.int64), np.array([1, 0], bool),
                             dtype=pl.Datetime("us")).fill_null(strategy="mean")


# ----------------------------------------------------------------- identities
def test_identities(gpu):
    n = NS
    rng = np.random.default_rng(31)
    vals = _values(n, seed=31)
    valid = rng.random(n) >= 0.8
    valid[:700] = False
    valid[700] = True  # 700 leading nulls exactly
    s = pl.Series.from_numpy("x", vals, valid)
    r = pl.Series.from_numpy("x", vals[::-1].copy(), valid[::-1].copy())
    for limit in (None, 0, 5, 64, T):
        bv, bok = _fill(s, "backward", limit)
        fv, fok = _fill(r, "forward", limit)
        assert np.array_equal(bok, fok[::-1])
        assert np.array_equal(bv[bok].view(np.uint64), fv[::-1][bok].view(np.uint64))
    assert s.forward_fill().null_count() == 700
    a, b = s.forward_fill(limit=n), s.forward_fill()
    assert np.array_equal(a.validity_numpy(), b.validity_numpy())
    assert a.to_numpy().tobytes() == b.to_numpy().tobytes()
    # limit 0 fills nothing
    z = s.forward_fill(0)
    assert np.array_equal(z.validity_numpy(), valid)


# ------------------------------------------------------------------ strategies
def _agg_of(s, op):
    return pl.DataFrame([s]).select(getattr(pl.col(s.name), op)())[s.name].to_list()[0]


@pytest.mark.parametrize("dt", [pl.Float64, pl.Int64, pl.Int32])
def test_strategies_plain(gpu, dt):
    n = B + 7
    rng = np.random.default_rng(41)
    vals = (rng.standard_normal(n) * 100).astype(dt.np_dtype)
    valid = rng.random(n) >= 0.3
    s = pl.Series.from_numpy("x", vals, valid, dtype=dt)
    for op in ("zero", "one", "min", "max", "mean"):
        fill = {"zero": 0, "one": 1}.get(op)
        if fill is None:
            fill = _agg_of(s, op)
            if dt is not pl.Float64:
                fill = int(fill)
        exp = np.where(valid, vals, np.array(fill, dtype=dt.np_dtype))
        for r in (s.fill_null(strategy=op), pl.DataFrame([s]).select(pl.col("x").fill_null(strategy=op))["x"]):
            assert r.dtype is dt and r.null_count() == 0, (op, r.dtype)
            assert r.to_numpy().tobytes() == exp.tobytes(), op
    # the integer mean is truncated toward zero (fill_null.rs:210)
    assert pl.Series("x", [1, None, 2]).fill_null(strategy="mean").to_list() == [1, 1, 2]
    assert pl.Series("x", [-1, None, -2]).fill_null(strategy="mean").to_list() == [-1, -1, -2]
    # an all-null column: zero / one fill it, min / max / mean leave it as it is
    e = pl.Series.from_numpy("x", np.zeros(5, dt.np_dtype), np.zeros(5, bool), dtype=dt)
    assert e.fill_null(strategy="zero").to_list() == [0] * 5 and e.fill_null(strategy="one").to_list() == [1] * 5
    for op in ("min", "max", "mean"):
        r = e.fill_null(strategy=op)
        assert r.dtype is dt and r.to_list() == [None] * 5
    # the narrow, the unsigned 64-bit and the single-precision dtypes keep their dtype
    big = 2**63 + 5
    u = pl.Series.from_numpy("x", np.array([big, 0, 1], np.uint64), np.array([1, 0, 1], bool))
    assert u.fill_null(strategy="max").dtype is pl.UInt64 and u.fill_null(strategy="max").to_list() == [big, big, 1]
    assert u.fill_null(strategy="zero").to_list() == [big, 0, 1]
    i8 = pl.Series.from_numpy("x", np.array([3, 0, -7], np.int8), np.array([1, 0, 1], bool))
    assert i8.fill_null(strategy="min").dtype is pl.Int8 and i8.fill_null(strategy="min").to_list() == [3, -7, -7]
    f32 = pl.Series.from_numpy("x", np.array([1.5, 0], np.float32), np.array([1, 0], bool))
    assert f32.fill_null(strategy="one").dtype is pl.Float32 and f32.fill_null(strategy="one").to_list() == [1.5, 1.0]
    d = pl.Series.from_numpy("t", np.array([5, 0, 9], np.int64), np.array([1, 0, 1], bool), dtype=pl.Datetime("us"))
    r = d.fill_null(strategy="max")
    assert r.dtype == pl.Datetime("us") and r.to_numpy().tolist() == [5, 9, 9]


def test_strategies_over(gpu):
    k = np.array([2, 1, 2, 1, 3, 3, 2, 1, 4], np.int64)
    kvalid = np.array([1, 1, 1, 1, 1, 1, 1, 1, 0], bool)
    x = np.array([1.0, 0, 5.0, 4.0, 0, 0, 0, 8.0, 0])
    xvalid = np.array([1, 0, 1, 1, 0, 0, 0, 1, 0], bool)  # group 3 and the null key's group are all null
    i = np.array([7, 0, -4, 3, 0, 0, 0, 4, 0], np.int64)
    df = pl.DataFrame([pl.Series.from_numpy("k", k, kvalid), pl.Series.from_numpy("x", x, xvalid),
                       pl.Series.from_numpy("i", i, xvalid)])
    out = df.select(*[pl.col("x").fill_null(strategy=op).over("k").alias(op)
                      for op in ("min", "max", "mean", "zero", "one")],
                    pl.col("i").fill_null(strategy="mean").over("k").alias("imean"))
    assert out["min"].to_list() == [1.0, 4.0, 5.0, 4.0, None, None, 1.0, 8.0, None]
    assert out["max"].to_list() == [1.0, 8.0, 5.0, 4.0, None, None, 5.0, 8.0, None]
    assert out["mean"].to_list() == [1.0, 6.0, 5.0, 4.0, None, None, 3.0, 8.0, None]
    assert out["zero"].to_list() == [1.0, 0.0, 5.0, 4.0, 0.0, 0.0, 0.0, 8.0, 0.0]
    assert out["one"].to_list() == [1.0, 1.0, 5.0, 4.0, 1.0, 1.0, 1.0, 8.0, 1.0]
    # group 1: mean(3, 4) = 3.5 -> 3; group 2: mean(7, -4) = 1.5 -> 1
    assert out["imean"].dtype is pl.Int64
    assert out["imean"].to_list() == [7, 3, -4, 3, None, None, 1, 4, None]
    # the fill value is this library's own aggregate over the group
    g = df.group_by("k", maintain_order=True).agg(pl.col("x").mean())
    means = dict(zip(g["k"].to_list(), g["x"].to_list()))
    assert out["mean"].to_list()[1] == means[1] and out["mean"].to_list()[6] == means[2]


# ----------------------------------------------------------------------- over
def _group_ref(vals, valid, keys, op, limit):
    ev, eok = vals.copy(), valid.copy()
    for g in np.unique(keys):
        rows = np.flatnonzero(keys == g)
        v, ok = _ref(vals[rows], valid[rows], op, limit)
        ev[rows], eok[rows] = v, ok
    return ev, eok


def test_over_sorted_interleaved_and_forced_sort(gpu, plgpu_option):
    rng = np.random.default_rng(51)
    n = 2 * T + 51
    sym = np.sort(rng.integers(0, 8, n)).astype(np.int64)  # symbol 0 stands for the null key: one group
    kvalid = sym != 0
    close = rng.uniform(100, 150, n)
    cvalid = rng.random(n) >= 0.4
    exprs = [pl.col("close").forward_fill().over("symbol").alias("ff"),
             pl.col("close").backward_fill(2).over("symbol").alias("bf2"),
             pl.col("close").fill_null(strategy="forward", limit=3).over("symbol").alias("ff3")]
    want = {"ff": _group_ref(close, cvalid, sym, "forward", None), "bf2": _group_ref(close, cvalid, sym, "backward", 2),
            "ff3": _group_ref(close, cvalid, sym, "forward", 3)}

    def frame(order):
        return pl.DataFrame([pl.Series.from_numpy("symbol", sym[order], kvalid[order]),
                             pl.Series.from_numpy("close", close[order], cvalid[order])])

    def check(out, pos, what):
        for nm, (ev, eok) in want.items():
            r = out[nm]
            assert np.array_equal(r.validity_numpy()[pos], eok), (what, nm)
            assert np.array_equal(r.to_numpy()[pos][eok].view(np.uint64), ev[eok].view(np.uint64)), (what, nm)

    plgpu_option("ktime", 1)
    N.ktime_read()
    out_sorted = frame(np.arange(n)).with_columns(*exprs)
    kt = N.ktime_read()
    assert not [k for k in kt if k.startswith("srt_")], kt
    assert kt["seg_starts_kernel"][1] == 1, kt  # the three nodes share the segment cache
    assert kt["fill_apply_kernel"][1] == 3 and kt["fill_reduce_kernel"][1] == 3 and kt["fill_totals_kernel"][1] == 3, kt
    check(out_sorted, np.arange(n), "sorted")
    labels = rng.permutation(sym)  # interleaved: every group's rows keep their relative order
    pos = np.empty(n, np.int64)
    for g in np.unique(sym):
        pos[np.flatnonzero(sym == g)] = np.flatnonzero(labels == g)
    N.ktime_read()
    out_shuf = frame(np.argsort(pos)).with_columns(*exprs)
    kt = N.ktime_read()
    assert [k for k in kt if k.startswith("srt_")] and kt["invert_perm_kernel"][1] == 1, kt
    check(out_shuf, pos, "interleaved")
    plgpu_option("over_presorted", 0)
    N.ktime_read()
    out_forced = frame(np.arange(n)).with_columns(*exprs)
    assert [k for k in N.ktime_read() if k.startswith("srt_")]
    check(out_forced, np.arange(n), "forced sort")


def test_over_keys_and_composition(gpu):
    import pyarrow as pa

    rng = np.random.default_rng(52)
    n = 3000
    sym = rng.integers(0, 5, n).astype(np.int64)
    day = rng.integers(0, 3, n).astype(np.int32)
    x = rng.standard_normal(n)
    xvalid = rng.random(n) >= 0.5
    names = np.array(["aapl", "msft", "amd", "nvda", "tsm"], dtype=object)
    cat = pl.Series.from_arrow("cat", pa.array(names[sym].tolist(), pa.string()).dictionary_encode())
    df = pl.DataFrame([pl.Series.from_numpy("symbol", sym), pl.Series.from_numpy("day", day),
                       pl.Series.from_numpy("x", x, xvalid), cat])
    out = df.select(pl.col("x").forward_fill().over("cat").alias("bycat"),
                    pl.col("x").backward_fill(1).over("symbol", "day").alias("two"),
                    pl.col("x").forward_fill().diff().alias("d"),
                    (pl.col("x") / pl.col("x").forward_fill().shift(1) - 1).alias("ret"))
    ev, eok = _group_ref(x, xvalid, sym, "forward", None)
    assert np.array_equal(out["bycat"].validity_numpy(), eok)
    assert np.array_equal(out["bycat"].to_numpy()[eok].view(np.uint64), ev[eok].view(np.uint64))
    ev, eok = _group_ref(x, xvalid, sym * 3 + day, "backward", 1)
    assert np.array_equal(out["two"].validity_numpy(), eok)
    assert np.array_equal(out["two"].to_numpy()[eok].view(np.uint64), ev[eok].view(np.uint64))
    fv, fok = _ref(x, xvalid, "forward")
    dok = np.append(False, fok[1:] & fok[:-1])
    assert np.array_equal(out["d"].validity_numpy(), dok)
    assert np.array_equal(out["d"].to_numpy()[dok].view(np.uint64), (fv[1:] - fv[:-1])[dok[1:]].view(np.uint64))
    rok = np.append(False, xvalid[1:] & fok[:-1])
    assert np.array_equal(out["ret"].validity_numpy(), rok)
    with np.errstate(all="ignore"):
        er = x[1:] / fv[:-1] - 1
    assert np.array_equal(out["ret"].to_numpy()[rok].view(np.uint64), er[rok[1:]].view(np.uint64))
    with pytest.raises(pl.InvalidOperationError) as ei:
        df.group_by("symbol").agg(pl.col("x").forward_fill())
    assert "not an aggregation" in str(ei.value)


# --------------------------------------------------------------------- golden
def _golden_series(case, name="a"):
    import pyarrow as pa

    vals = case["values"]
    if case["dtype"] == "Categorical":
        return pl.Series.from_arrow(name, pa.array(vals, pa.string()).dictionary_encode())
    dt = getattr(pl, case["dtype"])
    if "chunks" in case:
        t = pa.int64() if case["dtype"] == "Int64" else pa.float64()
        batches = [pa.record_batch([pa.array(ch, t)], names=[name]) for ch in case["chunks"]]
        return pl.DataFrame.from_batches(batches)[name]
    return pl.Series(name, vals, dtype=dt)


def _golden_expr(case, name="a"):
    if case.get("method"):
        return getattr(pl.col(name), case["method"])(case["limit"])
    return pl.col(name).fill_null(strategy=case["op"], limit=case["limit"])


@pytest.mark.parametrize("case", load_golden("fill_cases.json")["cases"], ids=lambda c: c["name"])
def test_golden_cases(gpu, case):
    s = _golden_series(case)
    f = _golden_expr(case)
    cols = [s]
    if "keys" in case:
        cols.append(pl.Series("k", case["keys"], dtype=pl.Int64))
        f = f.over("k")
    out = pl.DataFrame(cols).select(f)["a"]
    if case["expected_dtype"] == "Categorical":
        assert out._cat_codes() is not None
    else:
        assert out.dtype is getattr(pl, case["expected_dtype"]), case["name"]
    assert out.to_list() == case["expected"], (case["name"], out.to_list())
    if "keys" not in case and case["dtype"] != "Categorical":
        eager = s.fill_null(strategy=case["op"], limit=case["limit"])
        assert eager.to_list() == case["expected"], (case["name"], eager.to_list())


# --------------------------------------------------------------------- plugin
def test_plugin_window_forward_fill_runs(gpu):
    from test_polars_engine import FakeNT, FakePolarsDF, PyExprIR, _table

    table, k, v, w, vvalid = _table(5000, 4)
    nt = FakeNT(table)
    scan = nt.p("DataFrameScan", ["k", "v", "w"], df=FakePolarsDF(table), projection=None, selection=None)
    fn = nt.e("Function", function_data=("fill_null_with_strategy", "forward", None), input=[nt.col("v")],
              options=None)
    win = nt.e("Window", function=fn, partition_by=[nt.col("k")], order_by=None, order_by_descending=False,
               order_by_nulls_last=False, options=type("WindowMapping", (), {"kind": "groups_to_rows"})())
    bf = nt.e("Function", function_data=("fill_null_with_strategy", "backward", 2), input=[nt.col("v")], options=None)
    nt.p("HStack", ["k", "v", "w", "fv", "bv"], input=scan, exprs=[PyExprIR(win, "fv"), PyExprIR(bf, "bv")])
    PE.execute_with_polaroid(nt, None, to_frame=lambda t: t)
    assert callable(nt.udf)
    out = nt.udf(None, None, None, False)
    assert out.column_names == ["k", "v", "w", "fv", "bv"]
    ev, eok = _group_ref(v, vvalid, k, "forward", None)
    assert out.column("fv").to_pylist() == [x if ok else None for x, ok in zip(ev.tolist(), eok.tolist())]
    ev, eok = _ref(v, vvalid, "backward", 2)
    assert out.column("bv").to_pylist() == [x if ok else None for x, ok in zip(ev.tolist(), eok.tolist())]
