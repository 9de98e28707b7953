"""GPU: ewm_mean (plgpu_ewm_mean) at the seams of its three launches, its exact
cases, the non-finite rule, min_samples, dtypes, and end to end, plain and over
groups.

Reference.  tests/ewm_ref.py restates the reference's loop
(polars-compute/src/ewm/mean.rs:52) per segment.  Validity is compared exactly
in every case.  The first non-null row of a segment, alpha = 1, all-null
segments and every non-finite row are compared without a tolerance.  Every
other value is held to the bound of DESIGN.md "Float tolerance against the
reference": with r80 the loop in numpy.longdouble, A_t the same mean of |x|
and e = max_t |v_t - r80_t| / (2^-53 A_t),

    e_gpu <= max(2 e_ref, E),   E = 4 D + 4,

e_ref the error of the loop in f64 and D the longest chain of map compositions
between an input row and an output in the kernels' schedule (`_chain`, counted
from ewm.hip).  Float32: units of 2^-24 A_t, e_ref the loop in float32, and
e_gpu <= max(e_ref, 1).  Each check prints its figures before it asserts."""

import ctypes as C

import numpy as np
import pytest

import polaroid_amd as pl
from conftest import load_golden
from ewm_ref import Yardstick, ewm_mean_ref, prepare_alpha
from polaroid_amd import _native as N
from test_ewm import check_golden, golden_runs

pytestmark = pytest.mark.gpu

T = N.CUM_TILE    # rows of one workgroup of the ewm kernels: one summary, one carry
B = N.CUM_BLOCK   # rows of one block scan of a workgroup
NS = 3 * T + 5
LENGTHS = [0, 1, 63, 64, 65, B - 1, B, B + 1, T - 1, T, T + 1, NS]
MODES = [(True, False), (True, True), (False, False), (False, True)]  # (adjust, ignore_nulls)
ALPHAS = [1.0, 0.5, 0.05, 1e-3, 1e-5]
_UINT = {4: np.uint32, 8: np.uint64}


def _chain(n):
    """D: map compositions between an input row and an output, the longest
    way.  ewm_reduce_kernel: the thread's rows, the wave's shuffle scan, the
    waves' totals, the tile's block scans.  ewm_totals_kernel: the row a tile
    left out, the thread's run of summaries, the wave scan, the waves and the
    lane before, the run again.  ewm_apply_kernel: the block scans before this
    one, the carry, the thread's rows."""
    per_thread = B // N.CUM_THREADS
    waves = N.CUM_THREADS // 64
    blocks = T // B
    tiles = (n + T - 1) // T
    run = (tiles + N.CUM_TOTALS_THREADS - 1) // N.CUM_TOTALS_THREADS
    reduce_ = per_thread + 6 + waves + blocks
    totals = 1 + run + 6 + N.CUM_TOTALS_THREADS // 64 + 1 + run
    apply_ = (blocks - 1) + 1 + per_thread
    return reduce_ + totals + apply_


def _floor(n):
    return 4 * _chain(n) + 4


def _ewm(s, alpha, adjust, ignore_nulls, min_samples=1, seg=None):
    out = N.Column()
    N.check(N.lib().plgpu_ewm_mean(C.byref(s._col), None if seg is None else C.byref(seg._col), alpha, int(adjust),
                                   int(ignore_nulls), min_samples, C.byref(out), None))
    r = pl.Series._from_native("x", out)
    return r.to_numpy(), r.validity_numpy()


def _first_rows(valid, starts):
    """The first non-null row of every segment."""
    n = len(valid)
    if n == 0:
        return np.zeros(0, np.int64)
    seg = np.zeros(n, np.int64) if starts is None else np.cumsum(np.append(True, np.asarray(starts)[1:])) - 1
    rows = np.flatnonzero(valid)
    _, first = np.unique(seg[rows], return_index=True)
    return rows[first]


def _check(got, vals, valid, alpha, adjust, ign, what, min_samples=1, starts=None):
    """Validity exactly, the exact cases bit for bit, the rest within the bound.
    Returns (e_gpu, e_ref)."""
    gv, gok = got
    f32 = vals.dtype == np.float32
    assert gv.dtype == vals.dtype and gv.shape == vals.shape, what
    kw = dict(alpha=alpha, adjust=adjust, min_samples=min_samples, ignore_nulls=ign, starts=starts)
    rv, rok = ewm_mean_ref(vals, valid, ftype=np.float32 if f32 else float, **kw)
    assert np.array_equal(gok, rok), (what, np.flatnonzero(gok != rok)[:8])
    if not rok.any():
        return 0.0, 0.0
    # non-finite rows: NaN where the reference has NaN, the same infinity where it has one
    g, r = gv[rok], rv[rok]
    assert np.array_equal(np.isnan(g), np.isnan(r)), (what, np.flatnonzero(np.isnan(g) != np.isnan(r))[:8])
    inf = np.isinf(r)
    assert np.array_equal(np.isinf(g), inf) and np.array_equal(g[inf], r[inf]), what
    # the first non-null row of every segment is its input, bit for bit
    first = _first_rows(valid, starts)
    first = first[gok[first]]
    u = _UINT[vals.dtype.itemsize]
    assert np.array_equal(gv[first].view(u), vals[first].view(u)), (what, "first rows")
    y = Yardstick(vals, valid, alpha, adjust, ign, starts, min_samples)
    assert np.array_equal(y.ok, rok)
    unit = 2.0 ** -24 if f32 else 2.0 ** -53
    e_gpu, e_ref = y.error(gv, unit), y.error(rv, unit)
    bound = max(e_ref, 1.0) if f32 else max(2 * e_ref, _floor(len(vals)))
    print(f"ewm {what}: e_gpu={e_gpu:.3g} e_ref={e_ref:.3g} bound={bound:.3g}")
    assert e_gpu <= bound, (what, e_gpu, e_ref, bound)
    return e_gpu, e_ref


def _prices(n, seed=0):
    return np.random.default_rng(seed).uniform(170.0, 330.0, n)


def _normal(n, seed=0):
    return np.random.default_rng(seed).normal(0.0, 1e4, n)


def _patterns(n, rng):
    """Null patterns: {name: validity array, None for no validity buffer}."""
    def only(rows):
        v = np.zeros(n, bool)
        v[[r for r in rows if 0 <= r < n]] = True
        return v

    first_null = np.ones(n, bool)
    first_null[:1] = False
    run = np.ones(n, bool)
    run[min(5, n):2 * T + 9] = False  # one null run from tile 0 into tile 2
    return {
        "no_validity": None,
        "all_valid": np.ones(n, bool),
        "all_null": np.zeros(n, bool),
        "only_row0": only([0]),
        "only_last": only([n - 1]),
        "first_null": first_null,
        "alternating": np.arange(n) % 2 == 0,
        "random_50": rng.random(n) >= 0.5,
        "random_99": rng.random(n) >= 0.99,
        "long_run": run,
    }


def _series(vals, valid, name="x"):
    return pl.Series.from_numpy(name, vals) if valid is None else pl.Series.from_numpy(name, vals, valid)


def _mask(valid, n):
    return np.ones(n, bool) if valid is None else valid


# ---------------------------------------------------------------------- seams
@pytest.mark.parametrize("adjust", [True, False], ids=["adjust", "noadjust"])
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_null_patterns(gpu, n, adjust):
    rng = np.random.default_rng(n)
    vals = _prices(n, seed=n)
    for name, valid in _patterns(n, rng).items():
        s = _series(vals, valid)
        for ign in (False, True):
            _check(_ewm(s, 0.05, adjust, ign), vals, _mask(valid, n), 0.05, adjust, ign, (n, name, adjust, ign))


@pytest.mark.parametrize("adjust, ign", MODES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_alphas_and_data_sets(gpu, alpha, adjust, ign):
    n = NS
    rng = np.random.default_rng(3)
    nulls30 = rng.random(n) >= 0.3
    for data, vals in (("prices", _prices(n, 1)), ("normal", _normal(n, 2))):
        for nm, valid in (("dense", None), ("nulls30", nulls30)):
            got = _ewm(_series(vals, valid), alpha, adjust, ign)
            _check(got, vals, _mask(valid, n), alpha, adjust, ign, (data, nm, alpha, adjust, ign))
            if alpha == 1.0:  # every non-null input comes back bit for bit
                ok = _mask(valid, n)
                assert np.array_equal(got[0][ok].view(np.uint64), vals[ok].view(np.uint64))


@pytest.mark.parametrize("adjust, ign", MODES)
def test_magnitude_1e300(gpu, adjust, ign):
    n = T + B + 9
    rng = np.random.default_rng(4)
    vals = rng.uniform(0.1, 1.0, n) * 1e300 * rng.choice([-1.0, 1.0], n)
    valid = rng.random(n) >= 0.2
    _check(_ewm(_series(vals, valid), 0.5, adjust, ign), vals, valid, 0.5, adjust, ign, ("1e300", adjust, ign))


def _placements(n, rng, valid):
    def at(rows):
        st = np.zeros(n, bool)
        st[[r for r in rows if 0 <= r < n]] = True
        return st

    base = np.append(True, rng.random(n - 1) < 0.01)
    # a start directly before / directly after the first non-null row of every segment of `base`
    first = _first_rows(valid, base)
    return {
        "word_seams": at([0, 63, 64, 65, 127, 128, 129, T + 63, T + 64, 2 * T + 1, n - 1]),
        "block_seams": at([0, B - 1, B, B + 1, 3 * B, 5 * B - 1, T + 2 * B, T + 7 * B - 1, 2 * T + B + 3]),
        "tile_seams": at([0, T - 1, T, T + 1, 2 * T - 1, 2 * T, 3 * T, 3 * T + 1]),
        "random_1pct": base,
        "before_first": base | at(first - 1),
        "after_first": base | at(first + 1),
    }


@pytest.mark.parametrize("adjust, ign", MODES)
@pytest.mark.parametrize("place", ["word_seams", "block_seams", "tile_seams", "random_1pct", "before_first",
                                   "after_first"])
def test_segments(gpu, place, adjust, ign):
    n = NS
    rng = np.random.default_rng(11)
    vals = _normal(n, seed=11)
    pats = _patterns(n, rng)
    for name in ("random_50", "random_99", "all_null", "long_run", "only_row0", "only_last"):
        valid = pats[name]
        starts = _placements(n, np.random.default_rng(12), valid)[place]
        seg = pl.Series.from_numpy("seg", starts)
        got = _ewm(_series(vals, valid), 0.05, adjust, ign, seg=seg)
        _check(got, vals, valid, 0.05, adjust, ign, (place, name, adjust, ign), starts=starts)


@pytest.mark.parametrize("adjust, ign", MODES)
def test_segment_identities(gpu, adjust, ign):
    n = NS
    rng = np.random.default_rng(13)
    vals = _normal(n, seed=13)
    valid = rng.random(n) >= 0.6
    s = _series(vals, valid)
    row0 = np.zeros(n, bool)
    row0[0] = True
    plain = _ewm(s, 0.05, adjust, ign)
    got = _ewm(s, 0.05, adjust, ign, seg=pl.Series.from_numpy("seg", row0))
    assert np.array_equal(got[1], plain[1])
    assert got[0].tobytes() == plain[0].tobytes()  # bit 0 only: the NULL-bitmap call, every byte
    # a start on every row: every non-null row is the first of its segment
    gv, gok = _ewm(s, 0.05, adjust, ign, seg=pl.Series.from_numpy("seg", np.ones(n, bool)))
    assert np.array_equal(gok, valid)
    assert np.array_equal(gv[valid].view(np.uint64), vals[valid].view(np.uint64))
    # an all-null segment is all null, and the segment after it starts afresh
    v2 = valid.copy()
    v2[B - 3:T + 70] = False
    st = np.zeros(n, bool)
    st[[0, B - 3, T + 70]] = True
    got = _ewm(_series(vals, v2), 0.05, adjust, ign, seg=pl.Series.from_numpy("seg", st))
    assert not got[1][B - 3:T + 70].any()
    _check(got, vals, v2, 0.05, adjust, ign, ("all-null segment", adjust, ign), starts=st)


@pytest.mark.parametrize("n", [65, B + 1, T + 1, NS])
@pytest.mark.parametrize("ms", [0, 1, 2, 3, 65, T + 1])
def test_min_samples(gpu, ms, n):
    rng = np.random.default_rng(ms + n)
    vals = _prices(n, seed=ms)
    valid = rng.random(n) >= 0.5
    starts = np.append(True, rng.random(n - 1) < 4.0 / T) if n > 1 else np.ones(n, bool)
    seg = pl.Series.from_numpy("seg", starts)
    for adjust, ign in MODES:
        s = _series(vals, valid)
        _check(_ewm(s, 0.05, adjust, ign, ms), vals, valid, 0.05, adjust, ign, ("ms", ms, n, adjust, ign), ms)
        if (adjust, ign) in ((True, False), (False, True)):
            _check(_ewm(s, 0.05, adjust, ign, ms, seg), vals, valid, 0.05, adjust, ign, ("ms seg", ms, n, adjust, ign),
                   ms, starts)
    # without a validity buffer the count is the row number within the segment
    gv, gok = _ewm(_series(vals, None), 0.5, True, False, ms)
    assert np.array_equal(gok, np.arange(n) >= max(ms, 1) - 1)


# ------------------------------------------------------------------ non-finite
@pytest.mark.parametrize("adjust, ign", MODES)
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "pinf", "ninf"])
def test_non_finite_rule(gpu, bad, adjust, ign):
    """The first non-finite value of a segment comes out as itself, every later
    non-null row of the segment as NaN; the next segment is clean.  At row 0,
    mid-tile, and just before a tile seam (the flag travels in the carry)."""
    n = 2 * T + 300
    rng = np.random.default_rng(21)
    base = _normal(n, seed=21)
    valid = rng.random(n) >= 0.3
    for at, start in ((0, 2 * T - 100), (T // 2 + 3, T + B), (T - 1, 2 * T + 5), (T - 2, T - 1)):
        vals = base.copy()
        vals[at] = bad
        ok = valid.copy()
        ok[at] = True
        if at + 7 < start:
            vals[at + 7] = -bad  # a second one in the same segment is NaN like every later row
            ok[at + 7] = True
        starts = np.zeros(n, bool)
        starts[[0, start]] = True
        gv, gok = _ewm(_series(vals, ok), 0.05, adjust, ign, seg=pl.Series.from_numpy("seg", starts))
        _check((gv, gok), vals, ok, 0.05, adjust, ign, ("non-finite", bad, at, adjust, ign), starts=starts)
        later = ok.copy()
        later[:at + 1] = False
        later[start:] = False
        assert np.array_equal(gv[at:at + 1].view(np.uint64), vals[at:at + 1].view(np.uint64))
        assert np.isnan(gv[later]).all() and (later.sum() > 50 or start - at < 100)
        assert np.isfinite(gv[start:][ok[start:]]).all()
        assert np.isfinite(gv[:at][ok[:at]]).all()
        # and in one segment only (no start bitmap), up to the column's end
        vals[start + 9] = bad
        ok[start + 9] = True
        gv, gok = _ewm(_series(vals, ok), 0.05, adjust, ign)
        assert np.isnan(gv[at + 1:][ok[at + 1:]]).all()
        _check((gv, gok), vals, ok, 0.05, adjust, ign, ("non-finite plain", bad, at, adjust, ign))


# ----------------------------------------------------------- offsets and dtypes
@pytest.mark.parametrize("off", [1, 3, 63, 65])
def test_slices(gpu, off):
    """A row offset: the validity and the start bits begin inside a word, and
    the values are not 16-byte aligned."""
    n = 2 * T + 77
    rng = np.random.default_rng(off)
    vals = _normal(n + off, seed=off)
    valid = rng.random(n + off) >= 0.4
    starts = rng.random(n + off) < 0.01
    s = pl.Series.from_numpy("x", vals, valid).slice(off, n)
    seg = pl.Series.from_numpy("seg", starts).slice(off, n)
    st = starts[off:].copy()
    st[0] = True
    v, ok = vals[off:].copy(), valid[off:].copy()
    for adjust, ign in MODES:
        _check(_ewm(s, 0.05, adjust, ign), v, ok, 0.05, adjust, ign, (off, adjust, ign))
        _check(_ewm(s, 0.05, adjust, ign, 1, seg), v, ok, 0.05, adjust, ign, (off, adjust, ign, "seg"), starts=st)


def test_bitmaps_at_odd_addresses(gpu):
    """Borrowed bitmaps that are not 8-byte aligned and not padded to a word."""
    n = T + 77
    rng = np.random.default_rng(17)
    vals = _normal(n, seed=17)
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
    for adjust, ign in MODES:
        _check(_ewm(s, 0.05, adjust, ign, 1, seg), vals, valid, 0.05, adjust, ign, ("odd", adjust, ign), starts=starts)


@pytest.mark.parametrize("adjust, ign", MODES)
def test_float32(gpu, adjust, ign):
    n = T + B + 5
    rng = np.random.default_rng(31)
    vals = _prices(n, seed=31).astype(np.float32)
    valid = rng.random(n) >= 0.3
    starts = np.append(True, rng.random(n - 1) < 0.001)
    s = pl.Series.from_numpy("x", vals, valid)
    assert s.dtype is pl.Float32
    r = s.ewm_mean(alpha=0.05, adjust=adjust, ignore_nulls=ign)
    assert r.dtype is pl.Float32 and r.name == "x"
    _check((r.to_numpy(), r.validity_numpy()), vals, valid, 0.05, adjust, ign, ("f32", adjust, ign))
    got = _ewm(s.slice(3, n - 3), 0.05, adjust, ign, 2, pl.Series.from_numpy("seg", starts).slice(3, n - 3))
    st = starts[3:].copy()
    st[0] = True
    _check(got, vals[3:].copy(), valid[3:].copy(), 0.05, adjust, ign, ("f32 seg", adjust, ign), 2, st)


_INTS = [pl.Int8, pl.Int16, pl.Int32, pl.Int64, pl.UInt8, pl.UInt16, pl.UInt32, pl.UInt64]


@pytest.mark.parametrize("dt", _INTS, ids=[str(d) for d in _INTS])
def test_every_integer_dtype_once(gpu, dt):
    """Integers are cast to Float64 (schema.rs:417 map_numeric_to_float_dtype)."""
    n = B + 1
    rng = np.random.default_rng(41)
    info = np.iinfo(dt.np_dtype)
    vals = rng.integers(max(info.min, -2**52), min(info.max, 2**52), n, dtype=dt.np_dtype, endpoint=True)
    valid = rng.random(n) >= 0.3
    s = pl.Series.from_numpy("x", vals, valid, dtype=dt)
    r = s.ewm_mean(span=20, adjust=False, min_samples=2)
    assert r.dtype is pl.Float64 and r.name == "x"
    _check((r.to_numpy(), r.validity_numpy()), vals.astype(np.float64), valid, 2.0 / 21.0, False, False, str(dt), 2)


# ----------------------------------------------------------------- many tiles
@pytest.mark.parametrize("adjust", [True, False], ids=["adjust", "noadjust"])
def test_many_tiles(gpu, adjust):
    """More tiles than the totals launch has threads: one non-null row per
    1,024 rows, a dense last tile, one segment start in the sparse part.  With
    ignore_nulls the nulls do not count, so the loop runs on the non-null rows
    alone."""
    n = 1025 * T + 3
    dense0 = 1024 * T
    vals = np.zeros(n)
    valid = np.zeros(n, bool)
    valid[np.arange(517, dense0, 1024)] = True
    valid[dense0:] = True
    rows = np.flatnonzero(valid)
    vals[rows] = _prices(len(rows), seed=5)
    start = 700 * T + 11
    starts = np.zeros(n, bool)
    starts[[0, start]] = True
    got = _ewm(_series(vals, valid), 1e-3, adjust, True, 3, pl.Series.from_numpy("seg", starts))
    cst = np.zeros(len(rows), bool)
    cst[[0, np.searchsorted(rows, start)]] = True
    rv, rok = ewm_mean_ref(vals[rows], np.ones(len(rows), bool), 1e-3, adjust, 3, True, cst)
    assert np.array_equal(got[1][rows], rok) and got[1].sum() == rok.sum()
    y = Yardstick(vals[rows], np.ones(len(rows), bool), 1e-3, adjust, True, cst, 3)
    e_gpu, e_ref = y.error(got[0][rows]), y.error(rv)
    print(f"ewm many tiles adjust={adjust}: e_gpu={e_gpu:.3g} e_ref={e_ref:.3g} floor={_floor(n)}")
    assert _chain(n) == _chain(T) + 2
    assert e_gpu <= max(2 * e_ref, _floor(n))
    first = rows[cst]
    assert np.array_equal(got[0][first[got[1][first]]].view(np.uint64), vals[first[got[1][first]]].view(np.uint64))


# ----------------------------------------------------------------- end to end
def _group_check(r, vals, valid, keys, alpha, adjust, ign, what, pos=None, ms=1):
    gv, gok = r.to_numpy(), r.validity_numpy()
    if pos is not None:
        gv, gok = gv[pos], gok[pos]
    for g in np.unique(keys):
        rows = np.flatnonzero(keys == g)
        _check((gv[rows], gok[rows]), vals[rows], valid[rows], alpha, adjust, ign, (what, int(g)), ms)


def test_over_sorted_interleaved_and_forced_sort(gpu, plgpu_option):
    rng = np.random.default_rng(51)
    n = 2 * T + 51
    sym = np.sort(rng.integers(0, 8, n)).astype(np.int64)  # symbol 0 stands for the null key: one group
    kvalid = sym != 0
    close = _prices(n, seed=51)
    cvalid = rng.random(n) >= 0.3
    a20 = prepare_alpha(span=20)
    ahl = prepare_alpha(half_life=5.0)
    exprs = [pl.col("close").ewm_mean(span=20).over("symbol").alias("e20"),
             pl.col("close").ewm_mean(half_life=5.0, adjust=False, ignore_nulls=True, min_samples=3)
             .over("symbol").alias("hl")]
    want = {"e20": (a20, True, False, 1), "hl": (ahl, False, True, 3)}

    def frame(order):
        return pl.DataFrame([pl.Series.from_numpy("symbol", sym[order], kvalid[order]),
                             pl.Series.from_numpy("close", close[order], cvalid[order])])

    def check(out, pos, what):
        for nm, (alpha, adjust, ign, ms) in want.items():
            assert out[nm].dtype is pl.Float64
            _group_check(out[nm], close, cvalid, sym, alpha, adjust, ign, (what, nm), pos, ms)

    plgpu_option("ktime", 1)
    N.ktime_read()
    out_sorted = frame(np.arange(n)).with_columns(*exprs)
    kt = N.ktime_read()
    assert not [k for k in kt if k.startswith("srt_")], kt
    assert kt["seg_starts_kernel"][1] == 1, kt  # the two nodes share the segment cache
    assert kt["ewm_apply_kernel"][1] == 2 and kt["ewm_reduce_kernel"][1] == 2 and kt["ewm_totals_kernel"][1] == 2, kt
    check(out_sorted, np.arange(n), "sorted")
    lazy = frame(np.arange(n)).lazy().select(exprs[0]).collect()
    assert lazy["e20"].to_numpy().tobytes() == out_sorted["e20"].to_numpy().tobytes()
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
    x = _normal(n, seed=52)
    xvalid = rng.random(n) >= 0.5
    names = np.array(["aapl", "msft", "amd", "nvda", "tsm"], dtype=object)
    cat = pl.Series.from_arrow("cat", pa.array(names[sym].tolist(), pa.string()).dictionary_encode())
    df = pl.DataFrame([pl.Series.from_numpy("symbol", sym), pl.Series.from_numpy("day", day),
                       pl.Series.from_numpy("x", x, xvalid), cat])
    out = df.select(pl.col("x").ewm_mean(alpha=0.1).over("cat").alias("bycat"),
                    pl.col("x").ewm_mean(com=3, adjust=False).over("symbol", "day").alias("two"),
                    (pl.col("x") - pl.col("x").ewm_mean(span=12)).alias("dev"),
                    pl.col("x").forward_fill().ewm_mean(alpha=0.1).alias("ffe"),
                    pl.col("x").ewm_mean(alpha=0.1).alias("plain"))
    _group_check(out["bycat"], x, xvalid, sym, 0.1, True, False, "bycat")
    _group_check(out["two"], x, xvalid, sym * 3 + day, 0.25, False, False, "two")
    a12 = prepare_alpha(span=12)
    e12 = pl.Series.from_numpy("x", x, xvalid).ewm_mean(span=12)
    _check((e12.to_numpy(), e12.validity_numpy()), x, xvalid, a12, True, False, "span12")
    assert np.array_equal(out["dev"].validity_numpy(), xvalid)
    assert np.array_equal(out["dev"].to_numpy()[xvalid].view(np.uint64),
                          (x - e12.to_numpy())[xvalid].view(np.uint64))
    ff = pl.Series.from_numpy("x", x, xvalid).forward_fill()
    _check((out["ffe"].to_numpy(), out["ffe"].validity_numpy()), ff.to_numpy(), ff.validity_numpy(), 0.1, True, False,
           "forward_fill().ewm_mean")
    _check((out["plain"].to_numpy(), out["plain"].validity_numpy()), x, xvalid, 0.1, True, False, "plain")
    with pytest.raises(pl.InvalidOperationError) as ei:
        df.group_by("symbol").agg(pl.col("x").ewm_mean(alpha=0.5))
    assert "not an aggregation" in str(ei.value)
    for bad in (pl.Series("b", [True, None, False]), pl.Series("s", ["a", None, "b"]), cat):
        with pytest.raises(pl.InvalidOperationError) as ei:
            bad.ewm_mean(alpha=0.5)
        assert "must be numeric" in str(ei.value)


# --------------------------------------------------------------------- golden
@pytest.mark.parametrize("case", load_golden("ewm_cases.json")["cases"], ids=lambda c: c["name"])
def test_golden_cases(gpu, case):
    s = pl.Series("a", case["values"], dtype=getattr(pl, case["dtype"]))
    for run in golden_runs(case):
        r = s.ewm_mean(**run)
        assert r.dtype is pl.Float64, case["name"]
        check_golden(case, r.to_list(), (case["name"], run, "series"))
        e = pl.DataFrame([s]).select(pl.col("a").ewm_mean(**run))["a"]
        check_golden(case, e.to_list(), (case["name"], run, "expr"))
