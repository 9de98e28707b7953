"""One oracle-exact case per kernel variant that a library option selects,
each proving that its variant ran.

The options below pick another kernel, template instantiation or launch
shape (plgpu_internal.hpp "(A/B)"); the rest of the suite runs their default
side only.  Every case here compares bit for bit with the oracle, exactly as
the default-path tests of the same operator do (their helpers are reused),
and then asserts the report that tells its variant from the default: the
kernel timer's name of the option-selected launch (option ktime,
_native.ktime_read), info["fused_variant"], info["part_layout"] or the
launched grid.

  sort      srt_w4, srt_up_tiles
  rolling   rl_stream, rl_grid, rl_div (crossed with rl_mean_hot / rl_var_hot)
  filter    filt_pipe (crossed with filt_fused)
  group-by  part_threads, part_rows4, part_direct, part_lds_kb (partitioned);
            gb_pair, grid_rounds, wave_report (fused)
  join      join_radix_load

tests/test_option_coverage.py keeps the list complete.
"""

import functools

import numpy as np
import pytest

import polaroid_amd as pl
from oracle import oracle as O
from polaroid_amd import _native as N
from polaroid_amd._native import fused_variant
from polaroid_amd.expr import col
from test_gpu_groupby_sweep import _compare as _gb_compare
from test_gpu_groupby_sweep import _data as _gb_data
from test_gpu_groupby_sweep import _gpu as _gb_gpu
from test_gpu_groupby_sweep import _oracle as _gb_oracle
from test_gpu_join_radix import _check as _rj_check
from test_gpu_join_radix import _join as _rj_join
from test_gpu_join_radix import FORCED_CASES, _forced_case
from test_gpu_reduce import _compare as _red_compare
from test_gpu_reduce import _oracle as _red_oracle
from test_gpu_sort_multi import _cols as _multi_cols
from test_gpu_sort_rolling import _rand_col, _rolling_check, _span_data, _var_check

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def _timed(fn):
    """fn()'s result and the kernel timer's names of its launches (option
    ktime is on)."""
    N.ktime_read()
    out = fn()
    return out, N.ktime_read()


# ------------------------------------------------------------------- sort
SORT_NS = [nt * 4096 - 5 for nt in (1, 7, 9, 17, 25)] + [4097, 100_003]


def _sort_names(w4, tiles):
    up = "srt_upsweep_kernel" if tiles == 1 else f"srt_upsweep_t{tiles}_kernel"
    return up, "srt_downsweep_w4_kernel"


def _assert_sort_variant(kt, w4, tiles, packed, tag):
    up, down4 = _sort_names(w4, tiles)
    assert up in kt, (tag, sorted(kt))
    others = [k for k in kt if k.startswith("srt_upsweep") and k != up]
    assert not others, (tag, others)
    if packed:
        # the separate passes and the pack transition keep the plain name
        assert "srt_downsweep_kernel" in kt, (tag, sorted(kt))
        assert (down4 in kt) == bool(w4), (tag, sorted(kt))


@pytest.mark.parametrize("tiles", [1, 2, 3, 8])
@pytest.mark.parametrize("w4", [0, 1])
def test_sort_packed_passes_and_upsweep_tiles(gpu, plgpu_option, w4, tiles):
    """srt_w4: the packed downsweeps compiled for 4 waves per SIMD;
    srt_up_tiles: 1, 2, 3 or 8 tiles per upsweep workgroup.  Keys that reach
    the packed passes: full-range Int64 (3 separate passes, the pack
    transition, 3 packed passes, the ids pass) and 40-bit values (packed from
    the first pass).  Rows: ntiles * 4096 - 5 for 1, 7, 9, 17 and 25 tiles,
    4097 and 100,003 (fewer tiles than a workgroup takes, a last workgroup
    with fewer, workgroup counts below 8 and no multiple of 8); with and
    without nulls, descending and nulls_last both ways.  Bit-exact
    permutation against the oracle; every sort's timer names show the two
    variants."""
    plgpu_option("srt_w4", w4)
    plgpu_option("srt_up_tiles", tiles)
    plgpu_option("ktime", 1)
    for n in SORT_NS:
        for keys in ("full", "bits40"):
            for nulls in (False, True):
                rng = np.random.default_rng(n + 3 * nulls + len(keys))
                if keys == "full":
                    v, valid = _rand_col(rng, n, "i64", nulls, True)
                else:
                    v = rng.integers(0, 1 << 40, n).astype(np.int64)
                    valid = (rng.random(n) > 0.1) if nulls else None
                s = pl.Series.from_numpy("x", v, valid)
                for descending, nulls_last in ((False, False), (True, True)) + (((False, True), (True, False)) if nulls else ()):
                    got, kt = _timed(lambda: s.arg_sort(descending=descending, nulls_last=nulls_last).to_numpy())
                    exp = O.arg_sort(O.HostCol(v, valid), descending, nulls_last)
                    tag = (n, keys, nulls, descending, nulls_last)
                    assert np.array_equal(got.astype(np.int64), exp), tag
                    _assert_sort_variant(kt, w4, tiles, True, tag)


@pytest.mark.parametrize("tiles", [1, 2, 3, 8])
@pytest.mark.parametrize("w4", [0, 1])
def test_sort_float_and_multi_column_variants(gpu, plgpu_option, w4, tiles):
    """The same two options under a Float64 key with NaN, +-0 and +-inf (all
    eight code bytes vary: packed passes) and under the five-column sort
    (u, j, i, f, b), whose passes run over each column's codes in turn."""
    plgpu_option("srt_w4", w4)
    plgpu_option("srt_up_tiles", tiles)
    plgpu_option("ktime", 1)
    for n in (9 * 4096 - 5, 100_003):
        for nulls in (False, True):
            rng = np.random.default_rng(n + nulls)
            v, valid = _rand_col(rng, n, "f64", nulls, True)
            s = pl.Series.from_numpy("x", v, valid)
            for descending, nulls_last in ((False, False), (True, True)):
                got, kt = _timed(lambda: s.arg_sort(descending=descending, nulls_last=nulls_last).to_numpy())
                exp = O.arg_sort(O.HostCol(v, valid), descending, nulls_last)
                assert np.array_equal(got.astype(np.int64), exp), (n, nulls, descending, nulls_last)
                _assert_sort_variant(kt, w4, tiles, True, (n, nulls, descending))
    n, by = 100_003, ("u", "j", "i", "f", "b")
    rng = np.random.default_rng(n + w4 + tiles)
    cols = _multi_cols(rng, n)
    desc = [bool(k & 1) for k in range(len(by))]
    nl = [bool((k >> 1) & 1) for k in range(len(by))]
    df = pl.DataFrame([pl.Series.from_numpy(k, v, m) for k, (v, m) in cols.items()] +
                      [pl.Series.from_numpy("row", np.arange(n, dtype=np.int64))])
    out, kt = _timed(lambda: df.sort(list(by), descending=desc, nulls_last=nl))
    assert np.array_equal(out["row"].to_numpy(), O.arg_sort_multi([cols[k] for k in by], desc, nl))
    # (few-valued columns: one or two code bytes vary, no packed pass to tell)
    _assert_sort_variant(kt, w4, tiles, False, "multi")
    # two wide keys (the Int64 column's ties leave rows to the Float64 one):
    # each column's passes reach the packed downsweeps
    a, _ = _rand_col(rng, n, "i64", False, True)
    x, xv = _rand_col(rng, n, "f64", True, True)
    df = pl.DataFrame([pl.Series.from_numpy("a", a), pl.Series.from_numpy("x", x, xv),
                       pl.Series.from_numpy("row", np.arange(n, dtype=np.int64))])
    out, kt = _timed(lambda: df.sort(["a", "x"], descending=[True, False], nulls_last=[False, True]))
    assert np.array_equal(out["row"].to_numpy(), O.arg_sort_multi([(a, None), (x, xv)], [True, False], [False, True]))
    _assert_sort_variant(kt, w4, tiles, True, "multi wide")


# ---------------------------------------------------------------- rolling
RL_BLOCK = 512   # outputs per block (rolling.hip kRwOut)
RL_WAVES = 4     # waves per workgroup (kRwWaves)


def _stream_waves(grid):
    """Waves of the stream grid when the column has at least that many
    blocks: CUs x workgroups per CU (option rl_grid; 0: 4) x 4."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * (grid if grid > 0 else 4) * RL_WAVES


# the forms of the blocks one wave visits in turn, by wave index mod 4:
# p narrow prices (the int64 form: the full-window scans and the hot kernels),
# m a 40-binade block (128-bit words), n prices with one NaN (the counted
# scans), h `huge` (per-output exact).  A prices block follows each of the
# other forms on some wave within three rounds.
STREAM_FORMS = ("pmpn", "nphp", "hpmp", "mnph")


def _stream_column(n, waves, rng, dtype=np.float64):
    """Block b is visited by wave b mod `waves` in round b // waves; its form
    is STREAM_FORMS[wave mod 4][round mod 4], so the blocks one wave scans
    over the same LDS rings differ, and narrow blocks come after mixed, NaN
    and huge ones."""
    if dtype != np.float64:
        info = np.iinfo(dtype)
        return rng.integers(info.min // 2, info.max // 2, n).astype(dtype)
    v = rng.uniform(100, 150, n)
    nblocks = (n + RL_BLOCK - 1) // RL_BLOCK
    for b in range(nblocks):
        form = STREAM_FORMS[(b % waves) % 4][(b // waves) % 4] if waves else "p"
        lo, hi = b * RL_BLOCK, min(n, (b + 1) * RL_BLOCK)
        if form == "m":
            v[lo:hi] = _span_data("mixed", hi - lo, rng)
        elif form == "n":
            v[lo + (b * 37) % (hi - lo)] = np.nan
        elif form == "h":
            v[lo:hi] = _span_data("huge", hi - lo, rng)
    return v


def _stream_name(kind, grid, mean_hot, var_hot, dtype=np.float64):
    """The timer's name of the launch under rl_stream 1."""
    g = "_grid" if grid > 0 else ""
    if kind in ("var", "std"):
        return f"rl_var_hot_stream{g}_kernel" if var_hot else f"rl_stream_var{g}_kernel"
    if mean_hot and (kind == "mean" or dtype == np.float64):
        return "rl_wave_kernel"  # rl_mean_hot_kernel has no streamed form: the option is not honoured
    return f"rl_stream{g}_kernel"


RL_WINDOWS = [(w, ms, center) for w in (1, 2, 20, 64) for ms in sorted({w, 1}) for center in (False, True)]


@pytest.mark.parametrize("var_hot", [1, 0])
@pytest.mark.parametrize("mean_hot", [1, 0])
@pytest.mark.parametrize("grid", [1, 0])
@pytest.mark.parametrize("n", [512 * 3 + 9, 1])
def test_rolling_stream_small(gpu, plgpu_option, n, grid, mean_hot, var_hot):
    """rl_stream 1 where most waves exit at once (3 blocks and a ragged one)
    and on one row, at both grids, crossed with rl_mean_hot and rl_var_hot:
    sum / mean on Float64, sum on Int64 / Int32, var / std with ddof 0 / 1;
    w 1, 2, 20, 64, min_samples w and 1, centred and not."""
    plgpu_option("rl_stream", 1)
    plgpu_option("rl_grid", grid)
    plgpu_option("rl_mean_hot", mean_hot)
    plgpu_option("rl_var_hot", var_hot)
    plgpu_option("ktime", 1)
    rng = np.random.default_rng(n + grid)
    # (fewer blocks than waves: each block is its wave's first, so blocks 0..3
    # take STREAM_FORMS' first forms: prices, one NaN, huge, mixed)
    data = {"forms": _stream_column(n, _stream_waves(grid), rng)}
    ints = {dt: _stream_column(n, 0, rng, dt) for dt in (np.int64, np.int32)}
    for w, ms, center in RL_WINDOWS:
        for v in data.values():
            for kind in ("sum", "mean"):
                _, kt = _timed(lambda: _rolling_check(v, None, kind, w, ms, center, ref_bound=False))
                assert _stream_name(kind, grid, mean_hot, var_hot) in kt, (kind, w, ms, center, sorted(kt))
            for ddof in (0, 1):
                for std in (False, True):
                    _, kt = _timed(lambda: _var_check(v, None, w, ms, center, ddof, std))
                    assert _stream_name("var", grid, mean_hot, var_hot) in kt, (w, ms, center, ddof, std, sorted(kt))
        for dt, iv in ints.items():
            _, kt = _timed(lambda: _rolling_check(iv, None, "sum", w, ms, center, ref_bound=False))
            assert _stream_name("sum", grid, mean_hot, var_hot, dt) in kt, (dt, w, ms, center, sorted(kt))


@functools.lru_cache(maxsize=None)
def _large_stream_data():
    waves = _stream_waves(1)
    # 3 W 512 + 5 512 + 77: every wave streams at least 3 blocks, five
    # stream 4 and one a ragged fifth (1,575,501 rows on 256 CUs)
    n = 3 * waves * RL_BLOCK + 5 * RL_BLOCK + 77
    rng = np.random.default_rng(n)
    return {"forms": _stream_column(n, waves, rng), "narrow": _span_data("narrow", n, rng),
            np.int64: _stream_column(n, waves, rng, np.int64), np.int32: _stream_column(n, waves, rng, np.int32)}


def _same_f64(gv, gok, ev, eok, tag):
    assert np.array_equal(gok, eok), tag
    g, e = gv[gok], ev[eok]
    assert np.array_equal(np.isnan(g), np.isnan(e)), tag
    m = ~np.isnan(e)
    assert np.array_equal(g[m].view(np.int64), e[m].view(np.int64)), tag


def _large_cases():
    """kind x w x min_samples (w, 1) x centre x ddof (var / std: 0, 1): one
    case each, since the oracle's exact mode takes up to 2 s per call at this
    size (its cost grows with w)."""
    out = []
    for kind in ("sum", "mean", "sum_i64", "sum_i32", "var", "std"):
        for w in (1, 2, 20, 64):
            for ms in sorted({w, 1}):
                for center in (False, True):
                    for ddof in ((0, 1) if kind in ("var", "std") else (0,)):
                        out.append((kind, w, ms, center, ddof))
    return out


@pytest.mark.parametrize("kind,w,ms,center,ddof", _large_cases(),
                         ids=["-".join(map(str, c)) for c in _large_cases()])
def test_rolling_stream_large(gpu, plgpu_option, kind, w, ms, center, ddof):
    """rl_stream 1 at rl_grid 1 on a column three and a bit times the stream
    grid's blocks: every wave scans blocks of different forms one after
    another over the same LDS rings (STREAM_FORMS: a full-window scan after a
    128-bit, a counted and an exact block; stale ring slots, the zeroed
    prefix -1 slots and the per-block number form are what a
    one-block-per-wave case cannot show).  With rl_mean_hot / rl_var_hot on
    and off (one reference for both); a uniform narrow column (full after
    full) under full uncentred windows of 2, 20 and 64."""
    plgpu_option("rl_stream", 1)
    plgpu_option("rl_grid", 1)
    plgpu_option("ktime", 1)
    data = _large_stream_data()
    base = {"sum_i64": "sum", "sum_i32": "sum"}.get(kind, kind)
    var = base in ("var", "std")
    cols = [data[np.int64]] if kind == "sum_i64" else [data[np.int32]] if kind == "sum_i32" else \
        [data["forms"]] + ([data["narrow"]] if w > 1 and ms == w and not center else [])
    for v in cols:
        s = pl.Series.from_numpy("x", v, None)
        hc = O.HostCol(v, None)
        if var:
            ev, eok = O.rolling_var(hc, w, ms, center, ddof, base == "std", O.ROLLING_EXACT)
            _, rok = O.rolling_var(hc, w, ms, center, ddof, base == "std", O.ROLLING_REFERENCE)
            assert np.array_equal(eok, rok)
        else:
            ev, eok = O.rolling(hc, base, w, ms, center, O.ROLLING_EXACT)
        for hot in (1, 0):
            plgpu_option("rl_mean_hot", hot)
            plgpu_option("rl_var_hot", hot)
            if var:
                fn = (s.rolling_std if base == "std" else s.rolling_var)
                out, kt = _timed(lambda: fn(w, min_samples=ms, center=center, ddof=ddof))
            else:
                fn = s.rolling_mean if base == "mean" else s.rolling_sum
                out, kt = _timed(lambda: fn(w, min_samples=ms, center=center))
            tag = (kind, w, ms, center, ddof, hot)
            assert _stream_name(base, 1, hot, hot, v.dtype) in kt, (tag, sorted(kt))
            gv, gok = out.to_numpy(), out.validity_numpy()
            if gv.dtype.kind in "iu":
                assert np.array_equal(gok, eok), tag
                assert np.array_equal(gv[gok].astype(np.int64), ev[eok].astype(np.int64)), tag
            else:
                _same_f64(gv, gok, ev, eok, tag)


@pytest.mark.parametrize("data", ["low", "high", "overflow", "narrow"])
def test_rolling_mean_without_one_correction_quotient(gpu, plgpu_option, data):
    """rl_div 0: full windows' means by a division instead of rw_div, on the
    data of test_rolling_full_waves_specialised_scan (exponents just outside
    rw_div's range, sums that round to inf, prices).  Equal to the oracle,
    hence to the rl_div 1 results."""
    plgpu_option("rl_div", 0)
    plgpu_option("ktime", 1)
    rng = np.random.default_rng(len(data) * 5)
    n = 4096 * 2 + 777
    v = {"narrow": lambda: rng.uniform(100, 150, n),
         "low": lambda: rng.uniform(1, 2, n) * 2.0 ** -851,
         "high": lambda: rng.uniform(1, 2, n) * 2.0 ** 990,
         "overflow": lambda: rng.uniform(0.5, 1, n) * 1.7e308}[data]()
    for w in (1, 2, 20, 64):
        for center in (False, True):
            for kind in ("sum", "mean"):
                _, kt = _timed(lambda: _rolling_check(v, None, kind, w, w, center, ref_bound=False))
                assert "rl_wave_nodiv_kernel" in kt and "rl_wave_kernel" not in kt, (kind, w, center, sorted(kt))


@pytest.mark.parametrize("data", ["low", "high"])
def test_rolling_var_without_one_correction_quotients(gpu, plgpu_option, data):
    """rl_div 0 under var / std, on the data of
    test_rolling_var_full_waves_specialised_scan: rw_var_scan_full divides
    (and rl_var_hot_kernel, which has the one-correction form only, is off)."""
    plgpu_option("rl_div", 0)
    plgpu_option("ktime", 1)
    rng = np.random.default_rng(len(data) * 7)
    n = 4096 * 2 + 777
    v = {"low": lambda: rng.uniform(1, 2, n) * 2.0 ** -420,
         "high": lambda: rng.uniform(1, 2, n) * 2.0 ** 494}[data]()
    for w in (2, 20, 64):
        for center in (False, True):
            for ddof in (0, 1, w):
                _, kt = _timed(lambda: _var_check(v, None, w, w, center, ddof, std=(ddof == 1)))
                assert "rl_wave_var_nodiv_kernel" in kt and "rl_wave_var_kernel" not in kt, (w, center, ddof, sorted(kt))


# ----------------------------------------------------------------- filter
def _filter_columns(rng, ncols, n):
    """Null-free 8-byte columns, Float64 (even index) and Int64 (odd)."""
    return [rng.uniform(0, 500, n) if j % 2 == 0 else rng.integers(-1000, 1000, n).astype(np.int64)
            for j in range(ncols)]


def _filter_predicates(name, v):
    """(expression, numpy mask) selecting about half, all and none."""
    if v.dtype == np.float64:
        return [(pl.col(name) > 250.0, v > 250.0), (pl.col(name) > -1.0, np.ones(v.shape[0], bool)),
                (pl.col(name) < -1.0, np.zeros(v.shape[0], bool))]
    return [(pl.col(name) >= 0, v >= 0), (pl.col(name) >= -5000, np.ones(v.shape[0], bool)),
            (pl.col(name) < -5000, np.zeros(v.shape[0], bool))]


@pytest.mark.parametrize("ncols", [1, 2, 3, 8])
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("pipe", [1, 0])
def test_filter_scatter_column_order_and_prefetch(gpu, plgpu_option, pipe, fused, ncols):
    """filt_pipe (the next column's loads before this column's stores) on and
    off, under the three-pass scatter (filter_scatter8_kernel) and the
    one-pass kernel (filter_fused8_kernel, which scatters the predicate's
    column first, then the others): 1, 2, 3 and 8 null-free 8-byte columns
    with the predicate on the first, a middle and the last; 1, 4095, 4097 and
    64 * 4096 + 5 rows; half, all and none selected; whole and sliced
    (offset 3) inputs.  Every output column against numpy masking."""
    plgpu_option("filt_pipe", pipe)
    plgpu_option("filt_fused", fused)
    plgpu_option("ktime", 1)
    suffix = "" if pipe else "_nopipe"
    for n in (1, 4095, 4097, 64 * 4096 + 5):
        rng = np.random.default_rng(n + ncols)
        host = _filter_columns(rng, ncols, n + 3)
        names = [f"c{j}" for j in range(ncols)]
        for off in (0, 3):
            df = pl.DataFrame([pl.Series.from_numpy(nm, v).slice(off, n) for nm, v in zip(names, host)])
            view = [v[off:off + n] for v in host]
            for pj in sorted({0, ncols // 2, ncols - 1}):
                for e, m in _filter_predicates(names[pj], view[pj]):
                    out, kt = _timed(lambda: df.filter(e))
                    tag = (n, off, pj, int(m.sum()))
                    assert out.height == int(m.sum()), tag
                    for nm, v in zip(names, view):
                        assert np.array_equal(out[nm].to_numpy().view(np.uint64), v[m].view(np.uint64)), (tag, nm)
                        assert out[nm].validity_numpy().all(), (tag, nm)
                    if fused:
                        assert f"filter_fused8{suffix}_kernel" in kt, (tag, sorted(kt))
                        assert "filter_mask_kernel" not in kt, (tag, sorted(kt))
                    else:
                        assert "filter_mask_kernel" in kt, (tag, sorted(kt))
                        scat = [k for k in kt if k.startswith("filter_scatter8")]
                        # (nothing selected: no scatter launch)
                        assert scat == ([f"filter_scatter8{suffix}_kernel"] if m.any() else []), (tag, sorted(kt))


def test_filter_mixed_frame_without_prefetch(gpu, plgpu_option):
    """filt_pipe 0 on a frame mixing a nullable column and an Int32 column
    with null-free 8-byte ones: filter_scatter8_kernel<false> for those next
    to filter_scatter_kernel for the others."""
    plgpu_option("filt_pipe", 0)
    plgpu_option("ktime", 1)
    for n in (4097, 64 * 4096 + 5):
        rng = np.random.default_rng(n)
        x = rng.uniform(0, 500, n)
        y, yv = rng.standard_normal(n), rng.random(n) > 0.2
        i = rng.integers(-50, 50, n).astype(np.int32)
        q = rng.integers(-10**12, 10**12, n).astype(np.int64)
        z = rng.standard_normal(n)
        df = pl.DataFrame([pl.Series.from_numpy("x", x), pl.Series.from_numpy("y", y, yv),
                           pl.Series.from_numpy("i", i), pl.Series.from_numpy("q", q), pl.Series.from_numpy("z", z)])
        for e, m in ((pl.col("x") > 250.0, x > 250.0), (pl.col("i") >= 0, i >= 0), (pl.col("y") > 0.0, yv & (y > 0.0))):
            out, kt = _timed(lambda: df.filter(e))
            assert out.height == int(m.sum())
            assert "filter_scatter8_nopipe_kernel" in kt and "filter_scatter8_kernel" not in kt, sorted(kt)
            for nm, v in (("x", x), ("q", q), ("z", z), ("i", i)):
                assert np.array_equal(out[nm].to_numpy(), v[m]), nm
                assert out[nm].validity_numpy().all(), nm
            assert np.array_equal(out["y"].validity_numpy(), yv[m])
            assert np.array_equal(_bits(out["y"].to_numpy()[yv[m]]), _bits(y[m][yv[m]]))


# ------------------------------------------------- partitioned group-by
PART_N = 300_001


@functools.lru_cache(maxsize=None)
def _part_frame(card, sorted_keys):
    """The sweep's frame at PART_N rows over `card` keys, plus g, h (one
    binade each: 2-limb sums) and w (40 binades: 3-limb sums, the recipe of
    tests/test_gpu_fused_variants.py)."""
    _, cols = _gb_data(900 + card % 97 + sorted_keys, n=PART_N, card=card, sorted_keys=sorted_keys)
    rng = np.random.default_rng(card + sorted_keys)
    cols["g"] = (rng.uniform(1, 2, PART_N), None)
    cols["h"] = (rng.uniform(128, 256, PART_N), None)
    cols["w"] = (rng.uniform(1, 2, PART_N) * 2.0 ** rng.integers(-20, 20, PART_N) * rng.choice([-1.0, 1.0], PART_N),
                 None)
    return pl.DataFrame([pl.Series.from_numpy(nm, v, m) for nm, (v, m) in cols.items()]), cols


def _S(*names):
    return [("sum", col(nm)) for nm in names]


# id, key, aggregations, sorted keys; then what the partition launcher does
# with it: fast (gb_fast_kernel over the partitions: sum-only accs), limbs,
# racc (register accumulators: the thread-count options do not apply)
PART_CASES = [
    ("sum1", "k", lambda: _S("c"), False, dict(fast=True, limbs=2, racc=False)),
    ("sum4", "k", lambda: _S("c", "b", "e", "f"), False, dict(fast=True, limbs=2, racc=False)),
    ("sum6", "k", lambda: _S("c", "b", "e", "f", "g", "h"), False, dict(fast=True, limbs=2, racc=False)),
    ("sum_3limb", "k", lambda: _S("w", "c"), False, dict(fast=True, limbs=3, racc=False)),
    ("mixed", "k", lambda: _S("c") + [("min", col("q")), ("max", col("b")), ("count", col("f"))], False,
     dict(fast=False, limbs=3, racc=False)),
    ("null_value", "k", lambda: _S("cn", "b"), False, dict(fast=True, limbs=2, racc=False)),
    ("null_key", "kn", lambda: _S("c", "b"), False, dict(fast=True, limbs=2, racc=False)),
    # (register accumulators where keys repeat in runs: 60 rows per key at
    # 5,000 keys; at 300,000 keys a key has one row or two and no run forms)
    ("sorted_keys", "k", lambda: _S("c", "b"), True, dict(fast=True, limbs=2, racc=None)),
]

T512, T1024, ROWS4 = "gb_part_agg_t512_kernel", "gb_part_agg_t1024_kernel", "gb_part_agg_rows4_kernel"


@pytest.mark.parametrize("case", PART_CASES, ids=[c[0] for c in PART_CASES])
@pytest.mark.parametrize("card", [5_000, 300_000])
def test_partitioned_launch_variants(gpu, plgpu_option, card, case):
    """The partitioned path (gb_path 3) at 300,001 rows over 5,000 and
    300,000 keys, each case under: 512 and 1024 threads per workgroup
    (part_threads; unforced, 1024 needs 65,536 rows per workgroup), 4 rows
    per thread (part_rows4 with 512 threads: 2-limb sum-only plans without
    register accumulators), partitions kept off their table regions
    (part_direct 0, with 2^10 partitions so that each has one workgroup), and
    LDS table budgets of 80 and 40 KiB (part_lds_kb: smaller tables, more
    partition bits).  Bit-exact against the oracle every time."""
    cid, key, build, sorted_keys, what = case
    df, cols = _part_frame(card, sorted_keys)
    specs = build()
    exp = _gb_oracle(cols, key, specs, None, PART_N, names_extra=("w",))
    plgpu_option("gb_path", 3)
    plgpu_option("plan_cache", 0)  # every run plans for its own options
    plgpu_option("ktime", 1)

    def run(tag):
        (out, info), kt = _timed(lambda: _gb_gpu(df, key, specs, None, False))
        assert info["path"] == 3, (cid, tag, info)
        assert info["sum_limbs"] == what["limbs"], (cid, tag, info)
        _gb_compare(out, key, exp, len(specs), False, (cid, tag, info))
        return info, kt

    racc = card == 5_000 if what["racc"] is None else what["racc"]
    shaped = what["fast"] and not racc  # part_threads / part_rows4 apply
    info0, kt = run("default")
    assert "gb_part_agg_kernel" in kt and not {T512, T1024, ROWS4} & set(kt), (cid, sorted(kt))
    for threads, name in ((512, T512), (1024, T1024)):
        plgpu_option("part_threads", threads)
        _, kt = run(("part_threads", threads))
        assert {T512, T1024, ROWS4} & set(kt) == ({name} if shaped else set()), (cid, threads, sorted(kt))
    plgpu_option("part_threads", 512)
    plgpu_option("part_rows4", 1)
    _, kt = run("part_rows4")
    want = set() if not shaped else {ROWS4} if what["limbs"] == 2 else {T512}
    assert {T512, T1024, ROWS4} & set(kt) == want, (cid, "part_rows4", sorted(kt))
    plgpu_option("part_rows4", 0)
    plgpu_option("part_threads", 0)

    plgpu_option("part_bits", 10)
    info, kt = run("part_bits 10")
    assert info["part_layout"] & 0xFF >= 10 and "gb_part_agg_kernel" in kt, (cid, info, sorted(kt))
    plgpu_option("part_direct", 0)
    _, kt = run("part_direct 0")
    assert "gb_part_agg_nodirect_kernel" in kt and "gb_part_agg_kernel" not in kt, (cid, sorted(kt))
    plgpu_option("part_direct", 1)
    plgpu_option("part_bits", -1)

    bits = [info0["part_layout"] & 0xFF]
    for kb in (80, 40):
        plgpu_option("part_lds_kb", kb)
        info, _ = run(("part_lds_kb", kb))
        bits.append(info["part_layout"] & 0xFF)
    # half the table budget: half the slots per partition, one more partition
    # bit.  (80 KiB changes nothing where the plan's other bound, the full
    # record layout within 160 KiB for a rerun through the generic kernel,
    # already halves the slim table: two sums hold 8 words per slot slim and
    # 10 full, so 2^11 slots fit 160 KiB slim but not full.)
    assert bits[0] <= bits[1] < bits[2], (cid, bits)
    if len(specs) != 2 or not what["fast"]:
        assert bits[0] < bits[1], (cid, bits)


# ------------------------------------------------------- fused group-by
@pytest.mark.parametrize("form", ["vwap", "vwap_rev", "vwap_swap"])
@pytest.mark.parametrize("pred", ["none", "on_a"])
def test_product_pair_variant_off(gpu, plgpu_option, form, pred):
    """gb_pair 0: (a * b).sum() next to b.sum() -- the vwap forms of
    test_derived_forms_over_two_columns -- through the general derived-input
    kernel instead of the product-pair variant (VAR 2 / 3), which the same
    query takes with the option on."""
    n = 100_003
    rng = np.random.default_rng(n + len(form) * 3 + len(pred))
    k = rng.integers(0, 64, n).astype(np.int64)
    a, b, c = rng.uniform(100, 200, n), rng.uniform(1e3, 1e5, n), rng.uniform(-1, 1, n)
    df = pl.DataFrame({"k": pl.Series.from_numpy("k", k), "a": pl.Series.from_numpy("a", a),
                       "b": pl.Series.from_numpy("b", b), "c": pl.Series.from_numpy("c", c)})
    forms = {"vwap": [("sum", col("a") * col("b")), ("sum", col("b"))],
             "vwap_rev": [("sum", col("b")), ("sum", col("a") * col("b"))],
             "vwap_swap": [("mean", col("b") * col("a")), ("sum", col("b"))]}[form]
    p = {"none": None, "on_a": col("a") > 150.0}[pred]
    names = [f"o{i}" for i in range(len(forms))]
    cols = {"k": (k, None), "a": (a, None), "b": (b, None), "c": (c, None)}
    okeys, _, oouts = _red_oracle(cols, ["k", "a", "b", "c"], "k", forms, p, n)
    for pair in (1, 0):
        plgpu_option("gb_pair", pair)
        lf = df.lazy() if p is None else df.lazy().filter(p)
        info = {}
        out = lf.group_by("k").agg(*[getattr(e, op)().alias(nm) for (op, e), nm in zip(forms, names)]).collect(info=info)
        assert info["path"] == 2, info
        _red_compare(out, "k", okeys, oouts, names)
        fv = fused_variant(info)
        assert fv["ran"] and (fv["var"] in (2, 3)) == bool(pair), (pair, fv)
        if not pair:
            assert fv["deriv"] and fv["var"] == 0, fv


def test_fused_grid_rounds(gpu, plgpu_option):
    """grid_rounds 1 and 8: the fused kernel's grid as that many rounds of
    the resident workgroups.  A 2^21-row run at 1 round reports the resident
    count R (its grid); the frame then has 8 R tiles of 1024 rows and a
    ragged one, the least at which 8 rounds are not clipped to one workgroup
    per tile: 8 * 1024 * R + 1027 rows, 4.2 M for R = 512 (2 workgroups per
    CU on 256 CUs).  Both grids bit-exact against the oracle and different."""
    plgpu_option("gb_path", 2)
    plgpu_option("plan_cache", 0)
    specs = _S("c", "b")

    def frame(n):
        rng = np.random.default_rng(n)
        cols = {"k": ((rng.integers(0, 300, n) * 7919 - 5).astype(np.int64), None),
                "c": (rng.uniform(10, 500, n), None), "b": (rng.uniform(0.5, 2.0, n), None),
                "d": (rng.uniform(-5, 5, n), None), "q": (rng.integers(-10**12, 10**12, n).astype(np.int64), None)}
        return pl.DataFrame([pl.Series.from_numpy(nm, v) for nm, (v, _) in cols.items()]), cols

    plgpu_option("grid_rounds", 1)
    df, _ = frame(1 << 21)
    _, info = _gb_gpu(df, "k", specs, None, False)
    resident = info["grid"]
    assert info["path"] == 2 and 0 < resident < 2048, info  # (2048 tiles: not clipped)
    n = 8 * 1024 * resident + 1027
    df, cols = frame(n)
    exp = _gb_oracle(cols, "k", specs, None, n)
    grids = {}
    for rounds in (1, 8):
        plgpu_option("grid_rounds", rounds)
        out, info = _gb_gpu(df, "k", specs, None, False)
        assert info["path"] == 2, info
        _gb_compare(out, "k", exp, len(specs), False, (rounds, info))
        grids[rounds] = info["grid"]
    assert grids[1] == resident and grids[8] == 8 * resident, (grids, resident)


@pytest.mark.parametrize("path", ["fused", "partitioned"])
def test_wave_report(gpu, plgpu_option, path):
    """wave_report 1: the kernels publish their diagnostics per wave instead
    of per workgroup.  One fused and one partitioned run, equal to the oracle
    and to the wave_report 0 run bit for bit."""
    plgpu_option("gb_path", 2 if path == "fused" else 3)
    plgpu_option("plan_cache", 0)
    plgpu_option("ktime", 1)
    df, cols = _part_frame(5_000, False)
    specs = _S("c", "b", "cn")
    exp = _gb_oracle(cols, "kn", specs, None, PART_N, names_extra=("w",))
    name = "gb_fast_wave_report_kernel" if path == "fused" else "gb_part_agg_wave_report_kernel"
    outs = []
    for wr in (0, 1):
        plgpu_option("wave_report", wr)
        (out, info), kt = _timed(lambda: _gb_gpu(df, "kn", specs, None, False))
        assert info["path"] == (2 if path == "fused" else 3), info
        _gb_compare(out, "kn", exp, len(specs), False, (path, wr, info))
        assert (name in kt) == bool(wr), (wr, sorted(kt))
        assert ("gb_fast_kernel" if path == "fused" else "gb_part_agg_kernel") in kt or wr, sorted(kt)
        gk, gkv = out["kn"].to_numpy().astype(np.int64), out["kn"].validity_numpy()
        order = np.lexsort((gk, ~gkv))
        outs.append([gkv[order], gk[order][gkv[order]]] +
                    [x for j in range(len(specs)) for x in (out[f"o{j}"].validity_numpy()[order],
                                                            _bits(out[f"o{j}"].to_numpy()[order]))])
    assert all(np.array_equal(x, y) for x, y in zip(*outs))


# ------------------------------------------------------------ radix join
@pytest.mark.parametrize("nl,nr,keys_per,ncarry", FORCED_CASES)
@pytest.mark.parametrize("batch", [8, 4])
@pytest.mark.parametrize("load", [10, 90])
def test_radix_join_sub_table_load(gpu, plgpu_option, load, batch, nl, nr, keys_per, ncarry):
    """join_radix_load 10 and 90 percent (the default is 35; 90 is the cap:
    the densest sub-tables and the longest probe runs) on the cases of
    test_radix_join_forced_vs_oracle, with both probe batch widths."""
    plgpu_option("join_radix", 2)
    plgpu_option("join_radix_keys", keys_per)
    plgpu_option("join_radix_batch", batch)
    plgpu_option("join_radix_load", load)
    left, right, lk, rk, lcols, pay = _forced_case(nl, nr, keys_per, ncarry)
    out, names = _rj_join(left, right)
    assert "rj_match_kernel" in names, names
    assert "rj_build_load_kernel" in names and "rj_build_kernel" not in names, names
    _rj_check(out, lk, rk, len(lcols) + 1, lcols, pay)
