"""Every operator on sliced (Arrow `offset` != 0) and borrowed, misaligned
columns.  A column reaches the library with an offset through the C ABI's
plgpu_column.offset, Series.slice and Series.from_device; the kernels pick
their code by where a column starts, and until this module every GPU test fed
them offset 0 in a fresh, 16-byte aligned upload.

One logical frame (host arrays) is laid out physically in several ways
(`LAYOUTS`, `_layout_frame`); every result is compared with one oracle result
computed from the host arrays, and with the `fresh` layout's result.  Rows
outside a slice are hostile junk (`_parent`): NaN / +-inf / 1e300, integer
extremes that occur nowhere in the logical rows (so a junk key is a new
group), validity bits the inverse of the neighbouring logical bit, strings
unlike any logical one whose bytes push the slice's first string off an
8-byte boundary.  Any read outside the slice changes a result.

Layouts
  fresh                 from_numpy, offset 0 (the control)
  off1 off63 off65      odd offsets
  off2 off62 off66      even, no multiple of 64
  off64 off1088         multiples of 64
  mixed                 each column in its own parent, offsets cycling through
                        64, 2, 0, 66, 128, 62
  ptr8                  borrowed (from_device): values at an allocation + 8
                        bytes, offset 0: naturally aligned, not 16-byte aligned
  bitmap_b1 .. b3       values fresh, bitmaps borrowed at an allocation + 1, 2,
                        3 bytes; `_off2`: the same at logical offset 2
  alias                 slices of ONE parent at offsets 2, 4, 6 under different
                        names (test_alias_*: its frame differs from the others')
Only natural alignment is used (the ABI's contract): no 8-byte column off a
multiple of 8, no 4-byte column off a multiple of 4.

The alignment gates, and the layouts that drive each to either side
  groupby.hip:2306-2328 gb_plan `ok` (the fused kernel: 8-byte columns,
      `(offset & 1) == 0`, values 16-byte aligned) and `ok_kp` (packed keys:
      the same, 8-byte aligned 4-byte keys, String data 8-byte aligned);
      groupby.hip:4040 kp_from_plan's copy of it.  Taken by fresh / off2 /
      off62 / off64 / off66 / off1088 / mixed / bitmap_b*; refused (generic
      kernel, path 0) by off1 / off63 / off65 / ptr8
      (test_launcher_branches_x_layouts, test_packed_keys_x_layouts).
  groupby.hip:2341-2348 gb_plan `wa` -> GbParams::vwords (whole validity
      words per wave, pair_word_wave) against groupby_kernels.hpp:1124-1225
      pair_word / pair_bit (`((validity & 3) * 8 + offset + r) & 31` per
      column).  vwords on fresh / off64 / off1088; off on off2 / off62 /
      off66 / mixed (columns of one call at different bit positions) /
      bitmap_b* (the `& 3` byte term).  fused_variant's bit 20 ("vwords")
      says which ran.
  groupby.hip:1501-1511 plan_groupby `same_col` (v_from / w_from), :1565 the
      pred_acc match, groupby_kernels.hpp:1947 same_dev_col (pair_normalize),
      join.hip:1968 the carried-column match: "the same column" by values,
      offset, dtype (and validity).  test_alias_* pass columns with equal
      values pointers that differ in offset only, and in validity only.
  groupby.hip:1737-1741 sq_split_kernel / :1885-1894 gb_materialize kind 3
      (the x * x split at `x.offset + i`, the parent's bitmap shared): the
      var rows on the generic and partitioned paths at off2 / off1
      (test_var_split_at_an_offset).
  Series.slice's null_count == -1: test_null_count_unknown.
  join.hip / sort.hip / rolling.hip (seg_starts.hpp seg_words: the start
      bitmap in place where the slice begins on an aligned 8-byte word, its
      repack otherwise: test_rolling_segmented_start_column; the same column
      into cumulative / lag, and at its own bit offset into fill / ewm:
      test_scans_segmented_start_column) / strings.hip /
      shuffle.hip / the interpreter's dev_load / dev_valid: section B below,
      on fresh / off1 / off2 / off63 / off64 / off65 / mixed.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import polaroid_amd as pl
import test_gpu_cumulative as TC
import test_gpu_ewm as TE
import test_gpu_fill as TF
from oracle import oracle as O
from polaroid_amd import _native as N
from polaroid_amd._native import fused_variant
from polaroid_amd.expr import col, lit, lower
from polaroid_amd.frame import _col_array
from test_gpu_fused_variants import CASES, N_PACKED, _POOL, _StrKeyAsInt, _check_var, _var_ref
from test_gpu_fused_variants import _frame as _variant_frame
from test_gpu_groupby_sweep import (MIXED, MIXED_NULLS, N as N_SWEEP, PATHS, PREDS, SUMONLY, _bits, _compare, _data,
                                    _gpu, _oracle, _set)

pytestmark = pytest.mark.gpu

TAIL = 131          # junk rows after every slice (at least 130)
_CYCLE = (64, 2, 0, 66, 128, 62)
OFFSETS = (1, 63, 65, 2, 62, 66, 64, 1088)
ODD = ("off1", "off63", "off65")
BITMAPS = tuple(f"bitmap_b{b}{s}" for s in ("", "_off2") for b in (1, 2, 3))
LAYOUTS = ("fresh",) + tuple(f"off{o}" for o in OFFSETS) + ("mixed", "ptr8") + BITMAPS
REFUSED = ODD + ("ptr8",)                      # the fused kernel's alignment gate refuses these
VWORDS = ("fresh", "off64", "off1088")         # whole-word validity reads
B_LAYOUTS = ("fresh", "off1", "off2", "off63", "off64", "off65", "mixed")
NAN_BITS = np.uint64(0x7FF8000000000000)


# ------------------------------------------------------------ 0. layouts
def _junk(v, m, phase=0):
    """m hostile values of v's dtype, none of them a logical value of an
    integer column."""
    if m == 0:
        return v[:0].copy()
    if v.dtype == object:
        return np.array([f"~junk{phase + j}~" + "x" * ((phase + j) % 5) for j in range(m)], dtype=object)
    if v.dtype == np.bool_:
        raise AssertionError("Boolean junk is the inverse of the neighbouring bit (_parent)")
    if v.dtype.kind == "f":
        big = 1e300 if v.dtype == np.float64 else 3e38
        pool = np.array([np.nan, np.inf, -np.inf, big, -big], v.dtype)
    else:
        ii = np.iinfo(v.dtype)
        cand = np.array([ii.max, ii.min, ii.max - 1, ii.min + 1, ii.max - 2, ii.min + 2, ii.max - 3, ii.min + 3],
                        v.dtype)
        pool = cand[~np.isin(cand, v)]
        if not pool.size:
            assert v.dtype.itemsize == 1  # (a 1-byte column can hold every value: plain extremes then)
            pool = cand
    return pool[(phase + np.arange(m)) % pool.size]


def _inverse_of(bits, m, first):
    """m validity (or Boolean value) bits, the inverse of the neighbouring logical bit."""
    if bits.size == 0:
        return np.ones(m, bool)
    return np.full(m, not bool(bits[0] if first else bits[-1]))


def _parent(v, valid, off, tail=TAIL):
    """The parent buffers of a slice [off, off + n): junk, the logical rows, junk."""
    if v.dtype == np.bool_:
        pv = np.concatenate([_inverse_of(v, off, True), v, _inverse_of(v, tail, False)])
    else:
        front = _junk(v, off)
        if v.dtype == object and off and sum(len(s) for s in front) % 8 == 0:
            front[0] += "y"   # the slice's first string starts off an 8-byte boundary
        pv = np.concatenate([front, v, _junk(v, tail, 3)])
    pvalid = None
    if valid is not None:
        pvalid = np.concatenate([_inverse_of(valid, off, True), valid, _inverse_of(valid, tail, False)])
    return pv, pvalid


def _upload_bytes(arr, shift=0):
    """A device allocation holding `arr` from byte `shift` on."""
    arr = np.ascontiguousarray(arr).view(np.uint8)
    buf = N.DeviceBuffer(arr.nbytes + shift + 16)
    assert buf.ptr % 8 == 0
    if arr.nbytes:
        N.check(N.lib().plgpu_memcpy_h2d(C.c_void_p(buf.ptr + shift), arr.ctypes.data_as(C.c_void_p), arr.nbytes, None))
    return buf


def _spec(layout, j):
    """(how, offset, bitmap byte shift) of column j in `layout`."""
    if layout == "fresh":
        return "fresh", 0, 0
    if layout == "mixed":
        return "slice", _CYCLE[j % len(_CYCLE)], 0
    if layout == "ptr8":
        return "ptr8", 0, 0
    if layout.startswith("bitmap_b"):
        return "bitmap", 2 if layout.endswith("_off2") else 0, int(layout[8])
    return "slice", int(layout[3:]), 0


def _place(name, v, valid, how, off=0, shift=0):
    """The logical column (v, valid) as a device Series in one physical layout."""
    n = v.shape[0]
    if how == "fresh" or (how == "ptr8" and v.dtype == np.bool_):
        return pl.Series.from_numpy(name, v, valid)
    if how == "slice":
        pv, pvalid = _parent(v, valid, off)
        s = pl.Series.from_numpy(name, pv, pvalid).slice(off, n)
        assert s.len() == n and int(s._col.offset) == off
        return s
    if how == "ptr8":
        front = 1 if v.dtype == object else 8 // v.dtype.itemsize
        pv, _ = _parent(v, None, front)
        base = pl.Series.from_numpy(name, pv)
        keep, vptr = [base], None
        if valid is not None:
            keep.append(_upload_bytes(np.packbits(valid, bitorder="little")))
            vptr = keep[-1].ptr
        return pl.Series.from_device(name, base.dtype, int(base._col.values) + 8, n, validity_ptr=vptr, offset=0,
                                     keepalive=keep, data_ptr=base._col.data or None)
    assert how == "bitmap"
    pv, pvalid = _parent(v, valid, off)
    base = pl.Series.from_numpy(name, pv)
    if valid is None:
        return base.slice(off, n)
    vbuf = _upload_bytes(np.packbits(pvalid, bitorder="little"), shift)
    return pl.Series.from_device(name, base.dtype, int(base._col.values), n, validity_ptr=vbuf.ptr + shift,
                                 offset=off, keepalive=[base, vbuf], data_ptr=base._col.data or None)


def _layout(cols, layout, names=None):
    """{name: (values, valid)} -> DataFrame of the same logical frame in `layout`."""
    series = []
    for j, (nm, (v, valid)) in enumerate(cols.items()):
        if names is None or nm in names:
            series.append(_place(nm, v, valid, *_spec(layout, j)))
    return pl.DataFrame(series)


@functools.lru_cache(maxsize=None)
def _host(kind):
    """The host arrays of the frames: the sweep's (random / sorted keys) and
    the launcher-branch frames (plus their String key s)."""
    if kind in ("sweep", "sweep_sorted"):
        df, cols = _data(2024 if kind == "sweep" else 77, sorted_keys=kind == "sweep_sorted")
        return df, cols
    df, cols = _variant_frame(kind)
    cols = dict(cols)
    cols["s"] = (_POOL[cols["i"][0] + 50], None)
    return df, cols


@functools.lru_cache(maxsize=3)
def _layout_frame(kind, layout):
    df, cols = _host(kind)
    return df if layout == "fresh" else _layout(cols, layout)


def _canon(out, key, names, maintain):
    """A result in comparable form: rows in key order where the order is
    unspecified, values as bits (every NaN one value, null slots zero)."""
    order, res = np.arange(out.height), []
    if key is not None:
        gk, gkv = out[key].to_numpy(), out[key].validity_numpy()
        kk = np.where(gkv, gk.astype(str), "") if gk.dtype == object else np.where(gkv, gk, 0)
        if not maintain:
            order = np.lexsort((kk, ~gkv))
        res.append((gkv[order], kk[order]))
    for nm in names:
        v, ok = out[nm].to_numpy()[order], out[nm].validity_numpy()[order]
        if v.dtype.kind == "f":
            b = v.astype(np.float64).view(np.uint64).copy()
            b[np.isnan(v)] = NAN_BITS
        else:
            b = v.astype(np.int64)
        res.append((ok, np.where(ok, b, 0)))
    return res


def _assert_same(a, b, tag):
    assert len(a) == len(b), tag
    for j, ((av, ab), (bv, bb)) in enumerate(zip(a, b)):
        assert np.array_equal(av, bv) and np.array_equal(ab, bb), (tag, j, "differs from the fresh layout")


# --------------------------------------------- A1. group-by paths x layouts
FAMILIES = {"sumonly4": SUMONLY[:4], "mixed": MIXED, "nulls": MIXED_NULLS}
_A1_ORACLE, _A1_FRESH = {}, {}


def _a1_queries():
    for fam, pool in FAMILIES.items():
        for pname in ("none", "simple"):
            for key in ("k", "kn"):
                yield fam, [(kind, col(c)) for kind, c in pool], pname, key


@pytest.mark.parametrize("layout,path", [(la, p) for la in LAYOUTS[1:] for p in PATHS])
def test_groupby_paths_x_layouts(gpu, plgpu_option, layout, path):
    """Every group-by path x every layout x (sum-only, mixed, nullable
    aggregations) x (plain, nullable key) x (no, simple predicate) x
    maintain_order: bit for bit the oracle's result (first-occurrence order
    included) and the fresh layout's."""
    kind = "sweep_sorted" if path == "fused_runs" else "sweep"
    fresh, cols = _host(kind)
    df = _layout_frame(kind, layout)
    _set(plgpu_option, path)
    for fam, specs, pname, key in _a1_queries():
        pf = PREDS[pname]
        ck = (kind, fam, pname, key)
        if ck not in _A1_ORACLE:
            _A1_ORACLE[ck] = _oracle(cols, key, specs, pf() if pf else None, N_SWEEP)
        names = [f"o{j}" for j in range(len(specs))]
        for maintain in (False, True):
            out, info = _gpu(df, key, specs, pf() if pf else None, maintain)
            tag = (layout, path, fam, pname, key, maintain, info.get("path"))
            _compare(out, key, _A1_ORACLE[ck], len(specs), maintain, tag)
            fk = (path,) + ck + (maintain,)
            if fk not in _A1_FRESH:
                fout, _ = _gpu(fresh, key, specs, pf() if pf else None, maintain)
                _A1_FRESH[fk] = _canon(fout, key, names, maintain)
            _assert_same(_canon(out, key, names, maintain), _A1_FRESH[fk], tag)
            if path in ("fused", "fused_runs") and layout in REFUSED:
                assert info["path"] == 0 and not fused_variant(info)["ran"], tag
            elif path in ("fused", "fused_runs"):
                assert info["path"] in (1, 2) and fused_variant(info)["ran"], tag
            elif path in ("part1", "part2"):
                assert info["path"] == 3, tag


# ---------------------------------------- A2. launcher branches x layouts
A2_IDS = ("nulls_var5_nacc4", "nulls_sumonly2_pred", "nulls_general_nopred", "nulls_general_pred", "fast_sumonly2",
          "fast_mixed3", "fast_runs_sumonly", "fast_deriv2", "pair2_2limb", "pair3_3limb", "var4", "var1_3limb")
_CASE = {c[0]: c for c in CASES}
_A2_ORACLE = {}


def _run_case(plgpu_option, cid, layout, opts=None):
    """One row of test_gpu_fused_variants.CASES on `layout`: oracle-exact as
    there; returns (info, the row's expected variant)."""
    _, kind, key, build, pred, maintain, copts, expect = _CASE[cid]
    _, cols = _host(kind)
    df = _layout_frame(kind, layout)
    n = N_PACKED if kind == "packed" else N_SWEEP
    for name, value in (copts if opts is None else opts).items():
        plgpu_option(name, value)
    if isinstance(build, tuple):
        _, xname, ddof = build
        return _check_var(df, cols, key, xname, ddof, pred, maintain, n), expect
    specs = build()
    if cid not in _A2_ORACLE:
        _A2_ORACLE[cid] = _oracle(cols, "i" if key == "s" else key, specs, pred() if pred else None, n,
                                  names_extra=("w",))
    out, info = _gpu(df, key, specs, pred() if pred else None, maintain)
    if key == "s":
        out, key = _StrKeyAsInt(out), "i"
    _compare(out, key, _A2_ORACLE[cid], len(specs), maintain, (cid, layout, info))
    return info, expect


def _assert_variant(info, expect, tag):
    """The assertions of test_fused_variant_vs_oracle: the row's own instantiation ran."""
    fv = fused_variant(info)
    assert fv["ran"], (tag, "the fused kernel did not run", info)
    assert {name: fv[name] for name in expect} == expect, (tag, fv, info)
    assert info["path"] == (4 if expect["var"] in (1, 4) else 2 if expect["sumonly"] else 1), (tag, info)
    assert info["sum_limbs"] == (expect["limbs"] if expect["sumonly"] else 3), (tag, info)
    assert info["key_pack"] == (1 if expect.get("pack", 0) else 0), (tag, info)
    return fv


@pytest.mark.parametrize("layout,cid", [(la, c) for la in LAYOUTS for c in A2_IDS])
def test_launcher_branches_x_layouts(gpu, plgpu_option, layout, cid):
    """The fused kernel forced: on even offsets of 16-byte aligned buffers
    the same instantiation as on a fresh column (NULLS rows: whole-word
    validity reads exactly where every bitmap allows them); on odd offsets
    and 8-byte aligned values the gate refuses and the generic kernel runs."""
    info, expect = _run_case(plgpu_option, cid, layout)
    tag = (cid, layout)
    if layout in REFUSED:
        assert info["path"] == 0, (tag, info)
        assert fused_variant(info)["ran"] is False, (tag, info)
        return
    fv = _assert_variant(info, expect, tag)
    assert fv["vwords"] == (bool(expect.get("nulls")) and layout in VWORDS), (tag, fv)


@pytest.mark.parametrize("layout", ["off2", "off1"])
@pytest.mark.parametrize("gb_path", [0, 3])
@pytest.mark.parametrize("cid", ["var4", "var1_3limb"])
def test_var_split_at_an_offset(gpu, plgpu_option, cid, gb_path, layout):
    """var() off the fused kernel: gb_materialize's x * x split (kind 3)
    writes at the column's own offset and shares the parent's bitmap."""
    opts = {"gb_path": gb_path}
    if gb_path == 3:
        opts.update(part_levels=1, part_bits=6)
    info, _ = _run_case(plgpu_option, cid, layout, opts)
    assert info["path"] == gb_path and not fused_variant(info)["ran"], (cid, layout, info)


@pytest.mark.parametrize("layout", ["off2", "off64", "off1"])
@pytest.mark.parametrize("cid", ["fast_sumonly2_pack1", "fast_sumonly2_pack2"])
def test_packed_keys_x_layouts(gpu, plgpu_option, cid, layout):
    """Keys packed in the fused kernel's registers (an Int32 key, a short
    String key whose slice starts off an 8-byte boundary of its bytes): packed
    on even offsets, refused (a key / code column) on an odd one."""
    if cid.endswith("pack2") and layout != "fresh":
        s = _layout_frame("packed", layout)["s"]
        first = N.download_many([(int(s._col.values) + 8 * int(s._col.offset), 8)])[0].view(np.int64)[0]
        assert first % 8 != 0, "the slice's first string must start off an 8-byte boundary"
    info, expect = _run_case(plgpu_option, cid, layout)
    if layout == "off1":
        assert info["key_pack"] == 0, (cid, layout, info)
    else:
        _assert_variant(info, expect, (cid, layout))


# ------------------------------------------------------------ A3. aliasing
ALIAS_PATHS = ("fused", "generic_global", "part1")


@functools.lru_cache(maxsize=None)
def _alias():
    """x0, x1, x2: slices of one parent P of n + 200 rows at offsets 2, 4, 6
    (junk in P's first 6 rows and after row n + 2: each slice sees some of it
    as its own logical rows); y0 / y1: the same values and offset, with and
    without a bitmap."""
    n = N_SWEEP
    _, cols = _host("sweep")
    rng = np.random.default_rng(99)
    P = np.empty(n + 200)
    P[:6] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    P[6:n + 2] = rng.uniform(10, 500, n - 4)
    P[n + 2:] = _junk(P, 198, 3)
    yv = rng.random(n) > 0.1
    pvalid = np.concatenate([_inverse_of(yv, 4, True), yv, _inverse_of(yv, 196, False)])
    par = pl.Series.from_numpy("P", P)
    vbuf = _upload_bytes(np.packbits(pvalid, bitorder="little"))
    host = {nm: cols[nm] for nm in ("k", "kn", "c", "b", "d", "q")}
    series = [pl.Series.from_numpy(nm, *host[nm]) for nm in host]
    for j in range(3):
        host[f"x{j}"] = (P[2 + 2 * j: 2 + 2 * j + n].copy(), None)
        series.append(par.slice(2 + 2 * j, n).alias(f"x{j}"))
    host["y0"], host["y1"] = (P[4:4 + n].copy(), yv), (P[4:4 + n].copy(), None)
    series.append(pl.Series.from_device("y0", pl.Float64, int(par._col.values), n, validity_ptr=vbuf.ptr, offset=4,
                                        keepalive=[par, vbuf]))
    series.append(par.slice(4, n).alias("y1"))
    ptrs = {int(s._col.values) for s in series[-5:]}
    assert len(ptrs) == 1, "the aliased columns share one values pointer"
    return pl.DataFrame(series), host


def _S(*names):
    return [("sum", col(nm)) for nm in names]


ALIAS_QUERIES = {
    "sum3_pred_x1": (lambda: _S("x0", "x1", "x2"), lambda: col("x1") > 250.0),
    "sum3_pred_x0": (lambda: _S("x0", "x1", "x2"), lambda: col("x0") > 250.0),
    "prod_next_to_x1": (lambda: [("sum", col("x0") * col("x1"))] + _S("x1"), None),
    "prod_next_to_x0": (lambda: [("sum", col("x0") * col("x1"))] + _S("x0"), None),
    "x1_next_to_prod": (lambda: _S("x1") + [("sum", col("x0") * col("x1"))], lambda: col("x1") > 250.0),
    "square": (lambda: [("sum", col("x1") * col("x1"))], None),
    "bitmap_first": (lambda: _S("y0", "y1"), lambda: col("y1") > 250.0),
    "bitmap_second": (lambda: _S("y1", "y0"), lambda: col("y1") > 250.0),
}


@pytest.mark.parametrize("path", ALIAS_PATHS)
@pytest.mark.parametrize("query", list(ALIAS_QUERIES))
def test_alias_groupby(gpu, plgpu_option, query, path):
    """Columns of one call with equal values pointers that differ in offset
    only (or in validity only): none may be taken for another."""
    df, host = _alias()
    build, pred = ALIAS_QUERIES[query]
    specs = build()
    extra = tuple(nm for nm in host if nm[0] in "xy")
    exp = _oracle(host, "k", specs, pred() if pred else None, N_SWEEP, names_extra=extra)
    _set(plgpu_option, path)
    for maintain in (False, True):
        out, info = _gpu(df, "k", specs, pred() if pred else None, maintain)
        _compare(out, "k", exp, len(specs), maintain, (query, path, maintain, info))
        if path == "fused":
            assert fused_variant(info)["ran"], (query, maintain, info)  # (even offsets: the gate takes them)


@pytest.mark.parametrize("path", ALIAS_PATHS)
def test_alias_var_next_to_sum(gpu, plgpu_option, path):
    """x0.var() next to x1.sum(): the variance triple's x * x split of one
    slice beside the sum of another slice of the same buffer."""
    df, host = _alias()
    n = N_SWEEP
    _set(plgpu_option, path)
    exp = _oracle(host, "k", _S("x1"), None, n, names_extra=("x1",))
    okeys, _, oouts = exp
    want_sum = dict(zip(okeys.tolist(), _bits(oouts[0][0]).tolist()))
    out = df.lazy().group_by("k").agg(col("x0").var().alias("v"), col("x1").sum().alias("s")).collect()
    k, x0 = host["k"][0], host["x0"][0]
    gk, gv, gok = out["k"].to_numpy(), out["v"].to_numpy(), out["v"].validity_numpy()
    gs = out["s"].to_numpy()
    assert sorted(gk.tolist()) == sorted(want_sum)
    for g in range(out.height):
        vals = x0[k == gk[g]]
        want = np.uint64(want_sum[int(gk[g])]).view(np.float64)
        assert _bits(gs[g]) == _bits(want) or (np.isnan(gs[g]) and np.isnan(want)), (path, g, gs[g], want)
        if vals.shape[0] <= 1:
            assert not gok[g], (path, g)
        elif not np.isfinite(vals).all():
            assert gok[g] and np.isnan(gv[g]), (path, g, gv[g])
        else:
            assert gok[g] and _bits(gv[g]) == _bits(_var_ref(vals, 1)), (path, g, gv[g])


def test_alias_filter_and_join(gpu):
    """filter (outputs x0, x1; predicate on x1) and join (payloads x0, x1 of
    the left frame) over two slices of one buffer."""
    df, host = _alias()
    x0, x1, k = host["x0"][0], host["x1"][0], host["k"][0]
    sub = pl.DataFrame([df["k"], df["x0"], df["x1"]])
    out = sub.filter(col("x1") > 250.0)
    m = x1 > 250.0
    assert out.height == int(m.sum())
    assert np.array_equal(_bits(out["x0"].to_numpy()), _bits(x0[m]))
    assert np.array_equal(_bits(out["x1"].to_numpy()), _bits(x1[m]))
    assert np.array_equal(out["k"].to_numpy(), k[m])
    rk = np.unique(k)[::3].copy()
    right = pl.DataFrame([pl.Series.from_numpy("k", rk), pl.Series.from_numpy("p", np.arange(rk.shape[0]))])
    ol, orr = O.join_inner(O.HostCol(k), O.HostCol(rk))
    for order in ("left", "none"):
        j = sub.join(right, on="k", maintain_order=order)
        assert j.height == ol.shape[0]
        g0, g1, gp = _bits(j["x0"].to_numpy()), _bits(j["x1"].to_numpy()), j["p"].to_numpy().astype(np.int64)
        e0, e1 = _bits(x0[ol]), _bits(x1[ol])
        if order == "none":
            a, b = np.lexsort((g1, g0, gp)), np.lexsort((e1, e0, orr))
            g0, g1, gp, e0, e1, eo = g0[a], g1[a], gp[a], e0[b], e1[b], orr[b]
        else:
            eo = orr
        assert np.array_equal(g0, e0) and np.array_equal(g1, e1) and np.array_equal(gp, eo), order


# ------------------------------------------------- A4. null_count == -1
def _nc_cases():
    rng = np.random.default_rng(41)
    n, off = 5000, 70
    k = (rng.integers(0, 40, n) * 13).astype(np.int64)
    x = rng.uniform(-100, 100, n)
    q = rng.integers(-10**9, 10**9, n).astype(np.int64)
    ones, zeros = np.ones(n, bool), np.zeros(n, bool)
    return {"no_null": (n, off, k, x, q, ones), "only_nulls": (n, off, k, x, q, zeros),
            "one_row": (1, 3, k[:1], x[:1], q[:1], ones[:1]), "one_null_row": (1, 3, k[:1], x[:1], q[:1], zeros[:1])}


NC_KINDS = ("sum", "mean", "min", "count", "first", "last")


@pytest.mark.parametrize("case", ["no_null", "only_nulls", "one_row", "one_null_row"])
@pytest.mark.parametrize("keyed", [True, False])
def test_null_count_unknown(gpu, case, keyed):
    """Slices of nullable parents carry null_count == -1: a slice without a
    null, of nulls only, of one row; keyed and keyless (nkeys = 0)."""
    n, off, k, x, q, valid = _nc_cases()[case]
    host = {"k": (k, None), "x": (x, valid), "q": (q, valid)}
    zero = (np.zeros(n), None)
    full = dict(host, c=zero, b=zero, d=zero)
    df = _layout(host, f"off{off}")
    for nm in ("x", "q"):
        assert df[nm]._col.null_count == -1 and df[nm]._col.validity and df[nm]._col.offset == off
        parent_valid = df[nm]._keep[0].validity_numpy()
        assert parent_valid[off - 1] != valid[0] and parent_valid[off + n] != valid[-1]  # the parent has both
    specs = [(kind, col(nm)) for nm in ("x", "q") for kind in NC_KINDS]
    key = "k" if keyed else None
    exp = _oracle(full, key, specs, None, n, names_extra=("x",))
    for maintain in ((False, True) if keyed else (False,)):
        out, info = _gpu(df, key, specs, None, maintain)
        _compare(out, key, exp, len(specs), maintain, (case, keyed, maintain, info))


def test_typed_reductions_mixed_layout(gpu):
    """first / last and the keyless reductions over Int8 / UInt16 / UInt64 /
    Float32 columns, each at its own offset: the fresh layout's result."""
    rng = np.random.default_rng(8)
    n = 30_000
    host = {"k": (rng.integers(-20, 20, n).astype(np.int64), rng.random(n) > 0.03),
            "i8": (rng.integers(-128, 127, n).astype(np.int8), rng.random(n) > 0.1),
            "u16": (rng.integers(0, 65535, n).astype(np.uint16), rng.random(n) > 0.1),
            "f": (rng.random(n), None),
            "u64": (rng.integers(0, 2**63, n).astype(np.uint64) * np.uint64(2), rng.random(n) > 0.1),
            "f32": ((rng.standard_normal(n) * 1e3).astype(np.float32), rng.random(n) > 0.1)}
    kinds = ("sum", "mean", "min", "max", "first", "last", "count")
    typed = ("i8", "u16", "u64", "f32")
    sel = host["f"][0] > 0.3
    res = {}
    for layout in ("fresh", "mixed", "off1"):
        df = _layout(host, layout)
        for nm in typed:
            aggs = [getattr(col(nm), kind)().alias(kind) for kind in kinds]
            for keyed in (True, False):
                lf = df.lazy().filter(col("f") > 0.3)
                out = (lf.group_by("k", maintain_order=True).agg(*aggs) if keyed else lf.select(*aggs)).collect()
                res[layout, nm, keyed] = _canon(out, "k" if keyed else None, kinds, True)
                if keyed:
                    continue
                # the keyless result against numpy
                v, ok = host[nm][0][sel], host[nm][1][sel]
                assert out["count"].to_list() == [int(ok.sum())], (layout, nm)
                assert out["first"].to_list() == [v[0].item() if ok[0] else None], (layout, nm)
                assert out["last"].to_list() == [v[-1].item() if ok[-1] else None], (layout, nm)
                assert out["min"].to_list() == [v[ok].min().item()], (layout, nm)
                assert out["max"].to_list() == [v[ok].max().item()], (layout, nm)
    for layout in ("mixed", "off1"):
        for nm in typed:
            for keyed in (True, False):
                _assert_same(res[layout, nm, keyed], res["fresh", nm, keyed], (layout, nm, keyed))


# ------------------------------------------------------------ B. gather
def _take_check(got, v, valid, idx, iok, tag):
    ok = iok & (valid[np.where(iok, idx, 0)] if valid is not None else True)
    assert got.len() == idx.shape[0], tag
    assert np.array_equal(got.validity_numpy(), ok), tag
    want = v[np.where(iok, idx, 0)]
    g = got.to_numpy()
    if v.dtype == object:
        assert g[ok].tolist() == want[ok].tolist(), tag
    else:
        assert np.array_equal(g[ok].view(np.uint8), want[ok].view(np.uint8)), tag


@functools.lru_cache(maxsize=None)
def _gather_host():
    rng = np.random.default_rng(21)
    n = 10_000
    words = np.array(["", "a", "bc", "defghijk", "lmnopqrstuvwxyz0123", "é"], dtype=object)
    ok = lambda: rng.random(n) > 0.15  # noqa: E731
    return {"f64": (rng.standard_normal(n), ok()), "i64": (rng.integers(-2**62, 2**62, n).astype(np.int64), None),
            "i32": (rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), ok()),
            "u16": (rng.integers(0, 65535, n).astype(np.uint16), ok()),
            "i8": (rng.integers(-128, 127, n).astype(np.int8), ok()),
            "u8": (rng.integers(0, 255, n).astype(np.uint8), None),
            "bool": (rng.random(n) > 0.5, ok()), "str": (words[rng.integers(0, 6, n)], ok()),
            "f32": (rng.standard_normal(n).astype(np.float32), None)}


@pytest.mark.parametrize("ioff", [0, 1, 64])
@pytest.mark.parametrize("layout", B_LAYOUTS)
def test_gather_sliced(gpu, layout, ioff):
    """plgpu_gather: sliced sources of every width, Boolean and String,
    nullable, through a sliced nullable UInt32 index; numpy's take."""
    host = _gather_host()
    n = 10_000
    rng = np.random.default_rng(5 + ioff)
    idx = rng.integers(0, n, n + 37).astype(np.uint32)
    idx[:100] = idx[0]
    iok = rng.random(n + 37) > 0.1
    s_idx = _place("idx", idx, iok, "slice" if ioff else "fresh", ioff)
    df = _layout(host, layout)
    series = [df[nm] for nm in host]
    out = (N.Column * len(series))()
    N.check(N.lib().plgpu_gather(_col_array(series), len(series), C.byref(s_idx._col), out, None))
    got = [pl.Series._from_native(s.name, out[i]) for i, s in enumerate(series)]
    for g, (nm, (v, valid)) in zip(got, host.items()):
        _take_check(g, v, valid, idx.astype(np.int64), iok, (layout, ioff, nm))
    # one column at a time (Series.gather) agrees
    for nm in ("f64", "str", "bool"):
        _take_check(df[nm].gather(s_idx), *host[nm], idx.astype(np.int64), iok, (layout, ioff, nm, "single"))


# -------------------------------------------------------------- B. sort
SORT_NP = {"Int8": np.int8, "Int16": np.int16, "Int32": np.int32, "Int64": np.int64, "UInt8": np.uint8,
           "UInt16": np.uint16, "UInt32": np.uint32, "UInt64": np.uint64, "Float32": np.float32,
           "Float64": np.float64, "Boolean": np.bool_, "String": object}


@functools.lru_cache(maxsize=None)
def _sort_host():
    from test_gpu_dtypes import rand

    rng = np.random.default_rng(17)
    n = 40_000
    words = np.array([f"w{j % 97:02d}" + "z" * (j % 11) for j in range(400)] + [""], dtype=object)
    host = {}
    for name in SORT_NP:
        if name == "Boolean":
            v = rng.random(n) > 0.4
        elif name == "String":
            v = words[rng.integers(0, words.shape[0], n)]
        else:
            v = rand(name, n, rng)
            v[rng.random(n) < 0.3] = v[0]  # ties: the sort is stable
        host[name] = (v, rng.random(n) > 0.05)
    return host


def _str_codes(v):
    """Strings as the ranks of their UTF-8 bytes (the oracle sorts integers)."""
    enc = np.array([s.encode() for s in v], dtype=object)
    uniq = sorted(set(enc.tolist()))
    rank = {b: j for j, b in enumerate(uniq)}
    return np.array([rank[b] for b in enc.tolist()], np.int64)


def _sort_key(v):
    """A column in a form O.arg_sort_multi orders as the library must (it
    takes Float64 and what fits Int64): String and UInt64 as ranks."""
    if v.dtype == object:
        return _str_codes(v)
    if v.dtype == np.uint64:
        return np.unique(v, return_inverse=True)[1].reshape(-1).astype(np.int64)
    return v.astype(np.float64) if v.dtype == np.float32 else v


@pytest.mark.parametrize("layout", B_LAYOUTS)
def test_arg_sort_sliced(gpu, layout):
    """arg_sort of every dtype, nullable, descending / nulls_last both ways,
    and three key columns at different offsets: the oracle's permutation."""
    host = _sort_host()
    df = _layout(host, layout)
    for name, (v, valid) in host.items():
        hc = None if name in ("Boolean", "String") else O.HostCol(v, valid)
        for desc in (False, True):
            for nl in (False, True):
                got = df[name].arg_sort(descending=desc, nulls_last=nl).to_numpy().astype(np.int64)
                want = (O.arg_sort(hc, desc, nl) if hc is not None
                        else O.arg_sort_multi([(_sort_key(v), valid)], [desc], [nl]))
                assert np.array_equal(got, want), (layout, name, desc, nl)
    for by in (("Int8", "String", "Float64"), ("Boolean", "UInt16", "Int64"), ("Int32", "Float32", "UInt64")):
        for desc, nl in (((False, True, False), (False, False, True)), ((True, False, True), (True, True, False))):
            out = N.Column()
            keys = [df[nm] for nm in by]
            N.check(N.lib().plgpu_arg_sort_multi(_col_array(keys), 3, (C.c_int32 * 3)(*map(int, desc)),
                                                 (C.c_int32 * 3)(*map(int, nl)), C.byref(out), None))
            got = pl.Series._from_native("i", out).to_numpy().astype(np.int64)
            want = O.arg_sort_multi([(_sort_key(host[nm][0]), host[nm][1]) for nm in by], list(desc), list(nl))
            assert np.array_equal(got, want), (layout, by, desc, nl)


# ----------------------------------------------------------- B. rolling
ROLL_N = 3 * 4096 + 37


@functools.lru_cache(maxsize=None)
def _roll_host():
    rng = np.random.default_rng(33)
    n = ROLL_N
    ok = lambda: rng.random(n) > 0.1  # noqa: E731
    return {"Float64": (rng.uniform(10, 500, n) * np.exp(0.02 * rng.standard_normal(n)), ok()),
            "Int64": (rng.integers(-10**9, 10**9, n).astype(np.int64), ok()),
            "Int32": (rng.integers(-10**6, 10**6, n).astype(np.int32), ok())}


_ROLL_ORACLE = {}


def _roll_oracle(name, kind, w, ms, center):
    ck = (name, kind, w, ms, center)
    if ck not in _ROLL_ORACLE:
        v, valid = _roll_host()[name]
        hc = O.HostCol(v, valid)
        if kind in ("var", "std"):
            _ROLL_ORACLE[ck] = O.rolling_var(hc, w, ms, center, 1, kind == "std", O.ROLLING_EXACT)
        else:
            _ROLL_ORACLE[ck] = O.rolling(hc, kind, w, ms, center, O.ROLLING_EXACT)
    return _ROLL_ORACLE[ck]


@pytest.mark.parametrize("layout", B_LAYOUTS)
def test_rolling_sliced(gpu, layout):
    """plgpu_rolling over sliced nullable columns: the exact oracle, bit for bit."""
    host = _roll_host()
    df = _layout(host, layout)
    for name in host:
        s = df[name]
        for kind in ("sum", "mean", "min", "max", "var", "std"):
            for w in (1, 7, 64, 65):
                for ms in (1, w):
                    for center in (False, True):
                        out = getattr(s, "rolling_" + kind)(w, min_samples=ms, center=center)
                        gv, gok = out.to_numpy(), out.validity_numpy()
                        ev, eok = _roll_oracle(name, kind, w, ms, center)
                        tag = (layout, name, kind, w, ms, center)
                        assert np.array_equal(gok, eok), tag
                        if gv.dtype.kind in "iu":
                            assert np.array_equal(gv[gok].astype(np.int64), ev[eok].astype(np.int64)), tag
                        else:
                            g, e = gv[gok].astype(np.float64), ev[eok].astype(np.float64)
                            assert np.array_equal(np.isnan(g), np.isnan(e)), tag
                            m = ~np.isnan(e)
                            assert np.array_equal(_bits(g[m]), _bits(e[m])), tag


@pytest.mark.parametrize("soff", [0, 64, 8, 3])
def test_rolling_segmented_start_column(gpu, soff):
    """plgpu_rolling_segmented with the Boolean start column sliced: offset
    64 (the slice starts on an 8-byte word: the bitmap is used in place), 8
    (a whole byte but no aligned word) and 3 (repacked); the parent's bits
    are set in the junk after the slice, whose last word they share."""
    rng = np.random.default_rng(44)
    n = ROLL_N
    v = rng.uniform(-50, 50, n)
    valid = rng.random(n) > 0.1
    starts = np.append(True, rng.random(n - 1) < 0.01)
    starts[-1] = False  # the junk after the slice is its inverse: set bits
    seg = _place("seg", starts, None, "slice" if soff else "fresh", soff)
    if soff:
        assert seg._keep[0].to_numpy()[soff + n:].all()
    x = _place("x", v, valid, "slice", 66)
    seg_id = np.cumsum(starts) - 1
    for kind in ("sum", "min"):
        for w, ms in ((7, 1), (65, 65)):
            out = x._rolling(N.ROLLING[kind], w, ms, False, seg=seg)
            gv, gok = out.to_numpy(), out.validity_numpy()
            ev, eok = np.zeros(n), np.zeros(n, bool)
            for sid in np.unique(seg_id):
                rows = np.flatnonzero(seg_id == sid)
                e, ok = O.rolling(O.HostCol(v[rows], valid[rows]), kind, w, ms, False, O.ROLLING_EXACT)
                ev[rows], eok[rows] = e, ok
            assert np.array_equal(gok, eok), (soff, kind, w)
            assert np.array_equal(_bits(gv[gok]), _bits(ev[eok])), (soff, kind, w)


SCAN_N = N.CUM_TILE + N.CUM_BLOCK + 5  # one tile, one block and a ragged tail: a carry, a block hand-over, a partial word


@functools.lru_cache(maxsize=None)
def _scan_host():
    """The columns of test_scans_segmented_start_column and what every scan
    must give, by the per-segment numpy folds of the operators' own modules."""
    rng = np.random.default_rng(45)
    n = SCAN_N
    valid = rng.random(n) > 0.1
    starts = np.append(True, rng.random(n - 1) < 0.01)
    starts[-1] = False  # the junk after the slice is its inverse: set bits
    i64 = rng.integers(-10**12, 10**12, n).astype(np.int64)
    f64 = rng.uniform(-50, 50, n)
    first = TC._seg_info(starts)
    exp = {("cum", "sum"): TC._ref(i64, valid, first, "sum"), ("cum", "max"): TC._ref(f64, valid, first, "max"),
           ("lag", "shift", 1): TC._lag_ref(f64, valid, first, "shift", 1),
           ("lag", "diff", 2): TC._lag_ref(f64, valid, first, "diff", 2)}
    for op in ("forward", "backward"):
        exp["fill", op] = TF._ref(f64, valid, op, 3, starts)
    return valid, starts, i64, f64, exp


def _start_column(starts, soff):
    """The Boolean start column sliced at bit `soff`, or ("borrowed") at bit 2
    of a bitmap that begins 3 bytes into its allocation."""
    if soff != "borrowed":
        seg = _place("seg", starts, None, "slice", soff)
        assert seg._keep[0].to_numpy()[soff + starts.size:].all()
        return seg
    pv, _ = _parent(starts, None, 2)
    assert pv[2 + starts.size:].all()
    buf = _upload_bytes(np.packbits(pv, bitorder="little"), 3)
    return pl.Series.from_device("seg", pl.Boolean, buf.ptr + 3, starts.size, offset=2, keepalive=[buf])


@pytest.mark.parametrize("soff", [64, 8, 3, "borrowed"])
def test_scans_segmented_start_column(gpu, soff):
    """plgpu_cumulative, plgpu_lag, plgpu_fill and plgpu_ewm_mean with the
    Boolean start column of test_rolling_segmented_start_column: offset 64
    (used in place by the two that read whole words), 8 (a whole byte but no
    aligned word), 3, and a borrowed bitmap at an odd byte address; the
    parent's bits are set in the junk after the slice."""
    valid, starts, i64, f64, exp = _scan_host()
    seg = _start_column(starts, soff)
    xi, xf = _place("x", i64, valid, "slice", 66), _place("x", f64, valid, "slice", 66)
    TC._assert_same(*TC._cum(xi, "sum", seg), *exp["cum", "sum"], (soff, "cum_sum"))
    TC._assert_same(*TC._cum(xf, "max", seg), *exp["cum", "max"], (soff, "cum_max"), bits=True)
    for op, k in (("shift", 1), ("diff", 2)):
        (gv, gok), (ev, eok) = TC._lag(xf, op, k, seg), exp["lag", op, k]
        assert np.array_equal(gok, eok), (soff, op, "validity")
        assert gv[eok].tobytes() == ev[eok].tobytes(), (soff, op)
    for op in ("forward", "backward"):
        TF._same(TF._fill(xf, op, 3, seg), exp["fill", op], (soff, op))
    for adjust in (True, False):
        TE._check(TE._ewm(xf, 0.3, adjust, False, seg=seg), f64, valid, 0.3, adjust, False, (soff, "ewm", adjust),
                  starts=starts)


# --------------------------------------------------- B. eval and filter
@functools.lru_cache(maxsize=None)
def _eval_host():
    rng = np.random.default_rng(55)
    n = 20_000
    ok = lambda: rng.random(n) > 0.1  # noqa: E731
    words = np.array(["alpha", "alphabet", "beta", "", "gamma-alpha", "be", "délta", "a" * 20], dtype=object)
    return {"b": (rng.uniform(0.5, 2.0, n), ok()), "d": (rng.uniform(-5, 5, n), ok()),
            "q": (rng.integers(-10**12, 10**12, n).astype(np.int64), ok()),
            "a": (rng.integers(-50, 50, n).astype(np.int64), ok()),
            "e": (rng.integers(-50, 50, n).astype(np.int64), ok()),
            "c": (rng.random(n) < 0.5, ok()), "s": (words[rng.integers(0, 8, n)], ok())}


def _eval_exprs():
    return [PREDS["program"](),
            pl.when(col("c")).then(col("a")).otherwise(col("e")),
            pl.when(col("a") > col("e")).then(col("a") - col("e")).otherwise(0),
            pl.when(col("c")).then(col("a")).when(col("a") > 3).then(lit(7)).otherwise(None),
            col("a").fill_null(col("e")), col("a").fill_null(3), col("a").is_in([1, 2, 3, 40]),
            col("a").is_in([5, None], nulls_equal=True), col("a").is_between(-3, 10),
            col("a").is_between(col("e"), 20, closed="none"), col("c") ^ (col("a") > 0)]


def _eval_layouts():
    """B_LAYOUTS plus the Boolean column at offsets 1, 7, 63, 64 beside
    operands at two other offsets."""
    return list(B_LAYOUTS) + [f"bool{o}" for o in (1, 7, 63, 64)]


def _eval_frame(layout):
    host = _eval_host()
    if not layout.startswith("bool"):
        return _layout(host, layout)
    boff = int(layout[4:])
    series = []
    for j, (nm, (v, valid)) in enumerate(host.items()):
        series.append(_place(nm, v, valid, "slice", boff if nm == "c" else (2, 65)[j % 2]))
    return pl.DataFrame(series)


@pytest.mark.parametrize("layout", _eval_layouts())
def test_eval_and_filter_sliced(gpu, layout):
    """plgpu_eval / plgpu_filter_expr with operands at different offsets, and
    String predicates on a sliced String column: the oracle's interpreter."""
    from test_gpu_dtypes import check_eval

    host = _eval_host()
    n = 20_000
    df = _eval_frame(layout)
    names = [nm for nm in host if nm != "s"]
    hosts = [O.HostCol(*host[nm]) for nm in names]
    num = pl.DataFrame([df[nm] for nm in names])
    for e in _eval_exprs():
        check_eval(num, hosts, names, e, n)
    pred = PREDS["program"]()
    prog = lower(pred, {nm: i for i, nm in enumerate(names)}, {nm: num[nm].dtype.code for nm in names})
    out = num.filter(pred)
    _, keep, keep_ok = O.eval_program(hosts, prog, n)
    keep &= keep_ok
    for i, nm in enumerate(names):
        if nm == "c":  # (the oracle's filter moves fixed-width columns: the Boolean one by its mask)
            vals, valid = host[nm][0][keep], host[nm][1][keep]
            assert np.array_equal(out[nm].validity_numpy(), valid), (layout, nm)
            assert np.array_equal(out[nm].to_numpy()[valid], vals[valid]), (layout, nm)
            continue
        vals, valid = O.filter_column(hosts, prog, n, i)
        assert np.array_equal(out[nm].validity_numpy(), valid), (layout, nm)
        assert np.array_equal(out[nm].to_numpy()[valid].view(np.uint8), vals[valid].view(np.uint8)), (layout, nm)
    # String predicates: python's str semantics on the UTF-8 bytes
    sv, sok = host["s"]
    enc = [x.encode() for x in sv]
    for name, e, f in (("starts_with", col("s").str.starts_with("alpha"), lambda b: b.startswith(b"alpha")),
                       ("ends_with", col("s").str.ends_with("alpha"), lambda b: b.endswith(b"alpha")),
                       ("contains", col("s").str.contains("ta", literal=True), lambda b: b"ta" in b),
                       ("eq", col("s") == "beta", lambda b: b == b"beta")):
        got = df.select(e.alias("o"))["o"]
        want = np.array([f(b) for b in enc])
        assert np.array_equal(got.validity_numpy(), sok), (layout, name)
        assert np.array_equal(got.to_numpy()[sok], want[sok]), (layout, name)
        kept = df.filter(e)
        m = want & sok
        assert kept.height == int(m.sum()), (layout, name)
        assert kept["s"].to_list() == sv[m].tolist(), (layout, name)
        assert np.array_equal(kept["q"].validity_numpy(), host["q"][1][m]), (layout, name)


# -------------------------------------------------------------- B. join
JOIN_NL, JOIN_NR = 20_000, 3_000
JOIN_RIGHT = {"fresh": "fresh", "off1": "off64", "off2": "off63", "off63": "off2", "off64": "off65", "off65": "off1",
              "mixed": "mixed"}
JOIN_KEYS = (("k64",), ("k32",), ("k64", "k32"))
JOIN_FORMS = [("inner", o) for o in ("none", "left", "right", "left_right", "right_left")] + [
    ("left", "left_right"), ("right", "right_left"), ("full", "left_right"), ("full", "none"), ("semi", "left"),
    ("anti", "left")]


@functools.lru_cache(maxsize=None)
def _join_host():
    rng = np.random.default_rng(71)
    words = np.array(["", "x", "yy", "payload-string", "ß", "0123456789abcdef"], dtype=object)

    def side(n, pre):
        kidx = rng.integers(0, 2500, n)
        k64 = kidx.astype(np.int64) * 1_000_003 - 7
        k64[rng.random(n) < 0.01] = np.iinfo(np.int64).min
        k32 = (kidx % 1500).astype(np.int32)
        k32[rng.random(n) < 0.1] = -1
        pay = {pre + "f": (rng.standard_normal(n), rng.random(n) > 0.2),
               pre + "i": (np.arange(n, dtype=np.int64), None),
               pre + "s": (words[rng.integers(0, 6, n)], rng.random(n) > 0.1),
               pre + "b": (rng.random(n) > 0.5, rng.random(n) > 0.1),
               pre + "w": (rng.integers(-2**31, 2**31 - 1, n).astype(np.int32), None)}
        keys = {"k64": (k64, rng.random(n) > 0.05), "k32": (k32, rng.random(n) > 0.05)}
        # (the right side lists its payloads first: in `mixed` its keys sit at other offsets than the left's)
        return {**keys, **pay} if pre == "l" else {**pay, **keys}

    return side(JOIN_NL, "l"), side(JOIN_NR, "r")


_JOIN_ORACLE = {}


def _join_oracle(on, how, ne, order):
    ck = (on, how, ne, order)
    if ck not in _JOIN_ORACLE:
        lh, rh = _join_host()
        if len(on) == 1:
            _JOIN_ORACLE[ck] = O.join(O.HostCol(*lh[on[0]]), O.HostCol(*rh[on[0]]), how, ne, order)
        else:
            _JOIN_ORACLE[ck] = O.join_multi([lh[k] for k in on], [rh[k] for k in on], how, ne, order)
    return _JOIN_ORACLE[ck]


def _row_ids(s):
    return np.where(s.validity_numpy(), s.to_numpy().astype(np.int64), -1)


def _pairs_equal(gl, gr, ol, orr, unordered, tag):
    assert gl.shape == ol.shape, tag
    perm = np.arange(gl.size)
    if unordered:
        perm, b = np.lexsort((gr, gl)), np.lexsort((orr, ol))
        gl, gr, ol, orr = gl[perm], gr[perm], ol[b], orr[b]
    assert np.array_equal(gl, ol) and np.array_equal(gr, orr), tag
    return perm


@pytest.mark.parametrize("layout", B_LAYOUTS)
def test_join_sliced(gpu, layout):
    """Every join type and order over both sides sliced at different offsets:
    nullable Int64 / Int32 keys and the pair, nulls_equal both ways, Float64 /
    Int32 / Boolean / String payloads following their rows; the oracle's pairs
    (a multiset where the order is unspecified)."""
    lh, rh = _join_host()
    left, right = _layout(lh, layout), _layout(rh, JOIN_RIGHT[layout])
    for on in JOIN_KEYS:
        lks, rks = [left[k] for k in on], [right[k] for k in on]
        for ne in (False, True):
            for how, order in JOIN_FORMS:
                tag = (layout, on, ne, how, order)
                ol, orr = _join_oracle(on, how, ne, order)
                out = left.join(right, on=on[0] if len(on) == 1 else list(on), how=how, nulls_equal=ne,
                                maintain_order=order)
                gl = _row_ids(out["li"])
                if how in ("semi", "anti"):
                    assert np.array_equal(gl, ol), tag
                    for nm in ("lf", "ls", "lb", "lw"):
                        _take_check(out[nm], *lh[nm], gl, gl >= 0, tag + (nm,))
                    continue
                gr = _row_ids(out["ri"])
                _pairs_equal(gl, gr, ol, orr, order == "none" and how in ("inner", "full"), tag)
                if ne or order not in ("none", "left_right"):
                    continue  # the payloads of two forms per join type say enough
                for nm in ("lf", "ls", "lb", "lw"):
                    _take_check(out[nm], *lh[nm], np.maximum(gl, 0), gl >= 0, tag + (nm,))
                for nm in ("rf", "rs", "rb", "rw"):
                    _take_check(out[nm], *rh[nm], np.maximum(gr, 0), gr >= 0, tag + (nm,))
            # the index-only inner entry points
            ol, orr = _join_oracle(on, "inner", ne, "left_right")
            li, ri = N.Column(), N.Column()
            if len(on) == 1:
                N.check(N.lib().plgpu_join_inner(C.byref(lks[0]._col), C.byref(rks[0]._col), int(ne),
                                                 N.JOIN_ORDER["left_right"], 0, C.byref(li), C.byref(ri), None))
            else:
                N.check(N.lib().plgpu_join_inner_multi(_col_array(lks), _col_array(rks), len(on), int(ne),
                                                       N.JOIN_ORDER["left_right"], 0, C.byref(li), C.byref(ri), None))
            gl, gr = _row_ids(pl.Series._from_native("l", li)), _row_ids(pl.Series._from_native("r", ri))
            _pairs_equal(gl, gr, ol, orr, False, (layout, on, ne, "plgpu_join_inner"))


@pytest.mark.parametrize("mode", ["pairs", "rowformat", "radix"])
@pytest.mark.parametrize("layout", B_LAYOUTS)
def test_join_take_paths_sliced(gpu, plgpu_option, layout, mode):
    """The fused join + take (plgpu_join_inner_take) over a unique-keyed right
    side with one payload: the pairs + gather route at 20,000 rows, the
    row-format table (taken from 2^16 left rows on: 2^16 + 3 here), and the
    radix path forced as test_radix_join_forced_vs_oracle forces it.  The
    kernel timer says which ran."""
    from test_gpu_join_radix import _check as radix_check
    from test_gpu_join_radix import _join as timed_join
    from test_gpu_join_radix import _unique_keys

    radix = mode == "radix"
    nl, nr = (2**16 + 3 if mode == "rowformat" else JOIN_NL), JOIN_NR
    rng = np.random.default_rng(nl + nr)
    rk = _unique_keys(rng, nr, 4 * nr)
    rk[0] = np.iinfo(np.int64).max
    lk = rk[rng.integers(0, nr, nl)].copy()
    miss = rng.random(nl) < 0.5
    lk[miss] = rng.integers(0, 1 << 40, int(miss.sum())) * 2 + 1  # odd: never a build key
    lk[3] = np.iinfo(np.int64).min
    pay = np.arange(nr, dtype=np.int64) * 5 - 7
    c0 = rng.standard_normal(nl)
    left = _layout({"k": (lk, None), "li": (np.arange(nl, dtype=np.int64), None), "c0": (c0, None)}, layout)
    right = _layout({"p": (pay, None), "k": (rk, None)}, JOIN_RIGHT[layout])
    right = pl.DataFrame([right["k"], right["p"]])
    if radix:
        plgpu_option("join_radix", 2)
        plgpu_option("join_radix_keys", 64)
    out, names = timed_join(left, right)
    assert ("rj_match_kernel" in names) == radix, (layout, names)
    assert ("jn_build_rowformat_kernel" in names) == (mode == "rowformat"), (layout, names)
    radix_check(out, lk, rk, 2, [c0], pay)
    if not radix:
        out = left.join(right, on="k", maintain_order="left")
        ol, orr = O.join_inner(O.HostCol(lk), O.HostCol(rk))
        assert np.array_equal(out["li"].to_numpy(), ol) and np.array_equal(out["p"].to_numpy(), pay[orr])
        assert np.array_equal(_bits(out["c0"].to_numpy()), _bits(c0[ol]))


# ------------------------------------------------------- B. row shuffle
@functools.lru_cache(maxsize=None)
def _shuffle_host():
    rng = np.random.default_rng(81)
    n = 30_000
    words = np.array([f"sym{j:03d}" + "q" * (j % 9) for j in range(200)] + [""], dtype=object)
    return {"i64n": (rng.integers(0, 1000, n).astype(np.int64) * 1_000_000_007, rng.random(n) > 0.1),
            "pay": (rng.standard_normal(n), rng.random(n) > 0.3),
            "s": (words[rng.integers(0, 201, n)], rng.random(n) > 0.05),
            "f64": (np.array([0.0, -0.0, np.nan, -np.nan, 1.5, -2.25, np.inf])[rng.integers(0, 7, n)], None),
            "i32": (rng.integers(-3, 3, n).astype(np.int32), rng.random(n) > 0.05),
            "flag": (rng.random(n) < 0.5, rng.random(n) > 0.2)}


def _tuple_ids(host, keys):
    """Dense ids of the TotalEq classes of the key tuples (-0.0 with 0.0,
    every NaN together), and the rows whose tuple holds a null."""
    n = host[keys[0]][0].shape[0]
    words, anynull = [], np.zeros(n, bool)
    for k in keys:
        v, m = host[k]
        valid = np.ones(n, bool) if m is None else m
        anynull |= ~valid
        words.append(O._row_words(_str_codes(v) if v.dtype == object else v, valid))
    ids = np.unique(np.concatenate(words, axis=1), axis=0, return_inverse=True)[1].reshape(-1)
    return ids, anynull


_SHUFFLE_FRESH = {}


@pytest.mark.parametrize("keys", [("i64n",), ("s",), ("f64", "i32")], ids=["i64n", "str", "f64_i32"])
@pytest.mark.parametrize("layout", B_LAYOUTS)
def test_row_shuffle_sliced(gpu, layout, keys):
    """plgpu_hash_partition over sliced keys into 3 partitions, then
    plgpu_gather_rows / plgpu_pack_bits round the rows through the wire form."""
    from polaroid_amd import distributed as D

    host = _shuffle_host()
    n = 30_000
    df = _layout(host, layout)
    ids, anynull = _tuple_ids(host, keys)
    for ne in (False, True):
        tag = (layout, keys, ne)
        perm, counts = D.GpuJoinOps.partition(df, list(keys), 3, ne)
        p = perm.to_numpy().astype(np.int64)
        live = np.flatnonzero(~anynull) if not ne else np.arange(n)
        assert len(counts) == 3 and sum(counts) == p.shape[0] == live.shape[0], tag
        assert np.array_equal(np.sort(p), live), (tag, "not a permutation of the routed rows")
        part = np.full(n, -1)
        bounds = np.concatenate([[0], np.cumsum(counts)])
        for r in range(3):
            seg = p[bounds[r]:bounds[r + 1]]
            assert np.all(np.diff(seg) > 0), (tag, r, "rows of a partition must ascend")
            part[seg] = r
        if ne:
            assert np.all(part[anynull] == 0), (tag, "null keys go to partition 0")
        # equal keys share a partition
        order = np.argsort(ids[live], kind="stable")
        si, sp = ids[live][order], part[live][order]
        same = si[1:] == si[:-1]
        assert np.array_equal(sp[1:][same], sp[:-1][same]), (tag, "equal keys in different partitions")
        fk = (keys, ne)
        if fk not in _SHUFFLE_FRESH:
            fperm, fcounts = D.GpuJoinOps.partition(_layout(host, "fresh"), list(keys), 3, ne)
            _SHUFFLE_FRESH[fk] = (fperm.to_numpy().astype(np.int64), fcounts)
        assert counts == _SHUFFLE_FRESH[fk][1] and np.array_equal(p, _SHUFFLE_FRESH[fk][0]), (tag, "differs from fresh")
        back = D.GpuJoinOps.from_wire(D.GpuJoinOps.to_wire(df, perm), p.shape[0])
        for nm, (v, m) in host.items():
            _take_check(back[nm], v, m, p, np.ones(p.shape[0], bool), tag + (nm,))
    back = D.GpuJoinOps.from_wire(D.GpuJoinOps.to_wire(df), n)
    for nm, (v, m) in host.items():
        _take_check(back[nm], v, m, np.arange(n), np.ones(n, bool), (layout, nm, "no perm"))
