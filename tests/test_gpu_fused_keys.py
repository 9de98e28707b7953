"""Fused key packing and Categorical keys (round 4).

* Several integer keys (and one Int32 / UInt32 key) of a large input are
  packed into the exact Int64 tuple code (mk_plan_pack's layout) inside the
  fused group-by kernel's registers: no code column is written or read
  (info["key_pack"] = the number of key columns packed in the kernel).
  Checked bit-exact against the oracle's row-encoding restatement
  (oracle.group_by_agg_multi, polars-core/src/chunked_array/ops/
  row_encode.rs), against the code-column path (option fuse_keys = 0) on the
  same data, through the sampled plan's repack (an outlier row) and through
  the fallbacks (many groups, derived inputs).
* A Categorical column (an Arrow dictionary array: polars' export) groups
  by its UInt32 codes (polars-core/src/frame/group_by/into_groups.rs:132-139
  groups a Categorical by its physical codes); the strings are gathered only
  for the output keys (info["categorical_codes"]).  Pinned by the fixtures of
  tests/golden/categorical_cases.json (test_group_by.py:903-957 with nulls
  and maintain_order, test_categorical.py:104-118 two chunks, an empty key).
"""

import math

import numpy as np
import pyarrow as pa
import pytest

import polaroid_amd as pl
from polaroid_amd._native import fused_variant
from conftest import load_golden
from oracle import oracle as O
from test_gpu_groupby_multi import _check
from test_gpu_parity import _rand_frame

pytestmark = pytest.mark.gpu

N = 1_500_003  # above the sampled-plan / fused-packing threshold (2^20 rows)


def _dense(rng, n):
    """_rand_frame's columns without validity (the fused kernel's inputs are
    null-free; NaN / inf / -0.0 stay)."""
    return {k: (v, None) for k, (v, _) in _rand_frame(rng, n).items()}


@pytest.mark.parametrize("layout", ["day_ordered", "random"])
@pytest.mark.parametrize("aggs", ["sums", "mixed"])
@pytest.mark.parametrize("pred", [None, "simple_f64"])
def test_fused_two_keys_vs_oracle(gpu, layout, aggs, pred):
    """(symbol: Int64, day: Int32) packed in the fused kernel, exact vs the
    oracle: time-ordered days (range-local table) and random tuples."""
    rng = np.random.default_rng(len(layout) + 3 * len(aggs) + (pred is None))
    # day-ordered: 25,000 groups, ~100 per row range (the range-local table,
    # which needs >= 2^22 rows); random: 120 groups (one LDS table: the
    # mixed aggregations' table layout holds 256 slots at load 1/2)
    n = 4_500_001 if layout == "day_ordered" else N
    nsym = 100 if layout == "day_ordered" else 30
    sym = (rng.integers(0, nsym, n) * 7919 + 1_000_000).astype(np.int64)
    day = ((np.arange(n) * 250) // n).astype(np.int32) if layout == "day_ordered" else \
        rng.integers(0, 4, n).astype(np.int32)
    cols = _dense(rng, n)
    ag = [("sum", "a"), ("sum", "d")] if aggs == "sums" else \
        [("sum", "a"), ("min", "d"), ("max", "b"), ("count", "d"), ("len", "a"), ("mean", "d")]
    info = {}
    _check({"sym": (sym, None), "day": (day, None)}, cols, ag, False, pred, info=info)
    assert info["key_pack"] == 2, info


@pytest.mark.parametrize("dtype", [np.int32, np.uint32])
@pytest.mark.parametrize("maintain_order", [False, True])
def test_fused_single_narrow_key(gpu, dtype, maintain_order):
    """One null-free Int32 / UInt32 key (dates, Categorical codes): the fused
    kernel reads the 4-byte key and packs it (was: the generic kernel)."""
    rng = np.random.default_rng(int(maintain_order) + (dtype == np.uint32) * 2)
    lo = 0 if dtype == np.uint32 else -(1 << 30)
    k = (rng.integers(0, 300, N) * 1_000_003 % (1 << 30) + lo).astype(dtype)
    # the type's extremes and -1 (all-ones in 32 bits) as keys too
    info_ = np.iinfo(dtype)
    k[rng.integers(0, N, 50)] = info_.min
    k[rng.integers(0, N, 50)] = info_.max
    if dtype == np.int32:
        k[rng.integers(0, N, 50)] = -1
    cols = _dense(rng, N)
    info = {}
    _check({"k": (k, None)}, cols, [("sum", "a"), ("len", "b"), ("max", "d")], maintain_order, info=info)
    assert info["key_pack"] == 1, info


def test_fused_matches_code_column_path(gpu, plgpu_option):
    """fuse_keys = 0 (the packed code column) gives the same frame."""
    rng = np.random.default_rng(5)
    sym = rng.integers(0, 100, N).astype(np.int64)
    day = rng.integers(0, 5, N).astype(np.int32)  # 500 groups: one LDS table
    a = rng.uniform(10, 500, N)
    df = pl.DataFrame({"sym": pl.Series.from_numpy("sym", sym), "day": pl.Series.from_numpy("day", day),
                       "a": pl.Series.from_numpy("a", a)})
    q = df.lazy().filter(pl.col("a") > 250.0).group_by("sym", "day", maintain_order=True).agg(
        pl.col("a").sum(), pl.len())
    i1, i0 = {}, {}
    fused = q.collect(info=i1)
    plgpu_option("fuse_keys", 0)
    plain = q.collect(info=i0)
    assert i1["key_pack"] == 2 and i0["key_pack"] == 0
    for c in ("sym", "day", "len"):
        assert fused[c].to_list() == plain[c].to_list()
    assert np.array_equal(fused["a"].to_numpy().view(np.uint64), plain["a"].to_numpy().view(np.uint64))


@pytest.mark.parametrize("outlier", ["i64_high", "i32_low", "i32_high", "i32_negative_base"])
def test_fused_outlier_repacks(gpu, outlier):
    """A row outside the sampled packing plan (far from every sampled key)
    is caught in the fused kernel (ST_KPACK): the group-by repacks with the
    exact ranges and runs fused again, exact.  The Int32 cases take the
    32-bit field test (KeyPack mode 1), below and above the sampled range."""
    rng = np.random.default_rng(9)
    k1 = (rng.integers(0, 40, N) * 3 - 500).astype(np.int64)
    k2 = rng.integers(0, 10, N).astype(np.int32)  # ~400 groups: one LDS table
    if outlier == "i32_negative_base":
        k2 = (k2 - 1_000_000).astype(np.int32)
    r = N // 2 + 7
    if outlier == "i64_high":
        k1[r] = 1 << 40
    elif outlier == "i32_low":
        k2[r] = np.iinfo(np.int32).min + 3
    elif outlier == "i32_high":
        k2[r] = np.iinfo(np.int32).max
    else:
        k2[r] = 2_000_000_000
    cols = _dense(rng, N)
    info = {}
    _check({"k1": (k1, None), "k2": (k2, None)}, cols, [("sum", "a"), ("len", "b")], False, info=info)
    assert info["key_pack"] == 2, info


def test_fused_fallbacks(gpu):
    """Off the fused kernel the code column is used, with the same result:
    many groups (the partitioned / global path) and derived inputs."""
    rng = np.random.default_rng(11)
    n = 2_000_000
    k1 = rng.integers(0, 1000, n).astype(np.int64)
    k2 = rng.integers(0, 1000, n).astype(np.int32)
    cols = {"a": (rng.standard_normal(n), None), "b": (rng.integers(-9, 9, n).astype(np.int64), None)}
    info = {}
    _check({"k1": (k1, None), "k2": (k2, None)}, cols, [("sum", "a"), ("len", "a")], False, info=info)
    assert info["key_pack"] == 0 and info["groups"] > 600_000
    # (a * b).sum(): a derived input fused in registers is not a PACK variant
    df = pl.DataFrame({"k1": pl.Series.from_numpy("k1", k1 % 10), "k2": pl.Series.from_numpy("k2", k2 % 10),
                       "a": pl.Series.from_numpy("a", cols["a"][0]),
                       "b": pl.Series.from_numpy("b", cols["a"][0] * 2.0)})
    info = {}
    out = df.lazy().group_by("k1", "k2").agg((pl.col("a") * pl.col("b")).sum().alias("ab")).collect(info=info)
    assert info["key_pack"] == 0
    got = dict(zip(zip(out["k1"].to_list(), out["k2"].to_list()), out["ab"].to_list()))
    a, b = cols["a"][0], cols["a"][0] * 2.0
    for key in list(got)[:10]:
        m = ((k1 % 10) == key[0]) & ((k2 % 10) == key[1])
        assert got[key] == math.fsum(a[m] * b[m])


def _cat_frame(strings, vals=None, chunks=None):
    """A frame with a Categorical column "c" built as polars exports it: an
    Arrow dictionary array (one chunk, or several with their own dictionaries)."""
    if chunks is None:
        chunks = [strings]
    arrs = [pa.array(ch, pa.string()).dictionary_encode() for ch in chunks]
    s = pl.Series.from_arrow("c", pa.chunked_array(arrs) if len(arrs) > 1 else arrs[0])
    cols = [s]
    if vals is not None:
        cols.append(pl.Series.from_numpy("v", np.asarray(vals)))
    return pl.DataFrame(cols)


def test_categorical_golden(gpu):
    for case in load_golden("categorical_cases.json")["cases"]:
        if "chunks" in case:
            df = _cat_frame(None, case["vals"], case["chunks"])
        else:
            df = _cat_frame(case["key"], np.arange(len(case["key"]), dtype=np.int64))
        info = {}
        out = df.lazy().group_by("c", maintain_order=case["maintain_order"]).agg(pl.len()).collect(info=info)
        got = list(zip(out["c"].to_list(), out["len"].to_list()))
        want = list(zip(case["groups"], case["len"]))
        if not case["maintain_order"]:
            got, want = sorted(got, key=str), sorted(want, key=str)
        assert got == want, case["name"]
        if len(case["groups"]):
            assert info.get("categorical_codes") == 1, (case["name"], info)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("maintain_order", [False, True])
def test_categorical_headline_vs_strings(gpu, nulls, maintain_order):
    """The headline query (four sums under close > 250, the predicate's
    column last, and len) on a Categorical symbol: grouped by the codes,
    bit-equal to the oracle's group-by on the same UInt32 codes and identical
    to the same query on the String column.  Null-free, the fused kernel
    packs the 4-byte key (PACK 1) and, on the sum-only layout, runs the
    unsigned-limb variant (VAR 5); maintain_order adds the first-row field,
    so the mixed layout runs and VAR 5 (sum-only) cannot."""
    rng = np.random.default_rng(int(nulls) * 2 + maintain_order)
    syms = np.array([f"SYM{i:03d}" for i in range(100)], dtype=object)
    k = rng.integers(0, 100, N)
    strs = syms[k].tolist()
    if nulls:
        for i in rng.integers(0, N, 1000):
            strs[i] = None
    names = ["open", "high", "low", "close"]
    vals = {c: rng.uniform(10, 490, N) for c in names}
    vser = [pl.Series.from_numpy(c, v) for c, v in vals.items()]
    arr = pa.array(strs, pa.string()).dictionary_encode()
    df = pl.DataFrame([pl.Series.from_arrow("c", arr)] + vser)
    info = {}

    def query(frame):
        return frame.lazy().filter(pl.col("close") > 250.0).group_by("c", maintain_order=maintain_order).agg(
            *[pl.col(c).sum() for c in names], pl.len())

    out = query(df).collect(info=info)
    fv = fused_variant(info)
    assert info["categorical_codes"] == 1
    assert info["key_pack"] == (0 if nulls else 1), info
    if not nulls:
        assert fv["pack"] == 1 and fv["nacc"] == 4 and fv["pred"] == 1, (info, fv)
        if maintain_order:
            assert not fv["sumonly"] and fv["var"] == 0, (info, fv)
        else:
            assert info["path"] == 2 and fv["var"] == 5 and fv["limbs"] == 2, (info, fv)
    # the oracle on the codes (a null code: the null group)
    kvalid = ~np.asarray(arr.indices.is_null())
    codes = np.asarray(arr.indices.fill_null(0)).astype(np.uint32)
    pool = arr.dictionary.to_pylist()
    hc = [O.HostCol(vals[c]) for c in ["close", "open", "high", "low"]]
    okeys, oouts = O.group_by_agg_multi([(codes, kvalid if nulls else None)], hc,
                                        [(1, 0, 0), (2, 0, 250.0), (24, 0, 0)],
                                        [("sum", 1), ("sum", 2), ("sum", 3), ("sum", 0), ("len", 0)], N)
    (ok, okv), = okeys
    okl = [pool[int(c)] if v else None for c, v in zip(ok, okv)]
    want = {key: ([o[0][i] for o in oouts[:4]], int(oouts[4][0][i])) for i, key in enumerate(okl)}
    gkeys = out["c"].to_list()
    assert len(gkeys) == len(want) and set(gkeys) == set(want)
    vc = [out[c].to_numpy() for c in names]
    lens = out["len"].to_list()
    for i, key in enumerate(gkeys):
        got = np.array([v[i] for v in vc])
        assert np.array_equal(got.view(np.int64), np.array(want[key][0]).view(np.int64)), key
        assert lens[i] == want[key][1], key
    if maintain_order:
        assert gkeys == okl  # first-occurrence order of the selected rows
    sdf = pl.DataFrame([pl.Series("c", strs, pl.String)] + vser)
    ref = query(sdf).collect()
    cols_ = ["c"] + names + ["len"]
    a = sorted(zip(*[out[c].to_list() for c in cols_]), key=str)
    b = sorted(zip(*[ref[c].to_list() for c in cols_]), key=str)
    assert a == b
    if maintain_order:
        assert out["c"].to_list() == ref["c"].to_list()
    # the output keys stay codes over the dictionary until exported
    oarr = out["c"].to_arrow()
    assert pa.types.is_dictionary(oarr.type) and oarr.to_pylist() == out["c"].to_list()


def test_categorical_key_also_used_elsewhere(gpu):
    """A Categorical key that the predicate or an aggregation also reads
    keeps its strings for those (and still groups correctly)."""
    rng = np.random.default_rng(2)
    n = 200_000
    strs = np.array(["AAPL", "MSFT", "GOOG", "AMZN"], dtype=object)[rng.integers(0, 4, n)].tolist()
    v = rng.uniform(0, 1, n)
    df = _cat_frame(strs, v)
    out = df.lazy().filter(pl.col("c") != "MSFT").group_by("c").agg(pl.col("v").sum().alias("s")).collect()
    got = dict(zip(out["c"].to_list(), out["s"].to_list()))
    sa = np.array(strs, dtype=object)
    assert set(got) == {"AAPL", "GOOG", "AMZN"}
    for key, val in got.items():
        assert val == math.fsum(v[sa == key])
    # the column's strings are gathered for other uses (a filter of the frame)
    f = df.filter(pl.col("c") == "GOOG")
    assert f["c"].to_list() == [s for s in strs if s == "GOOG"]


def _string_frame(keys_list, vals):
    return pl.DataFrame([pl.Series("s", keys_list, pl.String), pl.Series.from_numpy("v", vals)])


@pytest.mark.parametrize("case", ["short", "long_selected", "long_unselected", "empty_strings"])
def test_fused_string_key(gpu, case):
    """One null-free String key of a large input: its exact short-string
    codes are formed inside the fused kernel from the offsets and data words
    (no code column); a selected string longer than 7 bytes sends the
    query to the hashed long-string path (key_pack 0), one in an unselected
    row does not.  Same groups and exact sums as Python on the strings."""
    rng = np.random.default_rng(len(case))
    n = 1_200_001
    pool = np.array([f"S{i}" for i in range(150)] + ["", "abcdefg"], dtype=object)
    if case == "empty_strings":
        pool[:20] = ""
    idx = rng.integers(0, len(pool), n)
    strs = pool[idx].astype(object)
    v = rng.uniform(0, 100, n)
    if case == "long_selected":
        strs[n // 3] = "a-much-longer-symbol"
        v[n // 3] = 99.0
    if case == "long_unselected":
        strs[n // 3] = "a-much-longer-symbol"
        v[n // 3] = 1.0
    df = _string_frame(strs.tolist(), v)
    info = {}
    out = df.lazy().filter(pl.col("v") > 50.0).group_by("s").agg(pl.col("v").sum().alias("sv"), pl.len()).collect(
        info=info)
    assert info["key_pack"] == (0 if case == "long_selected" else 1), info
    sel = v > 50.0
    want = {}
    for sv, x in zip(strs[sel].tolist(), v[sel].tolist()):
        want.setdefault(sv, []).append(x)
    got = dict(zip(out["s"].to_list(), zip(out["sv"].to_list(), out["len"].to_list())))
    assert set(got) == set(want)
    for key, xs in want.items():
        assert got[key] == (math.fsum(xs), len(xs)), key



_NONNEG_PREDS = {  # name -> (expr, the oracle's program over column 0 = close)
    "gt0": (lambda: pl.col("close") > 0.0, [(1, 0, 0), (2, 0, 0.0), (24, 0, 0)]),
    "ge0": (lambda: pl.col("close") >= 0.0, [(1, 0, 0), (2, 0, 0.0), (25, 0, 0)]),
    "gt250": (lambda: pl.col("close") > 250.0, [(1, 0, 0), (2, 0, 250.0), (24, 0, 0)]),
    "eq0": (lambda: pl.col("close") == 0.0, [(1, 0, 0), (2, 0, 0.0), (20, 0, 0)]),
    "eq": (lambda: pl.col("close") == 3.5, [(1, 0, 0), (2, 0, 3.5), (20, 0, 0)]),
    "gtneg": (lambda: pl.col("close") > -1.0, [(1, 0, 0), (2, 0, -1.0), (24, 0, 0)]),
}


_NONNEG_N = {"int64": 400_003, "runs": 400_003, "int64_nulls": 400_003}  # the others: _PACKED_N
_PACKED_N = 2**20 + 515  # just over the fused packing threshold (2^20 rows), no multiple of any tile
_NONNEG_PACK = {"int64": 0, "runs": 0, "int64_nulls": 0, "sym_day": 1, "i32": 1, "cat": 1, "str": 2}
_NONNEG_KEY_PACK = {"int64": 0, "runs": 0, "int64_nulls": 0, "sym_day": 2, "i32": 1, "cat": 1, "str": 1}
_HOT = 0.65         # share of the rows in the hot group (see _nonneg_data)
_SUBNORMAL = 5e-324


def _nonneg_data(pname, keys, order):
    """Inputs of test_nonneg_predicate_column_sum: (n, key arrays for the
    oracle, key pool or None, value columns, validity, names)."""
    rng = np.random.default_rng(len(pname) + 7 * len(keys) + len(order))
    n = _NONNEG_N.get(keys, _PACKED_N)
    names = ["open", "high", "low", "close"] if order == "close_last" else ["close", "open", "high", "low"]
    # magnitudes in [1, 500) with either sign: nine binades, so that every
    # selected nonzero value fits the 2-limb window (19 binades below the
    # largest sampled exponent); values nearer zero would send the plan to
    # three limbs (correctly), where VAR 5 does not exist
    cols = {c: rng.uniform(1, 500, n) * rng.choice([-1.0, 1.0], n) for c in names}
    x = cols["close"]
    x[rng.random(n) < 0.05] = 0.0
    x[rng.random(n) < 0.05] = -0.0
    x[rng.random(n) < 0.02] = 3.5
    x[rng.integers(0, n, 30)] = np.nan
    x[rng.integers(0, n, 20)] = np.inf
    x[rng.integers(0, n, 20)] = -np.inf
    x[rng.integers(0, n, 200)] = np.nextafter(250.0, 0)
    x[rng.integers(0, n, 200)] = np.nextafter(250.0, 500)
    if pname in ("gt250", "eq0", "eq"):
        # the smallest subnormal, where the predicate rejects it (it is
        # neither == 0 nor > 250).  A selected one lies below every 2-limb
        # window, so the call reruns with three limbs:
        # test_nonneg_selected_subnormal_takes_three_limbs.  The rows avoid
        # the plan's samples (16-row clusters every n // 4096 rows): under
        # eq0 no selected nonzero close is sampled, the plan samples the
        # columns unfiltered, and a sampled subnormal chooses three limbs.
        r = rng.integers(0, n - 64, 40)
        x[np.where(r % (n // 4096) < 16, r + 16, r)] = _SUBNORMAL
    # one hot group, its close in [499, 500): the unsigned limbs of one slot
    # carry as often as this size allows.  65 % of the rows, not more: above
    # ~70 % most sampled rows equal their successor's key and the plan takes
    # the register-run kernel (RUNS) for every layout, which has no VAR 5.
    hot = rng.random(n) < _HOT
    x[hot] = rng.uniform(499.0, 500.0, int(hot.sum()))
    x[rng.choice(n, 2000, replace=False)] = 250.0
    sym = rng.integers(0, 100, n).astype(np.int64)
    sym[hot] = 37
    pool = None
    if keys == "runs":
        sym = np.sort(sym)
    if keys == "sym_day":
        day = ((np.arange(n) * 4) // n).astype(np.int32)  # 100 x 4 tuples: one 1,024-slot LDS table
        day[hot] = 2
        hk = [sym * 7919 + 1_000_000, day]
    elif keys == "i32":
        k = (sym * 1_000_003 - (1 << 30)).astype(np.int32)
        for v in (np.iinfo(np.int32).min, -1, np.iinfo(np.int32).max):
            k[rng.integers(0, n, 50)] = v
        hk = [k]
    elif keys in ("cat", "str"):
        # at most 7 bytes, "" included (the String key's exact short codes)
        pool = np.array([f"SYM{i:03d}" for i in range(98)] + ["", "abcdefg"], dtype=object)
        hk = [sym]
    else:
        hk = [sym]
    valid = {c: (rng.random(n) > 0.02 if keys == "int64_nulls" else None) for c in names}
    return n, hk, pool, cols, valid, names


def _nonneg_frame(keys, hk, pool, cols, valid):
    vals = [pl.Series.from_numpy(c, v, valid[c]) for c, v in cols.items()]
    if keys == "cat":
        return pl.DataFrame([_cat_frame(pool[hk[0]].tolist())["c"]] + vals), ["c"]
    if keys == "str":
        return pl.DataFrame([pl.Series("s", pool[hk[0]].tolist(), pl.String)] + vals), ["s"]
    by = ["sym", "day"][:len(hk)]
    return pl.DataFrame([pl.Series.from_numpy(nm, k) for nm, k in zip(by, hk)] + vals), by


@pytest.mark.parametrize("pname", list(_NONNEG_PREDS))
@pytest.mark.parametrize("keys", ["int64", "sym_day", "runs", "int64_nulls", "i32", "cat", "str"])
@pytest.mark.parametrize("order", ["close_last", "close_first"])
def test_nonneg_predicate_column_sum(gpu, plgpu_option, pname, keys, order):
    """Four sums whose last column is the fused predicate's and keeps no
    value below a literal >= 0 (the headline's close.sum() under
    close > 250) run the variant whose last limbs carry no sign
    (gb_fast_kernel VAR 5, option sum_pos).  Checked bit-exact against the
    oracle (or_group_by_agg, SUM_EXACT) with the option on and off, and the
    instantiation each call launched is read back (info["fused_variant"]):
    VAR 5 with the option on, the column last and a literal >= 0; the signed
    kernel otherwise (close_first: var_x_nonneg's pred_acc is then 0; gtneg:
    a negative literal; option off), so on / off never compare one kernel
    with itself.  Data: negatives, zeros, -0.0, NaN, +-inf, exact hits of
    the literals, the doubles next to 250.0 on both sides, the smallest
    subnormal, and a hot group of large values (_nonneg_data).
    Key layouts: an Int64 key; (Int64, Int32), one Int32 key with the type's
    extremes and -1, and a Categorical's UInt32 codes, all packed in the
    kernel (PACK 1: the benchmark's Categorical and (symbol, day) legs); a
    String key of at most 7 bytes (PACK 2); a sorted Int64 key, which takes
    the register-run kernel (launch_fast tests pl.runs first) and never VAR
    5; and an Int64 key over value columns with ~2 % nulls (the NULLS
    variant; a null close drops its row, so VAR 5 still holds)."""
    n, hk, pool, cols, valid, names = _nonneg_data(pname, keys, order)
    x = cols["close"]
    # (the later writes of _nonneg_data overwrite earlier ones: each special survives)
    assert np.isnan(x).any() and (x == np.inf).any() and (x == -np.inf).any() and (x < 0).any()
    assert (x == np.nextafter(250.0, 0)).any() and (x == np.nextafter(250.0, 500)).any()
    assert (x == 250.0).sum() >= 2000 and (x == 3.5).any() and (np.signbit(x) & (x == 0)).any()
    assert (x == _SUBNORMAL).any() == (pname in ("gt250", "eq0", "eq"))
    df, by = _nonneg_frame(keys, hk, pool, cols, valid)
    mk, prog = _NONNEG_PREDS[pname]
    onames = ["close"] + [c for c in names if c != "close"]
    hc = [O.HostCol(cols[c], valid[c]) for c in onames]
    oidx = {c: i for i, c in enumerate(onames)}
    okeys, oouts = O.group_by_agg_multi([(k, None) for k in hk], hc, prog, [("sum", oidx[c]) for c in names], n)
    unkey = (lambda v: pool[int(v)]) if pool is not None else int
    want = {tuple(unkey(k[0][i]) for k in okeys): [o[0][i] for o in oouts] for i in range(len(okeys[0][0]))}
    for on in (1, 0):
        plgpu_option("sum_pos", on)
        info = {}
        out = df.lazy().filter(mk()).group_by(*by).agg(*[pl.col(c).sum() for c in names]).collect(info=info)
        fv = fused_variant(info)
        tag = (pname, keys, order, on, info, fv)
        assert out.height == len(want), tag
        assert info["path"] == 2 and info["sum_limbs"] == 2, tag
        assert info["key_pack"] == _NONNEG_KEY_PACK[keys], tag
        assert info.get("categorical_codes", 0) == (1 if keys == "cat" else 0), tag
        assert fv["pack"] == _NONNEG_PACK[keys] and fv["nulls"] == (keys == "int64_nulls"), tag
        assert fv["nacc"] == 4 and fv["pred"] == 1 and fv["sumonly"] and fv["limbs"] == 2, tag
        if keys == "runs":
            assert fv["runs"] and fv["var"] == 0 and info["register_runs"] == 1, tag
        elif on == 1 and order == "close_last" and pname != "gtneg":
            assert fv["var"] == 5 and not fv["runs"], tag
        else:
            assert fv["var"] == 0 and not fv["runs"], tag
        kc = [out[k].to_list() for k in by]
        vc = [out[c].to_numpy() for c in names]
        for i in range(out.height):
            w = want[tuple(k[i] for k in kc)]
            got = np.array([v[i] for v in vc])
            assert np.array_equal(got.view(np.int64), np.array(w).view(np.int64)), (tag, i)


@pytest.mark.parametrize("pname", ["gt0", "ge0"])
def test_nonneg_selected_subnormal_takes_three_limbs(gpu, pname):
    """A selected subnormal (5e-324 passes > 0 and >= 0) has bits below every
    2-limb window: the 2-limb pass flags it and the call runs again on three
    limbs (info["reruns"]), where the unsigned variant does not exist
    (launch_fast: VAR 5 needs pl.limbs == 2).  Still bit-exact against the
    oracle."""
    rng = np.random.default_rng(len(pname))
    n = 400_003
    sym = rng.integers(0, 100, n).astype(np.int64)
    names = ["open", "high", "low", "close"]
    cols = {c: rng.uniform(1, 500, n) * rng.choice([-1.0, 1.0], n) for c in names}
    cols["close"][rng.random(n) < 0.05] = -0.0
    # (off the plan's sampled rows, 16-row clusters every n // 4096 rows: the
    # plan then chooses two limbs and the main pass has to catch the value)
    r = rng.integers(0, n - 64, 40)
    cols["close"][np.where(r % (n // 4096) < 16, r + 16, r)] = _SUBNORMAL
    df = pl.DataFrame([pl.Series.from_numpy("sym", sym)] + [pl.Series.from_numpy(c, v) for c, v in cols.items()])
    mk, prog = _NONNEG_PREDS[pname]
    hc = [O.HostCol(cols[c]) for c in ["close", "open", "high", "low"]]
    okeys, oouts = O.group_by_agg_multi([(sym, None)], hc, prog, [("sum", i) for i in (1, 2, 3, 0)], n)
    want = {int(okeys[0][0][i]): [o[0][i] for o in oouts] for i in range(len(okeys[0][0]))}
    info = {}
    out = df.lazy().filter(mk()).group_by("sym").agg(*[pl.col(c).sum() for c in names]).collect(info=info)
    fv = fused_variant(info)
    assert info["path"] == 2 and info["sum_limbs"] == 3 and info["reruns"] >= 1, (info, fv)
    assert fv["var"] == 0 and fv["limbs"] == 3 and fv["nacc"] == 4, (info, fv)
    assert out.height == len(want)
    vc = [out[c].to_numpy() for c in names]
    for i, k in enumerate(out["sym"].to_list()):
        got = np.array([v[i] for v in vc])
        assert np.array_equal(got.view(np.int64), np.array(want[k]).view(np.int64)), (pname, k)
