"""The fused group-by kernel with claimed rows (option gb_claim, the
default): a grid of the resident workgroups whose waves claim chunks of
128-row units from per-segment counters, against the static grid of several
rounds (gb_claim 0).

Every case runs both sides with plan_cache 0, compares each bit for bit with
the oracle (the sweep's helpers: _data, _oracle, _gpu, _compare, which allow
any group order without maintain_order) and asserts the kernel timer's name
of the side it names: "gb_fast_kernel" for claimed rows,
"gb_fast_static_kernel" for the static grid that gb_claim 0 puts in their
place, never both.

Shapes, on the headline's kernel (4 sums, the predicate on the last one's
column: VAR 5): 1,024 rows (one tile: 8 units, fewer than the 64 segments),
1,025 and 3,071 rows (the masked units after the last full tile, one nearly
empty and seven of which the last is nearly full), 200,003 rows (the suite's
size: 1,563 units, no multiple of the segments or the chunk, fewer tiles than
resident workgroups) and 8 * 1024 * R + 1027 rows for R resident workgroups
(4.2 M at R = 512: every resident workgroup's waves claim several chunks and
move on to other segments when theirs is used up).

Variants at 200,003 rows (2^20 + 515 for the packed keys): each family of
template arguments of gb_fast_kernel, as tests/test_gpu_fused_variants.py
names them.

The cap: claim_cap_rows 2048 at 2^21 rows; the grid is then the 1,024
workgroups the cap needs, every one of them stops at its cap, and no row may
be left behind.
"""

import numpy as np
import pytest

import polaroid_amd as pl
from polaroid_amd import _native as N
from polaroid_amd._native import fused_variant
from polaroid_amd.expr import col
from test_gpu_fused_variants import CASES, N_PACKED, _check_var, _frame, _StrKeyAsInt
from test_gpu_groupby_sweep import MIXED
from test_gpu_groupby_sweep import N as N_SWEEP
from test_gpu_groupby_sweep import _compare, _data, _gpu, _oracle

pytestmark = pytest.mark.gpu

CLAIMED, STATIC = "gb_fast_kernel", "gb_fast_static_kernel"


def _timed(fn):
    N.ktime_read()
    out = fn()
    return out, N.ktime_read()


def _sides(plgpu_option, run, tag):
    """run() under gb_claim 1 and 0; each side's timer name, and its info."""
    plgpu_option("plan_cache", 0)
    plgpu_option("ktime", 1)
    infos = {}
    for claim in (1, 0):
        plgpu_option("gb_claim", claim)
        info, kt = _timed(run)
        want, other = (CLAIMED, STATIC) if claim else (STATIC, CLAIMED)
        assert want in kt and other not in kt, (tag, claim, sorted(kt))
        infos[claim] = info
    return infos


S4 = [("sum", col(nm)) for nm in ("b", "e", "f", "c")]


def _headline_case(plgpu_option, df, cols, n, tag):
    """The 4-sum VAR 5 kernel over df, both sides exact; the two infos."""
    plgpu_option("gb_path", 2)
    pred = col("c") > 250.0
    exp = _oracle(cols, "k", S4, pred, n)

    def run():
        out, info = _gpu(df, "k", S4, pred, False)
        _compare(out, "k", exp, len(S4), False, (tag, info))
        fv = fused_variant(info)
        assert info["path"] == 2 and fv["ran"] and fv["var"] == 5 and fv["nacc"] == 4 and fv["limbs"] == 2, (tag, info)
        return info

    return _sides(plgpu_option, run, tag)


@pytest.mark.parametrize("n", [1024, 1024 + 1, 2048 + 1023, N_SWEEP])
def test_claimed_rows_small_shapes(gpu, plgpu_option, n):
    df, cols = _data(4000 + n, n=n)
    infos = _headline_case(plgpu_option, df, cols, n, n)
    # fewer tiles than resident workgroups: one workgroup per full tile at most
    assert infos[1]["grid"] <= max(1, n // 1024), infos


def _wide_frame(n):
    rng = np.random.default_rng(n)
    c = rng.uniform(10, 500, n)
    cols = {"k": ((rng.integers(0, 300, n) * 7919 - 5).astype(np.int64), None), "c": (c, None),
            "b": (rng.uniform(0.5, 2.0, n), None), "e": (c * rng.uniform(0.99, 1.01, n), None),
            "f": (rng.uniform(1, 1000, n), None), "d": (rng.uniform(-5, 5, n), None),
            "q": (rng.integers(-10**12, 10**12, n).astype(np.int64), None)}
    return pl.DataFrame([pl.Series.from_numpy(nm, v) for nm, (v, _) in cols.items()]), cols


def _resident(plgpu_option):
    """The resident workgroups of the 2-sum kernel, as test_fused_grid_rounds
    reads them: the grid of a 2^21-row run in one round."""
    plgpu_option("gb_path", 2)
    plgpu_option("plan_cache", 0)
    plgpu_option("grid_rounds", 1)
    df, _ = _wide_frame(1 << 21)
    _, info = _gpu(df, "k", [("sum", col("c")), ("sum", col("b"))], None, False)
    plgpu_option("grid_rounds", 0)
    assert info["path"] == 2 and 0 < info["grid"] < 2048, info
    return info["grid"]


def test_claimed_rows_every_workgroup_claims_and_steals(gpu, plgpu_option):
    """8 * 1024 * R + 1027 rows: 64 units and more per resident workgroup."""
    resident = _resident(plgpu_option)
    n = 8 * 1024 * resident + 1027
    df, cols = _wide_frame(n)
    infos = _headline_case(plgpu_option, df, cols, n, n)
    # claimed rows never launch more than the resident workgroups of their
    # kernel here (no cap in reach); the static side launches several rounds
    assert 0 < infos[1]["grid"] <= 2 * resident and infos[0]["grid"] >= infos[1]["grid"], (infos, resident)


def test_claim_cap_reached_leaves_no_row(gpu, plgpu_option):
    """claim_cap_rows 2048 at 2^21 rows: 2 units per wave, so 1,024
    workgroups (more than are resident), all of which stop at the cap."""
    resident = _resident(plgpu_option)
    n, cap = 1 << 21, 2048
    df, cols = _wide_frame(n)
    plgpu_option("gb_path", 2)
    plgpu_option("plan_cache", 0)
    plgpu_option("ktime", 1)
    plgpu_option("gb_claim", 1)
    plgpu_option("claim_cap_rows", cap)
    specs = [("sum", col("c")), ("sum", col("b"))]
    exp = _oracle(cols, "k", specs, None, n)
    (out, info), kt = _timed(lambda: _gpu(df, "k", specs, None, False))
    assert CLAIMED in kt and STATIC not in kt, sorted(kt)
    _compare(out, "k", exp, len(specs), False, info)
    need = (n + cap - 1) // cap
    assert info["path"] == 2 and info["grid"] == need and need > resident, (info, need, resident)


# one row of tests/test_gpu_fused_variants.py's CASES per family
FAMILIES = ["fast_var5", "fast_sumonly3", "nulls_var5_nacc4", "nulls_general_pred", "fast_sumonly2_pack1",
            "fast_sumonly2_pack2", "fast_mixed_pack1", "fast_runs_sumonly", "fast_runs_mixed2", "fast_deriv2",
            "var1_2limb", "var4", "pair2_2limb", "pair3_3limb"]


@pytest.mark.parametrize("cid", FAMILIES)
def test_claimed_rows_variant_families(gpu, plgpu_option, cid):
    """3 limbs, NULLS, PACK 1 / 2, RUNS, DERIV, the variance triple (VAR 1 /
    4) and the product pair (VAR 2 / 3), each exact on both sides and the
    variant its row names."""
    _, kind, key, build, pred, maintain, opts, expect = next(c for c in CASES if c[0] == cid)
    df, cols = _frame(kind)
    n = N_PACKED if kind == "packed" else N_SWEEP
    for name, value in opts.items():
        plgpu_option(name, value)
    plgpu_option("local", 0)  # (sorted keys: the range-local mode keeps its own launch shape)
    if not isinstance(build, tuple):
        specs = build()
        exp = _oracle(cols, "i" if key == "s" else key, specs, pred() if pred else None, n, names_extra=("w",))

    def run():
        if isinstance(build, tuple):
            info = _check_var(df, cols, key, build[1], build[2], pred, maintain, n)
        else:
            out, info = _gpu(df, key, specs, pred() if pred else None, maintain)
            okey = key
            if key == "s":
                out, okey = _StrKeyAsInt(out), "i"
            _compare(out, okey, exp, len(specs), maintain, (cid, info))
        fv = fused_variant(info)
        assert fv["ran"] and {name: fv[name] for name in expect} == expect, (cid, fv, info)
        return info

    _sides(plgpu_option, run, cid)


@pytest.mark.parametrize("key", ["k", "kn"])
def test_claimed_rows_general_layout_in_first_row_order(gpu, plgpu_option, key):
    """min / max / first / last / count next to a sum under maintain_order:
    first, last and the group order come from row numbers, so they may not
    depend on which wave took which rows."""
    df, cols = _data(4242)
    plgpu_option("gb_path", 2)
    specs = [(kind, col(c)) for kind, c in MIXED]
    pred = col("c") > 250.0
    exp = _oracle(cols, key, specs, pred, N_SWEEP, names_extra=("a", "f"))

    def run():
        out, info = _gpu(df, key, specs, pred, True)
        _compare(out, key, exp, len(specs), True, (key, info))
        assert info["path"] == 1 and fused_variant(info)["ran"], info
        return info

    _sides(plgpu_option, run, key)


def test_claimed_rows_nulls_without_whole_word_validity(gpu, plgpu_option):
    """NULLS over columns at logical offset 2: a lane reads the validity word
    of its own row pair (fused_variant vwords False); the aligned frame of
    test_claimed_rows_variant_families reads whole words per wave."""
    n = N_SWEEP
    _, cols = _data(777, n=n)
    series = []
    for nm, (v, m) in cols.items():
        pv = np.concatenate([v[:2], v])
        pm = None if m is None else np.concatenate([[True, False], m])
        series.append(pl.Series.from_numpy(nm, pv, pm).slice(2, n))
    df = pl.DataFrame(series)
    plgpu_option("gb_path", 2)
    plgpu_option("sum_pos", 1)
    specs = [("sum", col(nm)) for nm in ("b", "e", "f", "cn")]
    pred = col("cn") > 250.0
    exp = _oracle(cols, "kn", specs, pred, n, names_extra=("cn",))

    def run():
        out, info = _gpu(df, "kn", specs, pred, False)
        _compare(out, "kn", exp, len(specs), False, info)
        fv = fused_variant(info)
        assert fv["ran"] and fv["nulls"] and not fv["vwords"] and fv["var"] == 5, (fv, info)
        return info

    _sides(plgpu_option, run, "off2")


def test_claimed_rows_keyless(gpu, plgpu_option):
    """select(sums): one group, every wave adding into the same slot."""
    df, cols = _data(4243)
    plgpu_option("gb_path", 2)
    specs = [("sum", col("c")), ("mean", col("b"))]
    pred = col("c") > 250.0
    exp = _oracle(cols, None, specs, pred, N_SWEEP)

    def run():
        out, info = _gpu(df, None, specs, pred, False)
        _compare(out, None, exp, len(specs), False, info)
        assert fused_variant(info)["ran"], info
        return info

    _sides(plgpu_option, run, "keyless")
