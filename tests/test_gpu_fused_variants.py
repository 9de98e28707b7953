"""One oracle-exact case per branch of the fused group-by kernel's launchers,
each proving that its branch ran.

groupby_kernels.hpp / groupby.hip choose among dozens of instantiations of
gb_fast_kernel<NACC, PRED, SUMONLY, ROWS, LIMBS, RUNS, ..., DERIV, VAR, PACK,
NULLS> (launch_fast_dispatch -> launch_fast_nulls / launch_fast /
launch_fast_var / launch_fast_pair); info["path"] tells the fused kernel from
the others but not one instantiation from another, so a case could pass while
running a different variant from the one it names.  Every row of CASES below
names one `return launch_fast_rows<...>` line, compares the result bit for
bit with the oracle exactly as tests/test_gpu_groupby_sweep.py does (its
_data, _oracle, _gpu, _compare), and then asserts the template arguments the
call reports (info["fused_variant"], decoded by _native.fused_variant).

Sizes: 200,003 rows with the fused kernel forced (gb_path 2) for the key
column variants (PACK 0); 2^20 + 515 rows, just over the fused key packing's
threshold and no multiple of a tile, for the packed ones (PACK 1: one Int32
key; PACK 2: one short String key).

Columns (the sweep's, plus): the 2-limb layout needs every summed column's
sampled exponents within ~15 binades, so the 2-limb rows sum c, b, e, f
(uniform, at most 10 binades); the 3-limb rows add `w`, 40 binades wide
(beyond the 2-limb window's 28, inside the 3-limb window's 68, so no wide-sum
fallback); the variance rows take v2 (one binade pair: 2 limbs for x, x * x
and its error term) and v3 (1e-3 .. 1e3: 3 limbs), the spreads
tests/test_gpu_var_std.py::test_var_triple_kernel_windows pins.
"""

import functools
from fractions import Fraction

import numpy as np
import pytest

import polaroid_amd as pl
from polaroid_amd._native import fused_variant
from polaroid_amd.expr import col
from test_gpu_groupby_sweep import N, _bits, _compare, _data, _gpu, _oracle

pytestmark = pytest.mark.gpu

N_PACKED = 2**20 + 515
_POOL = np.array([f"T{j}" for j in range(99)] + [""], dtype=object)  # <= 7 bytes, "" included


@functools.lru_cache(maxsize=None)
def _frame(kind):
    """plain / sorted: the sweep's frame at N rows (random / sorted keys);
    packed: at N_PACKED rows.  Plus w, v2, v3 and the String key s."""
    n = N_PACKED if kind == "packed" else N
    _, cols = _data({"plain": 311, "sorted": 312, "packed": 313}[kind], n=n, sorted_keys=kind == "sorted")
    rng = np.random.default_rng(n + len(kind))
    cols["w"] = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-20, 20, n) * rng.choice([-1.0, 1.0], n), None)
    cols["v2"] = (250 + rng.random(n) * 250, None)
    cols["v3"] = (np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n)) * rng.choice([-1.0, 1.0], n), None)
    series = [pl.Series.from_numpy(nm, v, m) for nm, (v, m) in cols.items()]
    series.append(pl.Series("s", _POOL[cols["i"][0] + 50].tolist(), pl.String))
    return pl.DataFrame(series), cols


class _StrKeyAsInt:
    """out["s"] as the Int32 key the strings were made from, for _compare."""

    def __init__(self, out):
        self._out = out
        back = {s: j - 50 for j, s in enumerate(_POOL.tolist())}
        self._k = np.array([back[s] for s in out["s"].to_list()], dtype=np.int64)

    height = property(lambda self: self._out.height)

    def __getitem__(self, name):
        return self if name == "i" else self._out[name]

    def to_numpy(self):
        return self._k

    def validity_numpy(self):
        return np.ones(self._k.shape[0], bool)


def S(*names):
    return [("sum", col(nm)) for nm in names]


GT250 = lambda c="c": (lambda: col(c) > 250.0)  # noqa: E731
F2 = {"gb_path": 2}

# id, frame, key, aggregations (kind, expr), predicate, maintain_order, options, expected variant subset
CASES = [
    # ---- launch_fast_nulls (a validity bitmap on the key, a value or the predicate's column)
    ("nulls_var5_nacc1", "plain", "k", lambda: S("cn"), GT250("cn"), False, {**F2, "sum_pos": 1},
     dict(nulls=True, var=5, nacc=1, pred=1, sumonly=True, limbs=2, pack=0, runs=False, deriv=False)),
    ("nulls_var5_nacc4", "plain", "k", lambda: S("b", "e", "f", "cn"), GT250("cn"), False, {**F2, "sum_pos": 1},
     dict(nulls=True, var=5, nacc=4, pred=1, sumonly=True, limbs=2)),
    ("nulls_sumonly2_nopred", "plain", "k", lambda: S("cn", "b"), None, False, F2,
     dict(nulls=True, var=0, nacc=2, pred=0, sumonly=True, limbs=2)),
    # (b first: the predicate's column is not the last acc, so not VAR 5)
    ("nulls_sumonly2_pred", "plain", "k", lambda: S("b", "cn"), lambda: col("b") > 1.0, False, F2,
     dict(nulls=True, var=0, nacc=2, pred=1, sumonly=True, limbs=2)),
    ("nulls_general_nopred", "plain", "kn", lambda: S("cn") + [("min", col("q"))], None, False, F2,
     dict(nulls=True, var=0, nacc=2, pred=0, sumonly=False, limbs=3)),
    ("nulls_general_pred", "plain", "k", lambda: S("cn") + [("min", col("q"))], GT250(), False, F2,
     dict(nulls=True, var=0, nacc=2, pred=1, sumonly=False, limbs=3)),
    # ---- launch_fast
    ("fast_runs_sumonly", "sorted", "k", lambda: S("c", "b"), None, False, F2,
     dict(runs=True, sumonly=True, limbs=2, var=0, nacc=2, pred=0, pack=0, nulls=False, deriv=False)),
    ("fast_var5", "plain", "k", lambda: S("b", "e", "f", "c"), GT250(), False, {**F2, "sum_pos": 1},
     dict(var=5, nacc=4, pred=1, sumonly=True, limbs=2, runs=False, pack=0, nulls=False)),
    ("fast_sumonly2", "plain", "k", lambda: S("c", "b"), None, False, F2,
     dict(var=0, runs=False, sumonly=True, limbs=2, nacc=2, pred=0, pack=0, nulls=False, deriv=False)),
    ("fast_runs_mixed2", "sorted", "k", lambda: S("c") + [("min", col("q")), ("max", col("b"))], None, False, F2,
     dict(runs=True, sumonly=False, limbs=2, var=0, nacc=3, deriv=False)),
    ("fast_sumonly3", "plain", "k", lambda: S("w", "c"), None, False, F2,
     dict(var=0, runs=False, sumonly=True, limbs=3, nacc=2, deriv=False)),
    ("fast_mixed3", "plain", "k", lambda: S("w") + [("min", col("q"))], GT250(), False, F2,
     dict(var=0, runs=False, sumonly=False, limbs=3, nacc=2, pred=1, deriv=False)),
    ("fast_sumonly2_pack1", "packed", "i", lambda: S("c", "b"), GT250(), False, {},
     dict(pack=1, var=0, runs=False, sumonly=True, limbs=2, nacc=2, pred=1)),
    ("fast_sumonly2_pack2", "packed", "s", lambda: S("c", "b"), GT250(), False, {},
     dict(pack=2, var=0, runs=False, sumonly=True, limbs=2, nacc=2, pred=1)),
    ("fast_mixed_pack1", "packed", "i", lambda: S("c") + [("min", col("q")), ("max", col("b"))], None, False, {},
     dict(pack=1, var=0, runs=False, sumonly=False, limbs=3, nacc=3, pred=0)),
    ("fast_deriv2", "plain", "k", lambda: [("sum", col("c") * col("b"))], None, False, F2,
     dict(deriv=True, var=0, sumonly=True, limbs=2, nacc=1, runs=False)),
    ("fast_deriv3", "plain", "k", lambda: [("sum", col("w") * col("b"))], GT250(), False, F2,
     dict(deriv=True, var=0, sumonly=True, limbs=3, nacc=1, pred=1, runs=False)),
    # ---- launch_fast_var: var() / std() of one column (x, x * x and its error: three accs)
    ("var1_mixed", "plain", "k", ("var", "v2", 1), None, True, F2,
     dict(var=1, sumonly=False, limbs=3, nacc=3, pred=0)),
    ("var4", "plain", "k", ("var", "v2", 1), lambda: col("v2") > 300.0, False, {**F2, "var_pos": 1},
     dict(var=4, sumonly=True, limbs=2, nacc=3, pred=1)),
    ("var1_2limb", "plain", "k", ("var", "v2", 0), None, False, F2,
     dict(var=1, sumonly=True, limbs=2, nacc=3, pred=0)),
    ("var1_3limb", "plain", "k", ("var", "v3", 1), None, False, F2,
     dict(var=1, sumonly=True, limbs=3, nacc=3, pred=0)),
    # ---- launch_fast_pair: a product's sum next to one operand's (VAR 2: product first; VAR 3: second)
    ("pair2_2limb", "plain", "k", lambda: [("sum", col("c") * col("b"))] + S("b"), GT250(), False, F2,
     dict(var=2, sumonly=True, limbs=2, nacc=2, runs=False, pred=1)),
    ("pair3_2limb", "plain", "k", lambda: S("b") + [("sum", col("c") * col("b"))], None, False, F2,
     dict(var=3, sumonly=True, limbs=2, nacc=2, runs=False, pred=0)),
    ("pair2_runs", "sorted", "k", lambda: [("sum", col("c") * col("b"))] + S("b"), None, False, F2,
     dict(var=2, sumonly=True, limbs=2, nacc=2, runs=True)),
    ("pair3_runs", "sorted", "k", lambda: S("b") + [("sum", col("c") * col("b"))], GT250(), False, F2,
     dict(var=3, sumonly=True, limbs=2, nacc=2, runs=True, pred=1)),
    ("pair2_3limb", "plain", "k", lambda: [("sum", col("w") * col("b"))] + S("b"), None, False, F2,
     dict(var=2, sumonly=True, limbs=3, nacc=2, runs=False)),
    ("pair3_3limb", "plain", "k", lambda: S("b") + [("sum", col("w") * col("b"))], GT250(), False, F2,
     dict(var=3, sumonly=True, limbs=3, nacc=2, runs=False, pred=1)),
]


def _var_ref(vals, ddof):
    """The fused variance of fin_slot (groupby.hip) in exact arithmetic:
    num = n sum(x^2) - sum(x)^2 rounded once to f64, then the two f64
    divisions (num / n) / (n - ddof)."""
    m, e = np.frexp(vals)
    mi, e = (m * 2.0**53).astype(np.int64).tolist(), (e - 53).tolist()
    emin = min(e)
    ints = [a << (b - emin) for a, b in zip(mi, e)]
    n = len(ints)
    s1 = sum(ints)
    num = float(Fraction(n * sum(v * v for v in ints) - s1 * s1) * Fraction(2) ** (2 * emin))
    return (num / float(n)) / float(n - ddof)


def _check_var(df, cols, key, xname, ddof, pred, maintain, n):
    lf = df.lazy()
    sel = np.ones(n, bool)
    if pred is not None:
        lf = lf.filter(pred())
        sel = cols[xname][0] > 300.0
    info = {}
    out = lf.group_by(key, maintain_order=maintain).agg(col(xname).var(ddof=ddof).alias("v")).collect(info=info)
    k, x = cols[key][0][sel], cols[xname][0][sel]
    uniq, first, inv = np.unique(k, return_index=True, return_inverse=True)
    gk, gv, gvalid = out[key].to_numpy(), out["v"].to_numpy(), out["v"].validity_numpy()
    assert out.height == uniq.shape[0]
    if maintain:
        assert np.array_equal(gk, uniq[np.argsort(first)])  # first-occurrence order
    go = np.argsort(gk)
    assert np.array_equal(gk[go], uniq)
    order = np.argsort(inv, kind="stable")
    bounds = np.searchsorted(inv[order], np.arange(uniq.shape[0] + 1))
    for g in range(uniq.shape[0]):
        vals = x[order[bounds[g]:bounds[g + 1]]]
        if vals.shape[0] <= ddof:
            assert not gvalid[go[g]], (g, uniq[g])
            continue
        assert gvalid[go[g]], (g, uniq[g])
        want = _var_ref(vals, ddof)
        assert _bits(gv[go[g]]) == _bits(want), (uniq[g], gv[go[g]], want)
    return info


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_variant_vs_oracle(gpu, plgpu_option, case):
    """Bit-exact vs the oracle, and the launcher branch the row names ran."""
    cid, kind, key, build, pred, maintain, opts, expect = case
    df, cols = _frame(kind)
    n = N_PACKED if kind == "packed" else N
    for name, value in opts.items():
        plgpu_option(name, value)
    if isinstance(build, tuple):
        _, xname, ddof = build
        info = _check_var(df, cols, key, xname, ddof, pred, maintain, n)
    else:
        specs = build()
        exp = _oracle(cols, "i" if key == "s" else key, specs, pred() if pred else None, n, names_extra=("w",))
        out, info = _gpu(df, key, specs, pred() if pred else None, maintain)
        if key == "s":
            out, key = _StrKeyAsInt(out), "i"
        _compare(out, key, exp, len(specs), maintain, (cid, info))
    fv = fused_variant(info)
    assert fv["ran"], (cid, "the fused kernel did not run", info)
    got = {name: fv[name] for name in expect}
    assert got == expect, (cid, fv, info)
    assert info["path"] == (4 if expect["var"] in (1, 4) else 2 if expect["sumonly"] else 1), (cid, info)
    assert info["sum_limbs"] == (expect["limbs"] if expect["sumonly"] else 3), (cid, info)
    assert info["key_pack"] == (1 if expect.get("pack", 0) else 0), (cid, info)
