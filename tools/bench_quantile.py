"""median / quantile at scale (DESIGN.md "Quantile").

Kernels.  plgpu_segment_quantile's four launches alone, timed by the library's
HIP-event timer (option "ktime"), the mean of --steps calls after --warmup.
The inputs are made in the sorted layout, so no sort runs: the values ascend
over the whole column (so in every segment), and the segment starts follow G:

  g1      no segment column: one segment
  g1000   1e3 segments of equal length
  g8th    a segment every 8 rows (G = n / 8)

with nq = 1 (the median) and nq = 3 (q = 0.25 / 0.5 / 0.75, linear), for an
Int64 and a Float64 column, null-free and (`_valid`) with a validity buffer of
set bits, which sends every segment through the binary search.  The yardstick,
an existing kernel in the same process at the same n: plgpu_cumulative MAX of an
Int64 column, the sibling scan that reads and writes every row.  `checks` holds
every case's summed kernel time over cum_max's (the bar: below 1).

End to end.  group_by("k").agg(pl.col("x").median()) with --groups groups, by
the host clock around a call that ends in a synchronise, and the same query
step by step (the steps of frame._group_by_quantile, each ended by a
synchronise): the group-by of the keys, the row ids and the join, the sort,
the gather and the segment starts, and plgpu_segment_quantile.

    python tools/bench_quantile.py [--rows 1e8] [--out profiles/quantile_1e8.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--groups", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import polaroid_amd as pl
    from polaroid_amd import _native as N
    from polaroid_amd import frame as F

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n = int(args.rows) // 64 * 64
    ones = torch.full((n // 8,), 255, device="cuda", dtype=torch.uint8)

    def column(dtype, valid):
        return pl.Series.from_torch("x", torch.arange(n, device="cuda", dtype=dtype), ones if valid else None)

    def starts(rows):
        bitmap = torch.zeros(n // 8, device="cuda", dtype=torch.uint8)
        for r in rows:
            bitmap[r >> 3] |= 1 << (r & 7)
        return pl.Series.from_device("starts", pl.Boolean, bitmap.data_ptr(), n, keepalive=bitmap)

    eighth = torch.full((n // 8,), 1, device="cuda", dtype=torch.uint8)
    segs = {"g1": None, "g1000": starts([j * (n // 1000) for j in range(1000)]),
            "g8th": pl.Series.from_device("starts", pl.Boolean, eighth.data_ptr(), n, keepalive=eighth)}
    quantiles = {1: ([0.5], ["linear"]), 3: ([0.25, 0.5, 0.75], ["linear"] * 3)}
    N.set_option("ktime", 1)
    recs = {}

    def timed(case, fn, prefixes):
        for _ in range(args.warmup):
            fn()
        N.ktime_read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        kern = {k: round(ms / args.steps, 4) for k, (ms, cnt) in sorted(N.ktime_read().items())
                if k.startswith(prefixes)}
        rec = {"case": case, "rows": n, "wall_ms": round(wall, 3), "kernels_ms": kern,
               "kernel_ms": round(sum(kern.values()), 4)}
        print(json.dumps(rec), flush=True)
        recs[case] = rec
        return rec

    def quantile(x, seg, nq):
        qs, ms = quantiles[nq]

        def run():
            outs = (N.Column * nq)()
            N.check(N.lib().plgpu_segment_quantile(
                C.byref(x._col), None if seg is None else C.byref(seg._col), (C.c_double * nq)(*qs),
                (C.c_int32 * nq)(*[N.QUANTILE[m] for m in ms]), nq, outs, None))
            for i in range(nq):
                N.lib().plgpu_column_release(C.byref(outs[i]))
        return run

    yard = column(torch.int64, False)

    def cum_max():
        out = N.Column()
        N.check(N.lib().plgpu_cumulative(C.byref(yard._col), None, N.CUM["max"], C.byref(out), None))
        N.lib().plgpu_column_release(C.byref(out))

    cm = timed("cum_max", cum_max, ("cum_",))
    checks = {}
    for dname, dtype in (("int64", torch.int64), ("float64", torch.float64)):
        for valid in (False, True):
            x = column(dtype, valid)
            for sname, seg in segs.items():
                for nq in (1, 3):
                    name = f"{sname}_nq{nq}_{dname}" + ("_valid" if valid else "")
                    rec = timed(name, quantile(x, seg, nq), ("quantile_",))
                    checks[name + "_over_cum_max"] = round(rec["kernel_ms"] / cm["kernel_ms"], 4)
            del x
    checks["worst_over_cum_max"] = max(checks.values())
    print(json.dumps({"checks": checks}), flush=True)

    # ---- end to end
    del yard
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    k = torch.randint(0, args.groups, (n,), device="cuda", generator=g, dtype=torch.int64)
    xv = torch.randn(n, device="cuda", generator=g, dtype=torch.float64)
    df = pl.DataFrame([pl.Series.from_torch("k", k), pl.Series.from_torch("x", xv)])
    sync = lambda: N.check(N.lib().plgpu_synchronize(None))  # noqa: E731

    def query():
        df.group_by("k").agg(pl.col("x").median())
        sync()

    e2e = timed("group_by_median", query, ("quantile_",))
    phases = {}

    def phase(name, fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        phases[name] = phases.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return out

    def stepwise():
        base = phase("group_by_len", lambda: F._group_by(df, "k", [pl.len().alias("__q_len")], True, None, None))

        def ids():
            right = pl.DataFrame([base["k"], F._row_ids(base["__q_len"]).alias("__q_gid")])
            return F._join(pl.DataFrame([df["k"]]), right, "k", "k", "_right", "m:m", True, "left", "left", None)["__q_gid"]
        gid = phase("row_ids_join", ids)
        cols = [gid, df["x"]]

        def sort():
            idx = N.Column()
            N.check(N.lib().plgpu_arg_sort_multi(F._col_array(cols), 2, (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 1),
                                                 C.byref(idx), None))
            return pl.Series._from_native("__idx", idx)
        idx = phase("sort", sort)

        def gather():
            got = (N.Column * 2)()
            N.check(N.lib().plgpu_gather(F._col_array(cols), 2, C.byref(idx._col), got, None))
            srt = [pl.Series._from_native(c.name, got[i]) for i, c in enumerate(cols)]
            return srt, F._segment_starts(srt[:1])[0]
        srt, seg = phase("gather_segment_starts", gather)
        phase("segment_quantile", quantile(srt[1], seg, 1))

    for _ in range(args.warmup):
        stepwise()
    phases.clear()
    for _ in range(args.steps):
        stepwise()
    phases = {k: round(v / args.steps, 3) for k, v in phases.items()}
    e2e["phases_ms"] = phases
    print(json.dumps({"group_by_median_phases_ms": phases}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": n, "groups": args.groups, "steps": args.steps, "warmup": args.warmup,
                       "device": torch.cuda.get_device_name(0), "checks": checks, "records": list(recs.values())},
                      f, indent=1)


if __name__ == "__main__":
    main()
