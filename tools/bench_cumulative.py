"""Cumulative and lag kernels at scale (DESIGN.md "Cumulative and lag
expressions"): per-kernel times by the library's HIP-event timer (option
"ktime"), the mean of --steps calls after --warmup, each case plain and with
--segments evenly spaced segment starts:

  cum_sum of Float64 prices and of Int64, cum_max of Float64 (24 B/row: the
  reduce reads the column, the apply reads it again and writes the result),
  shift(1) and diff(1) of Float64 (16 B/row), +1 bit/row when segmented;
  rolling_sum(20) of the same prices in the same process as a yardstick;
  close.cum_sum().over("symbol") end to end for sorted and shuffled keys.

`frac` is the fraction of the 8 TB/s HBM peak at those algorithmic bytes over
the summed kernel time.  One JSON line per case; --out collects them.

    python tools/bench_cumulative.py [--rows 1e9] [--out profiles/cumulative_1e9.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--over-rows", type=float, default=None, help="rows of the over() runs (default: --rows)")
    ap.add_argument("--segments", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-over", dest="over", action="store_false")
    ap.add_argument("--out")
    args = ap.parse_args()
    torch_threads = min(16, os.cpu_count() or 1)

    import torch

    import polaroid_amd as pl
    from polaroid_amd import _native as N

    torch.set_num_threads(torch_threads)
    n = int(args.rows)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    close = torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 400 + 100
    ints = torch.randint(-10**6, 10**6, (n,), device="cuda", generator=g, dtype=torch.int64)
    s_close, s_int = pl.Series.from_torch("close", close), pl.Series.from_torch("volume", ints)
    # the segment starts as a bitmap built on the device (bit i = row i starts a segment)
    bitmap = torch.zeros((n + 63) // 64 * 8, device="cuda", dtype=torch.uint8)
    for j in range(args.segments):
        r = j * n // args.segments
        bitmap[r >> 3] |= 1 << (r & 7)
    seg = pl.Series.from_device("seg", pl.Boolean, bitmap.data_ptr(), n, keepalive=bitmap)
    N.set_option("ktime", 1)
    recs = []

    def timed(case, fn, prefixes, bytes_per_row, rows=n):
        for _ in range(args.warmup):
            fn()
        N.ktime_read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        kt = N.ktime_read()
        kern = {k: round(ms / args.steps, 4) for k, (ms, cnt) in sorted(kt.items())
                if prefixes is None or any(k.startswith(p) for p in prefixes)}
        rec = {"case": case, "rows": rows, "wall_ms": round(wall, 3), "kernels_ms": kern}
        total = sum(kern.values())
        if bytes_per_row and total > 0:
            rec["kernel_ms"] = round(total, 4)
            rec["bytes_per_row"] = bytes_per_row
            rec["frac"] = round(rows * bytes_per_row / (total * 1e-3) / HBM_PEAK, 4)
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    def cum(series, kind, segd):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_cumulative(C.byref(series._col), C.byref(seg._col) if segd else None, N.CUM[kind],
                                             C.byref(out), None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    def lag(op, segd):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_lag(C.byref(s_close._col), C.byref(seg._col) if segd else None, N.LAG[op], 1, 0, 0,
                                      C.byref(out), None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    def rolling():
        out = N.Column()
        N.check(N.lib().plgpu_rolling(C.byref(s_close._col), N.ROLLING["sum"], 20, 20, 0, C.byref(out), None))
        N.lib().plgpu_column_release(C.byref(out))

    timed("rolling_sum20_f64", rolling, ("rl_",), 16)
    for segd in (False, True):
        tag = "_seg" if segd else ""
        bit = 0.125 if segd else 0.0
        timed("cum_sum_f64" + tag, cum(s_close, "sum", segd), ("cum_",), 24 + bit)
        timed("cum_sum_i64" + tag, cum(s_int, "sum", segd), ("cum_",), 24 + bit)
        timed("cum_max_f64" + tag, cum(s_close, "max", segd), ("cum_",), 24 + bit)
        timed("shift1_f64" + tag, lag("shift", segd), ("lag_",), 16 + bit)
        timed("diff1_f64" + tag, lag("diff", segd), ("lag_",), 16 + bit)
    if args.over:
        m = int(args.over_rows or n)
        sym = torch.arange(m, device="cuda", dtype=torch.int64) // max(1, m // args.segments)
        cl = close[:m]
        e = pl.col("close").cum_sum().over("symbol")
        df = pl.DataFrame([pl.Series.from_torch("symbol", sym), pl.Series.from_torch("close", cl)])
        timed("over_presorted", lambda: df.select(e), None, 0, m)
        perm = torch.randperm(m, device="cuda", generator=g)
        sh_sym, sh_cl = sym[perm].contiguous(), cl[perm].contiguous()
        del perm
        df2 = pl.DataFrame([pl.Series.from_torch("symbol", sh_sym), pl.Series.from_torch("close", sh_cl)])
        timed("over_shuffled", lambda: df2.select(e), None, 0, m)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": n, "segments": args.segments, "steps": args.steps, "warmup": args.warmup,
                       "hbm_peak": HBM_PEAK, "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
