"""Forward / backward fill at scale (DESIGN.md "Fill strategies"): per-kernel
times by the library's HIP-event timer (option "ktime"), the mean of --steps
calls after --warmup, of one Float64 column with about 10 % nulls placed in
runs:

  forward_fill(), forward_fill(limit=5), backward_fill(), and forward_fill()
  with --segments evenly spaced segment starts -- the reduce / totals / apply
  split, and `frac`, the fraction of the 8 TB/s HBM peak at the algorithmic
  bytes (8 B read + 8 B written + 3 bits per row; 5 bits with segment starts)
  over the summed kernel time;
  shift(1) (16 B/row) and cum_max() (24 B/row) of the same column in the same
  process as yardsticks;
  close.forward_fill().over("symbol") end to end for sorted and shuffled keys.

Null runs: a run starts at a row with probability 0.1 / 32.1; its length is 1
(50 %), 4 (30 %), 32 (15 %) or 512 (5 %) rows, mean 32.1; runs may overlap, so
the measured null fraction (reported) is slightly below 10 %.

    python tools/bench_fill.py [--rows 1e9] [--out profiles/fill_1e9.json]
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
RUN_LENGTHS = ((1, 0.50), (4, 0.30), (32, 0.15), (512, 0.05))


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

    import torch

    import polaroid_amd as pl
    from polaroid_amd import _native as N

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n = int(args.rows) // 64 * 64
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    close = torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 400 + 100

    def null_runs(m):
        """(packed validity bitmap, null fraction) of m rows (m a multiple of 64)."""
        mean_len = sum(length * p for length, p in RUN_LENGTHS)
        u = torch.rand(m, device="cuda", generator=g, dtype=torch.float32)
        delta = torch.zeros(m + 1, device="cuda", dtype=torch.int32)
        lo = 0.0
        for length, p in RUN_LENGTHS:
            hi = lo + p * 0.1 / mean_len
            at = torch.nonzero((u >= lo) & (u < hi)).flatten()
            delta.index_add_(0, at, torch.ones_like(at, dtype=torch.int32))
            delta.index_add_(0, torch.clamp(at + length, max=m), -torch.ones_like(at, dtype=torch.int32))
            lo = hi
        del u
        valid = torch.cumsum(delta[:m], 0, dtype=torch.int32) <= 0
        del delta
        valid[0] = True
        frac = 1.0 - float(valid.sum().item()) / m
        w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device="cuda", dtype=torch.uint8)
        packed = (valid.view(-1, 8).to(torch.uint8) * w).sum(1, dtype=torch.uint8).contiguous()
        return packed, frac

    vbits, null_frac = null_runs(n)
    s_close = pl.Series.from_torch("close", close, vbits)
    bitmap = torch.zeros(n // 8, device="cuda", dtype=torch.uint8)
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
        return rec

    def fill(op, limit, segd):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_fill(C.byref(s_close._col), C.byref(seg._col) if segd else None, N.FILL[op], limit,
                                       C.byref(out), None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    def shift1():
        out = N.Column()
        N.check(N.lib().plgpu_lag(C.byref(s_close._col), None, N.LAG["shift"], 1, 0, 0, C.byref(out), None))
        N.lib().plgpu_column_release(C.byref(out))

    def cum_max():
        out = N.Column()
        N.check(N.lib().plgpu_cumulative(C.byref(s_close._col), None, N.CUM["max"], C.byref(out), None))
        N.lib().plgpu_column_release(C.byref(out))

    plain_bytes, seg_bytes = 16 + 3 / 8, 16 + 5 / 8
    ff = timed("forward_fill", fill("forward", -1, False), ("fill_",), plain_bytes)
    timed("forward_fill_limit5", fill("forward", 5, False), ("fill_",), plain_bytes)
    timed("backward_fill", fill("backward", -1, False), ("fill_",), plain_bytes)
    fs = timed("forward_fill_seg", fill("forward", -1, True), ("fill_",), seg_bytes)
    timed("shift1_f64", shift1, ("lag_",), 16)
    cm = timed("cum_max_f64", cum_max, ("cum_",), 24)
    checks = {"forward_fill_over_cum_max": round(ff["kernel_ms"] / cm["kernel_ms"], 4),
              "segmented_over_plain": round(fs["kernel_ms"] / ff["kernel_ms"], 4)}
    print(json.dumps({"checks": checks}), flush=True)
    if args.over:
        m = int(args.over_rows or n) // 64 * 64
        sym = torch.arange(m, device="cuda", dtype=torch.int64) // max(1, m // args.segments)
        cl, vb = close[:m], vbits[:m // 8]
        e = pl.col("close").forward_fill().over("symbol")
        df = pl.DataFrame([pl.Series.from_torch("symbol", sym), pl.Series.from_torch("close", cl, vb)])
        timed("over_presorted", lambda: df.select(e), None, 0, m)
        perm = torch.randperm(m, device="cuda", generator=g)
        sh_sym = sym[perm].contiguous()
        del perm
        df2 = pl.DataFrame([pl.Series.from_torch("symbol", sh_sym), pl.Series.from_torch("close", cl, vb)])
        timed("over_shuffled", lambda: df2.select(e), None, 0, m)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": n, "segments": args.segments, "steps": args.steps, "warmup": args.warmup,
                       "hbm_peak": HBM_PEAK, "null_fraction": round(null_frac, 5),
                       "null_run_lengths": [{"rows": length, "share_of_runs": p} for length, p in RUN_LENGTHS],
                       "null_run_start_probability": 0.1 / sum(length * p for length, p in RUN_LENGTHS),
                       "checks": checks, "records": recs}, f, indent=1)


if __name__ == "__main__":
    main()
