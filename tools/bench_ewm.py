"""ewm_mean at scale (DESIGN.md "Exponentially weighted mean"): per-kernel
times by the library's HIP-event timer (option "ktime"), the mean of --steps
calls after --warmup, of one Float64 column of prices:

  ewm_mean(alpha=0.05) with adjust true / false, null-free / about 10 % nulls
  (independent rows), plain / with --segments evenly spaced segment starts --
  the reduce / totals / apply split of each case;
  cum_max() of the same column in the same process: it moves the same
  24 algorithmic bytes per row (8 B read by each of the two tile launches, 8 B
  written), so it is the yardstick.

`checks` holds every case's summed kernel time over cum_max's, its apply launch
over cum_max's, and segmented over plain.

    python tools/bench_ewm.py [--rows 1e9] [--out profiles/ewm_1e9.json]
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
    ap.add_argument("--segments", type=int, default=100)
    ap.add_argument("--alpha", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import polaroid_amd as pl
    from polaroid_amd import _native as N

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n = int(args.rows) // 64 * 64
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    close = torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 160 + 170
    valid = torch.rand(n, device="cuda", generator=g, dtype=torch.float32) >= 0.1
    null_frac = 1.0 - float(valid.sum().item()) / n
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device="cuda", dtype=torch.uint8)
    vbits = (valid.view(-1, 8).to(torch.uint8) * w).sum(1, dtype=torch.uint8).contiguous()
    del valid
    columns = {"dense": pl.Series.from_torch("close", close), "nulls10": pl.Series.from_torch("close", close, vbits)}
    bitmap = torch.zeros(n // 8, device="cuda", dtype=torch.uint8)
    for j in range(args.segments):
        r = j * n // args.segments
        bitmap[r >> 3] |= 1 << (r & 7)
    seg = pl.Series.from_device("seg", pl.Boolean, bitmap.data_ptr(), n, keepalive=bitmap)
    N.set_option("ktime", 1)
    recs = {}

    def timed(case, fn, prefix):
        for _ in range(args.warmup):
            fn()
        N.ktime_read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        kern = {k: round(ms / args.steps, 4) for k, (ms, cnt) in sorted(N.ktime_read().items()) if k.startswith(prefix)}
        total = sum(kern.values())
        rec = {"case": case, "rows": n, "wall_ms": round(wall, 3), "kernels_ms": kern, "kernel_ms": round(total, 4),
               "bytes_per_row": 24, "frac": round(n * 24 / (total * 1e-3) / HBM_PEAK, 4)}
        print(json.dumps(rec), flush=True)
        recs[case] = rec
        return rec

    def ewm(s, adjust, segd):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_ewm_mean(C.byref(s._col), C.byref(seg._col) if segd else None, args.alpha,
                                           int(adjust), 0, 1, C.byref(out), None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    def cum_max(s):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_cumulative(C.byref(s._col), None, N.CUM["max"], C.byref(out), None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    checks = {}
    for nulls, s in columns.items():
        cm = timed(f"cum_max_{nulls}", cum_max(s), "cum_")
        for adjust in (True, False):
            name = f"{'adjust' if adjust else 'noadjust'}_{nulls}"
            plain = timed(name, ewm(s, adjust, False), "ewm_")
            segd = timed(name + "_seg", ewm(s, adjust, True), "ewm_")
            for rec in (plain, segd):
                checks[rec["case"] + "_over_cum_max"] = round(rec["kernel_ms"] / cm["kernel_ms"], 4)
                checks[rec["case"] + "_apply_over_cum_max_apply"] = round(
                    rec["kernels_ms"]["ewm_apply_kernel"] / cm["kernels_ms"]["cum_apply_kernel"], 4)
            checks[name + "_segmented_over_plain"] = round(segd["kernel_ms"] / plain["kernel_ms"], 4)
    print(json.dumps({"checks": checks}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": n, "segments": args.segments, "alpha": args.alpha, "steps": args.steps,
                       "warmup": args.warmup, "hbm_peak": HBM_PEAK, "null_fraction": round(null_frac, 5),
                       "checks": checks, "records": list(recs.values())}, f, indent=1)


if __name__ == "__main__":
    main()
