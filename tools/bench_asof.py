"""join_asof at scale (DESIGN.md "As-of join"): per-kernel times by the
library's HIP-event timer (option "ktime"), the mean of --steps calls after
--warmup, of plgpu_join_asof on ascending Int64 keys (--rows left keys against
--right right keys over the same range, as trades against quotes):

  staged   option asof_path 1: every tile of left rows searches the window of
           the right column its keys can touch, in LDS where it fits;
  global   option asof_path 2: every row searches the whole right column;
  ranged   every left row searches one of --groups equal slices of the right
           column (the `by` form, its ranges given);
each for the three strategies.  `checks` holds global over staged per strategy
and whether the two wrote the same indices and validity.  `frac` is the
algorithmic bytes (8 B + 4 B + 1 bit per left row, 8 B per right row) over the
kernel time and the HBM peak.

    python tools/bench_asof.py [--rows 1e9] [--right 1e8] [--out profiles/asof_1e9.json]
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
    ap.add_argument("--right", type=float, default=1e8)
    ap.add_argument("--groups", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    import polaroid_amd as pl
    from polaroid_amd import _native as N

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    n, nr = int(args.rows) // 64 * 64, int(args.right) // 64 * 64
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)

    def ascending(m, gap):
        x = torch.randint(0, gap, (m,), device="cuda", generator=g, dtype=torch.int64)
        return torch.cumsum(x, 0)

    ratio = max(1, n // nr)
    left, right = ascending(n, 16), ascending(nr, 16 * ratio)  # the same range; duplicates on both sides
    per = nr // args.groups
    grp = torch.randint(0, args.groups, (n,), device="cuda", generator=g, dtype=torch.int32)
    lo = (grp * per).to(torch.int32).contiguous()
    hi = (lo + per).contiguous()
    del grp
    ls, rs = pl.Series.from_torch("t", left), pl.Series.from_torch("t", right)
    los = pl.Series.from_device("lo", pl.UInt32, lo.data_ptr(), n, keepalive=lo)
    his = pl.Series.from_device("hi", pl.UInt32, hi.data_ptr(), n, keepalive=hi)
    N.set_option("ktime", 1)
    recs = {}

    def call(strategy, ranged, keep=False):
        out = N.Column()
        N.check(N.lib().plgpu_join_asof(C.byref(ls._col), C.byref(rs._col), C.byref(los._col) if ranged else None,
                                        C.byref(his._col) if ranged else None, None, N.ASOF[strategy], 1, 0, 0, 0.0,
                                        C.byref(out), None, None))
        if keep:
            return pl.Series._from_native("idx", out)
        N.lib().plgpu_column_release(C.byref(out))

    def timed(case, fn):
        for _ in range(args.warmup):
            fn()
        N.ktime_read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        kern = {k: round(ms / args.steps, 4) for k, (ms, cnt) in sorted(N.ktime_read().items()) if k.startswith("asof_")}
        total = sum(kern.values())
        nbytes = n * (8 + 4 + 0.125) + nr * 8
        rec = {"case": case, "rows": n, "right_rows": nr, "wall_ms": round(wall, 3), "kernels_ms": kern,
               "kernel_ms": round(total, 4), "frac": round(nbytes / (total * 1e-3) / HBM_PEAK, 4)}
        print(json.dumps(rec), flush=True)
        recs[case] = rec
        return rec

    def same(a, b):
        ta, tb = a.to_torch(), b.to_torch()
        words = (n + 63) // 64
        va = pl.Series.from_device("v", pl.Int64, a._col.validity, words, keepalive=a).to_torch()
        vb = pl.Series.from_device("v", pl.Int64, b._col.validity, words, keepalive=b).to_torch()
        return bool(torch.equal(va, vb)) and bool(torch.equal(ta, tb))

    checks = {}
    for strategy in ("backward", "forward", "nearest"):
        N.set_option("asof_path", 1)
        st = timed(f"staged_{strategy}", lambda: call(strategy, False))
        a = call(strategy, False, keep=True)
        N.set_option("asof_path", 2)
        gl = timed(f"global_{strategy}", lambda: call(strategy, False))
        b = call(strategy, False, keep=True)
        N.set_option("asof_path", 0)
        checks[f"{strategy}_same_result"] = same(a, b)
        checks[f"{strategy}_matched_fraction"] = round(1.0 - a.null_count() / n, 6) if n <= 1 << 26 else None
        del a, b
        checks[f"{strategy}_global_over_staged"] = round(gl["kernel_ms"] / st["kernel_ms"], 4)
        timed(f"ranged_{strategy}", lambda: call(strategy, True))
    print(json.dumps({"checks": checks}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": n, "right_rows": nr, "groups": args.groups, "steps": args.steps, "warmup": args.warmup,
                       "hbm_peak": HBM_PEAK, "tile_rows": N.ASOF_TILE_ROWS, "lds_values": N.ASOF_LDS_VALUES,
                       "checks": checks, "records": list(recs.values())}, f, indent=1)


if __name__ == "__main__":
    main()
