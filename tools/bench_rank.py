"""rank at scale (DESIGN.md "Rank"): plgpu_rank's three launches alone, timed
by the library's HIP-event timer (option "ktime"), the mean of --steps calls
after --warmup.  The inputs are made in the sorted layout, so no sort runs:
sorted_idx is a random permutation (the scatter goes to random rows, as after
a sort of shuffled data), and the tie starts follow the shape:

  distinct   every sorted row starts a run
  d1000      1e3 runs of equal length
  one        one run

for every method, plain / with --segments evenly spaced segment starts, with
an Int64 and a Float64 ranked column (the kernels read only its validity, so
the dtype is expected to change nothing; both are run).  Null-free columns.

Two yardsticks, existing kernels, in the same process at the same n:
  cum_max     plgpu_cumulative MAX of an Int64 column, the sibling scan
  inv_gather  plgpu_invert_permutation of sorted_idx plus plgpu_gather of one
              UInt32 column through the inverse: the two passes that the
              scatter inside rank_apply_kernel replaces
plgpu_gather's kernel carries no timer scope, so inv_gather is timed by the
host clock around its two calls, each of which ends in a stream synchronise;
every case records that wall time too.  `checks` holds every case's summed
kernel time over cum_max's, and its wall time over inv_gather's and over
inv_gather + cum_max in wall time (the bar: below 1).

    python tools/bench_rank.py [--rows 1e9] [--out profiles/rank_1e9.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("distinct", "d1000", "one")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--segments", type=int, default=100)
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
    perm = torch.randperm(n, device="cuda", generator=g).to(torch.int32)  # (the bits of the UInt32 row ids)
    idx = pl.Series.from_device("idx", pl.UInt32, perm.data_ptr(), n, keepalive=perm)
    ranked = {"int64": pl.Series.from_torch("x", torch.zeros(n, device="cuda", dtype=torch.int64)),
              "float64": pl.Series.from_torch("x", torch.zeros(n, device="cuda", dtype=torch.float64))}

    def starts(rows):
        bitmap = torch.zeros(n // 8, device="cuda", dtype=torch.uint8)
        for r in rows:
            bitmap[r >> 3] |= 1 << (r & 7)
        return pl.Series.from_device("starts", pl.Boolean, bitmap.data_ptr(), n, keepalive=bitmap)

    every = torch.full((n // 8,), 255, device="cuda", dtype=torch.uint8)
    ties = {"distinct": pl.Series.from_device("tie", pl.Boolean, every.data_ptr(), n, keepalive=every),
            "d1000": starts([j * n // 1000 for j in range(1000)]), "one": starts([0])}
    seg = starts([j * n // args.segments for j in range(args.segments)])
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

    def rank(x, tie, segd, method):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_rank(C.byref(idx._col), C.byref(x._col), C.byref(tie._col),
                                       C.byref(seg._col) if segd else None, C.byref(x._col), N.RANK[method],
                                       C.byref(out), None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    def cum_max():
        out = N.Column()
        N.check(N.lib().plgpu_cumulative(C.byref(ranked["int64"]._col), None, N.CUM["max"], C.byref(out), None))
        N.lib().plgpu_column_release(C.byref(out))

    def inv_gather():
        inv, got = N.Column(), (N.Column * 1)()
        N.check(N.lib().plgpu_invert_permutation(C.byref(idx._col), C.byref(inv), None))
        N.check(N.lib().plgpu_gather((N.Column * 1)(idx._col), 1, C.byref(inv), got, None))
        N.lib().plgpu_column_release(C.byref(got[0]))
        N.lib().plgpu_column_release(C.byref(inv))

    cm = timed("cum_max", cum_max, ("cum_",))
    ig = timed("inv_gather", inv_gather, ("invert_perm_",))  # (kernels_ms: the inversion alone)
    bar = ig["wall_ms"] + cm["wall_ms"]
    checks = {"inv_gather_wall_over_cum_max_wall": round(ig["wall_ms"] / cm["wall_ms"], 4)}
    for dtype, x in ranked.items():
        for shape in SHAPES:
            for segd in (False, True):
                for method in N.RANK:
                    name = f"{method}_{shape}_{dtype}" + ("_seg" if segd else "")
                    rec = timed(name, rank(x, ties[shape], segd, method), ("rank_",))
                    checks[name + "_over_cum_max"] = round(rec["kernel_ms"] / cm["kernel_ms"], 4)
                    checks[name + "_over_inv_gather"] = round(rec["wall_ms"] / ig["wall_ms"], 4)
                    checks[name + "_over_bar"] = round(rec["wall_ms"] / bar, 4)
    worst = max(v for k, v in checks.items() if k.endswith("_over_bar"))
    checks["worst_over_bar"] = worst
    print(json.dumps({"checks": {k: v for k, v in checks.items() if not k.endswith(("_cum_max", "_inv_gather"))}}),
          flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": n, "segments": args.segments, "steps": args.steps, "warmup": args.warmup,
                       "checks": checks, "records": list(recs.values())}, f, indent=1)


if __name__ == "__main__":
    main()
