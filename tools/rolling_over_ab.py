"""Rolling windows, plain against segmented, and an earlier build of the
library against this one (DESIGN.md "Window expressions over groups"):

  plain      rolling_mean(20) and rolling_std(20) of one Float64 column, on
             the library --base names (an earlier build, e.g. the parent
             commit's) and on this tree's, alternating --rounds times, each
             library in a process of its own (PLGPU_LIB);
  segmented  plgpu_rolling_segmented, same column, --segments evenly spaced
             segment starts (this tree's library only);
  over       rolling_mean(20).over("symbol") end to end on keys that arrive
             sorted and on the same rows shuffled: wall time per step and
             the kernels the library's timer names (seg_starts_kernel, the
             sort's passes, invert_perm_kernel, the rolling kernel).

Kernel times are the library's HIP-event timer (option "ktime"), the mean
over --steps calls after --warmup.  One JSON line per measurement; --out
also collects them in one file.

    python tools/rolling_over_ab.py --base /path/to/libpolaroid_gpu_parent.so [--rows 1e9] [--out profiles/x.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _child(args):
    import numpy as np
    import torch

    from polaroid_amd import _native as N

    exported = C.CDLL(N.LIB_PATH)
    for nm in list(N.SIGNATURES):  # an earlier build lacks the newer entry points
        if not hasattr(exported, nm):
            del N.SIGNATURES[nm]
    import polaroid_amd as pl

    n = int(args.rows)
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    close = torch.rand(n, device="cuda", generator=g, dtype=torch.float64) * 400 + 100
    s = pl.Series.from_torch("close", close)
    N.set_option("ktime", 1)
    recs = []

    def timed(tag, fn, kernels):
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
        rec = {"lib": args.tag, "case": tag, "rows": n, "wall_ms": round(wall, 3),
               "kernels_ms": {k: round(ms / cnt, 4) for k, (ms, cnt) in sorted(kt.items())
                              if kernels is None or any(k.startswith(p) for p in kernels)}}
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    def plain(kind, ddof=0):
        def run():
            out = N.Column()
            N.check(N.lib().plgpu_rolling(C.byref(s._col), N.ROLLING[kind] | (ddof << 8), 20, 20, 0, C.byref(out),
                                          None))
            N.lib().plgpu_column_release(C.byref(out))
        return run

    timed("plain_mean20", plain("mean"), ("rl_",))
    timed("plain_std20", plain("std", 1), ("rl_",))
    if args.tag == "new":
        starts = np.zeros(n, bool)
        starts[(np.arange(args.segments, dtype=np.int64) * n) // args.segments] = True
        seg = pl.Series.from_numpy("seg", starts)

        def segmented(kind, ddof=0):
            def run():
                out = N.Column()
                N.check(N.lib().plgpu_rolling_segmented(C.byref(s._col), C.byref(seg._col),
                                                        N.ROLLING[kind] | (ddof << 8), 20, 20, 0, C.byref(out), None))
                N.lib().plgpu_column_release(C.byref(out))
            return run

        timed("segmented_mean20", segmented("mean"), ("rl_",))
        timed("segmented_std20", segmented("std", 1), ("rl_",))
        if args.over:
            m = int(args.over_rows)
            sym = torch.arange(m, device="cuda", dtype=torch.int64) // max(1, m // args.segments)
            cl = close[:m]
            e = pl.col("close").rolling_mean(20).over("symbol")
            df = pl.DataFrame([pl.Series.from_torch("symbol", sym), pl.Series.from_torch("close", cl)])
            timed("over_presorted", lambda: df.select(e), None)
            perm = torch.randperm(m, device="cuda", generator=g)
            sh_sym, sh_cl = sym[perm].contiguous(), cl[perm].contiguous()
            del perm
            df2 = pl.DataFrame([pl.Series.from_torch("symbol", sh_sym), pl.Series.from_torch("close", sh_cl)])
            timed("over_shuffled", lambda: df2.select(e), None)
    if args.child_out:
        with open(args.child_out, "w") as f:
            json.dump(recs, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", help="an earlier build of the library to compare against")
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--over-rows", type=float, default=None, help="rows of the over() runs (default: --rows)")
    ap.add_argument("--segments", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-over", dest="over", action="store_false")
    ap.add_argument("--out")
    ap.add_argument("--tag", help=argparse.SUPPRESS)
    ap.add_argument("--child-out", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.over_rows is None:
        args.over_rows = args.rows
    if args.tag:
        return _child(args)
    runs = []
    order = (["parent", "new"] if args.base else ["new"]) * args.rounds
    for i, tag in enumerate(order):
        env = dict(os.environ)
        if tag == "parent":
            env["PLGPU_LIB"] = os.path.abspath(args.base)
        else:
            env.pop("PLGPU_LIB", None)
        tmp = f"{args.out}.{i}.tmp" if args.out else ""
        cmd = [sys.executable, os.path.abspath(__file__), "--tag", tag, "--rows", str(args.rows), "--over-rows",
               str(args.over_rows), "--segments", str(args.segments), "--steps", str(args.steps), "--warmup",
               str(args.warmup)]
        # the end-to-end over() runs once, in the last process of this tree's library
        if not (args.over and tag == "new" and i == len(order) - 1):
            cmd.append("--no-over")
        if tmp:
            cmd += ["--child-out", tmp]
        subprocess.run(cmd, env=env, check=True, timeout=900)
        if tmp:
            with open(tmp) as f:
                runs.append({"round": i // (2 if args.base else 1), "lib": tag, "records": json.load(f)})
            os.remove(tmp)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": int(args.rows), "segments": args.segments, "steps": args.steps, "runs": runs}, f,
                      indent=1)


if __name__ == "__main__":
    main()
