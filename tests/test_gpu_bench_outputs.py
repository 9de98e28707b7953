"""bench.py --dump-outputs: a plain run at a small size writes the last timed
step's result frame, one float64 .npy per column in ascending key order, and
its JSON line is the headline alone (every other leg is behind --full).  The
inputs are seeded, so the frame is regenerated here with the bench's own
generator and the dumped sums are checked bit for bit against math.fsum."""

import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the bench's own data generator)

ROWS, GROUPS, STEPS, WARMUP = 100_003, 100, 3, 1
COLS = ("open", "high", "low", "close")


def test_plain_run_dumps_the_last_steps_frame(gpu, tmp_path):
    import torch

    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--rows", str(ROWS), "--groups", str(GROUPS),
                        "--dump-outputs", str(d)], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert line["unit"] == "Mrows/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert math.isclose(line["value"], ROWS / line["ms_per_step"] / 1e3, rel_tol=0.01)
    assert line["cpu_baseline"] is None
    assert not {"vwap", "std", "nulls", "keys", "many_groups", "filter", "sort", "join", "plugin"} & set(line)

    assert sorted(os.listdir(d)) == sorted(c + ".npy" for c in ("symbol",) + COLS)
    got = {c: np.load(d / (c + ".npy")) for c in ("symbol",) + COLS}
    assert all(a.dtype == np.float64 for a in got.values())

    sym, cols = bench.make_data(torch, ROWS, GROUPS, seed=1234)
    sym = sym.cpu().numpy()
    cols = {c: t.cpu().numpy() for c, t in cols.items()}
    sel = cols["close"] > bench.THRESHOLD
    keys = np.unique(sym[sel])
    assert 0 < keys.size <= GROUPS
    assert np.array_equal(got["symbol"], keys.astype(np.float64))
    for c in COLS:
        want = np.array([math.fsum(cols[c][sel & (sym == k)]) for k in keys])
        assert np.array_equal(got[c].view(np.uint64), want.view(np.uint64)), c
