#!/usr/bin/env python3
"""The batch epoch over valid entries beside the plain one: vsom_batch_epoch_masked with three masks and vsom_batch_epoch,
on the same state and rows in the same build.  One JSON line (appended to --out, profiles/masked_train_bench.jsonl by
default):

  epoch_us             one vsom_batch_epoch call (first epoch: the full search), MSE fetched
  all_valid_us         one vsom_batch_epoch_masked call with an all-valid per-row mask (no dirty column)
  one_dirty_us         ... with one column invalid in one row in ten (one dirty column)
  rows10_us            ... with 10 % of all entries invalid at random (every column dirty)
  all_valid_over_epoch, one_dirty_over_epoch, rows10_over_epoch
  valid_bytes          validity bytes a masked call uploads (rows x J)

128 x 128 x 784, 4096 rows.  Before every call the map is set back to the same initial state (outside the timed span), so
every call does the same work.  The calls are warmed up, then timed in rounds -- one call of each kind per round, in
turn, each a blocking call -- and each column is the median over --rounds rounds; the spread column is
(p90 - p10) / median of the plain epoch.

usage: tools/masked_train_bench.py [--rounds 15] [--rows 4096] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen  # noqa: E402
import vsom_amd  # noqa: E402
from vsom_amd import capi  # noqa: E402

W, H, J = 128, 128, 784
SIGMA = 8.0


def run(rows, rounds):
    N, B = W * H, rows
    X = gen.mnist_like(B, seed=3, dim=J)
    init = (gen.random_map(N, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    rng = np.random.default_rng(7)
    masks = {"all_valid_us": np.ones((B, J), np.uint8), "one_dirty_us": np.ones((B, J), np.uint8),
             "rows10_us": (rng.random((B, J)) >= 0.1).astype(np.uint8)}
    masks["one_dirty_us"][::10, J // 2] = 0
    ctx = vsom_amd.Context(W, H, J)
    ctx.upload_chunk(X)
    fns = {"epoch_us": lambda: ctx.batch_epoch(SIGMA, True)}
    for k, v in masks.items():
        fns[k] = (lambda v: lambda: ctx.batch_epoch_masked(SIGMA, True, v))(v)

    def timed(fn):
        ctx.set_state(map=init)
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    for _ in range(2):                                 # warm-up: code objects, scratch
        for fn in fns.values():
            timed(fn)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    res = {"shape": f"{W}x{H}x{J}", "rows": B, "rounds": rounds, "sigma": SIGMA, "valid_bytes": B * J}
    for k, v in ts.items():
        res[k] = float(np.median(v)) * 1e6
    e = np.array(ts["epoch_us"])
    res["epoch_spread"] = float((np.percentile(e, 90) - np.percentile(e, 10)) / np.median(e))
    for k in masks:
        res[k.replace("_us", "_over_epoch")] = res[k] / res["epoch_us"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_train_bench.jsonl"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("masked_train_bench.py needs a GPU")
    line = json.dumps(run(a.rows, a.rounds))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
