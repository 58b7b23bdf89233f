#!/usr/bin/env python3
"""The online chunk over valid entries beside the plain one: vsom_train_online_chunk_masked with three masks and
vsom_train_online_chunk forced onto the exact scan (vsom_set_bmu_mode), on the same state and rows in the same process.
One JSON line (appended to --out, profiles/online_masked_bench.jsonl by default):

  exact_us             microseconds per sample of one vsom_train_online_chunk_fetch call, exact scan
  all_valid_us         ... of one vsom_train_online_chunk_masked call with an all-valid per-row mask
  one_column_us        ... with one column invalid in every row (one_mask)
  entries10_us         ... with 10 % of all entries invalid at random
  all_valid_over_exact, one_column_over_exact, entries10_over_exact
  valid_bytes          validity bytes a per-row masked call uploads (rows x J)

128 x 128 x 784, sigma 8, a 1024-row chunk, Exponential.  Before every call the state is set back to the same initial
one (outside the timed span), so every call does the same work.  The calls are warmed up, then timed in rounds -- one call
of each kind per round, in turn, each a blocking call -- and each column is the median over --rounds rounds; the spread
column is (p90 - p10) / median of the exact chunk.  With --lib (another build of libvsom_hip.so, the parent commit's
for instance) that build is measured instead; the columns of calls it does not export are left out.

usage: tools/online_masked_bench.py [--rounds 9] [--rows 1024] [--lib LIB] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, J = 128, 128, 784
SIGMA, ETA = 8.0, 0.3


def run(rows, rounds):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen
    import vsom_amd
    from vsom_amd import capi

    if capi.device_count() < 1:
        raise SystemExit("online_masked_bench.py needs a GPU")
    N, B = W * H, rows
    X = gen.mnist_like(B, seed=3, dim=J)
    init = (gen.random_map(N, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    zeros = np.zeros((N, J), np.float32)
    rng = np.random.default_rng(7)
    one_column = np.ones(J, np.uint8)
    one_column[J // 2] = 0
    masks = {"all_valid_us": np.ones((B, J), np.uint8), "one_column_us": one_column,
             "entries10_us": (rng.random((B, J)) >= 0.1).astype(np.uint8)}
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_bmu_mode(capi.BMU_EXACT)
    ctx.upload_chunk(X)
    fns = {"exact_us": lambda: ctx.train_online_chunk_fetch(ETA, SIGMA, capi.EXPONENTIAL)}
    if hasattr(capi.lib(), "vsom_train_online_chunk_masked"):
        for k, v in masks.items():
            fns[k] = (lambda v: lambda: ctx.train_online_chunk_masked(ETA, SIGMA, capi.EXPONENTIAL, v))(v)

    def timed(fn):
        ctx.set_state(map=init, sigma=zeros, S=zeros, weight=np.zeros(N, np.float32))
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    for _ in range(2):                                 # warm-up: code objects, scratch, the neighbourhood table
        for fn in fns.values():
            timed(fn)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    res = {"shape": f"{W}x{H}x{J}", "rows": B, "rounds": rounds, "sigma": SIGMA, "decay": "exponential",
           "valid_bytes": B * J, "lib": os.path.relpath(capi.LIB_PATH, ROOT)}
    for k, v in ts.items():
        res[k] = float(np.median(v)) * 1e6 / B
    e = np.array(ts["exact_us"])
    res["exact_spread"] = float((np.percentile(e, 90) - np.percentile(e, 10)) / np.median(e))
    for k in masks:
        if k in res:
            res[k.replace("_us", "_over_exact")] = res[k] / res["exact_us"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--lib", default=None, help="another build of libvsom_hip.so to measure (the parent commit's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_masked_bench.jsonl"))
    a = ap.parse_args()
    if a.lib:
        os.environ["VSOM_LIB"] = os.path.abspath(a.lib)      # (a library is chosen when it is loaded)
    line = json.dumps(run(a.rows, a.rounds))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
