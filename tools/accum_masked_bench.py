#!/usr/bin/env python3
"""Masked accumulated epochs (vsom_batch_accum_chunk_masked) beside plain accumulated epochs (vsom_batch_accum_chunk) of
ANOTHER build of the library -- the parent commit's, --lib -- on the same state and rows.  One JSON line (appended to --out,
profiles/accum_masked_bench.jsonl by default):

  parent_plain_us        begin + 4 x (upload of --rows rows + vsom_batch_accum_chunk) + end with the --lib build
  plain_us               the same calls with this build (the plain path must not have moved)
  all_valid_us           ... + vsom_batch_accum_chunk_masked with a B x J mask of ones: the masked search, no dirty column
  one_dirty_us           one column with an invalid entry in every chunk (one ever-dirty column)
  ten_percent_us         10 % invalid entries: every column is ever dirty
  *_over_parent          each of the four as a ratio to parent_plain_us

128 x 128 x 784 on gen.mnist_like rows, sigma 8, first epoch (the full search).  A library is chosen when it is loaded, so
every (build, case) pair runs in a worker process of its own: the worker warms up, then times --epochs epochs (the map set
back to the same initial state before each, outside the timed span; each epoch ends in the blocking end call) and reports
their median.  The workers run one at a time, in rounds -- one worker of each kind per round, in turn -- and each column is
the median over --rounds rounds.

usage: tools/accum_masked_bench.py --lib PARENT_LIB [--rounds 3] [--epochs 5] [--rows 4096] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, J = 128, 128, 784
SIGMA = 8.0
PARTS = 4
CASES = ("plain", "all_valid", "one_dirty", "ten_percent")


def masks(case, rows):
    if case == "plain":
        return [None] * PARTS
    out = []
    for k in range(PARTS):
        v = np.ones((rows, J), np.uint8)
        if case == "one_dirty":
            v[k::7, 300] = 0
        elif case == "ten_percent":
            v = (np.random.default_rng(k).random((rows, J)) >= 0.1).astype(np.uint8)
        out.append(v)
    return out


def worker(case, rows, epochs):
    import torch  # noqa: F401  (first: libvsom_hip.so binds to the HIP runtime torch brings)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen
    import vsom_amd
    from vsom_amd import capi

    if capi.device_count() < 1:
        raise SystemExit("accum_masked_bench.py needs a GPU")
    X = gen.mnist_like(PARTS * rows, seed=3, dim=J)
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    valid = masks(case, rows)
    ctx = vsom_amd.Context(W, H, J)

    def epoch():
        ctx.set_state(map=init)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.batch_accum_begin(SIGMA, True, PARTS * rows)
        for k in range(PARTS):
            ctx.upload_chunk(X[k * rows:(k + 1) * rows])
            if valid[k] is None:
                ctx.batch_accum_chunk()
            else:
                ctx.batch_accum_chunk_masked(valid[k])
        ctx.batch_accum_end()
        return time.perf_counter() - t0

    for _ in range(2):                                 # warm-up: code objects, scratch
        epoch()
    ts = [epoch() for _ in range(epochs)]
    ctx.close()
    print(json.dumps({"us": float(np.median(ts)) * 1e6}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--lib", default=None, help="the parent commit's build of libvsom_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_masked_bench.jsonl"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.environ["VSOM_SIGMA_MODE"] = "eager"            # read when a context is created
    if a.worker:
        return worker(a.worker, a.rows, a.epochs)
    if not a.lib:
        raise SystemExit("--lib: the parent commit's libvsom_hip.so is the yardstick")
    kinds = [("parent_plain", "plain", os.path.abspath(a.lib))] + [(c, c, None) for c in CASES]
    ts = {name: [] for name, _, _ in kinds}
    for _ in range(a.rounds):
        for name, case, lib in kinds:
            env = dict(os.environ)
            env.pop("VSOM_LIB", None)
            if lib:
                env["VSOM_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", case, "--rows", str(a.rows),
                                  "--epochs", str(a.epochs)], env=env, check=True, capture_output=True, text=True).stdout
            ts[name].append(json.loads(out.strip().splitlines()[-1])["us"])
    res = {"shape": f"{W}x{H}x{J}", "rows": a.rows, "parts": PARTS, "rounds": a.rounds, "epochs": a.epochs, "sigma": SIGMA,
           "parent_lib": os.path.relpath(os.path.abspath(a.lib), ROOT)}
    for name, v in ts.items():
        res[name + "_us"] = float(np.median(v))
    for c in CASES:
        res[c + "_over_parent"] = res[c + "_us"] / res["parent_plain_us"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
