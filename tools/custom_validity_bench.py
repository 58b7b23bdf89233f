#!/usr/bin/env python3
"""One batch step (a local-search epoch) of a custom context with and without the chunk's validity set, beside the same step
of ANOTHER build of the library -- the parent commit's, --lib.  One JSON line (appended to --out,
profiles/custom_validity_bench.jsonl by default), per hook and case the median and the 10th / 90th percentile in microseconds:

  <hook>_parent_unset    the --lib build, setters never called (it has none)
  <hook>_unset           this build, setters never called: the launches pass the all-ones vector with stride 0
  <hook>_all_valid       vsom_set_chunk_validity with a B x J mask of ones: per-row value_weight arrays, stride J
  <hook>_ten_percent     10 % invalid entries
  *_over_parent          each median of this build as a ratio to <hook>_parent_unset

Hooks: "standard", the restated Standard source of tests/custom_hooks.py, which never reads value_weight, and "select", the
SELECT source of tests/custom_validity_hooks.py, which reads it in every hook call.  The shape is a reduced form of DESIGN
section 4b's timing line (128 x 128 x 784 x 4096 rows there; --width / --height / --rows here) so that a run stays short.
A library is chosen when it is loaded, so every (build, hook, case) runs in a worker process of its own: it warms up, then
times --epochs epochs (state and lastBMU set back before each, outside the timed span; vsom_batch_epoch blocks).  The
workers run one at a time, in rounds; the percentiles are over all epochs of all rounds.

usage: tools/custom_validity_bench.py --lib PARENT_LIB [--rounds 3] [--epochs 7] [--rows 2048] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 784
SIGMA = 8.0
HOOKS = ("standard", "select")
CASES = ("unset", "all_valid", "ten_percent")


def worker(hook, case, a):
    import torch  # noqa: F401  (first: libvsom_hip.so binds to the HIP runtime torch brings)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen
    import custom_hooks
    import custom_validity_hooks
    from vsom_amd import capi

    if capi.device_count() < 1:
        raise SystemExit("custom_validity_bench.py needs a GPU")
    W, H, B = a.width, a.height, a.rows
    X = gen.mnist_like(B, seed=3, dim=J)
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    source = custom_hooks.STANDARD if hook == "standard" else custom_validity_hooks.SELECT
    ctx = capi.Context(W, H, J, capi.CUSTOM, source=source, depth=J, residual_len=J)
    ctx.set_state(map=init)
    ctx.upload_chunk(X)
    if case == "all_valid":
        ctx.set_chunk_validity(np.ones((B, J), np.uint8))
    elif case == "ten_percent":
        ctx.set_chunk_validity(np.random.default_rng(1).random((B, J)) >= 0.1)
    ctx.batch_epoch(SIGMA, True)
    state, last = ctx.get_state(), ctx.get_last_bmu()

    def epoch():
        ctx.set_state(**state)
        ctx.set_last_bmu(last)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.batch_epoch(SIGMA, False)
        return time.perf_counter() - t0

    for _ in range(2):
        epoch()
    ts = [epoch() * 1e6 for _ in range(a.epochs)]
    ctx.close()
    print(json.dumps({"us": ts}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--lib", default=None, help="the parent commit's build of libvsom_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "custom_validity_bench.jsonl"))
    ap.add_argument("--worker", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1], a)
    if not a.lib:
        raise SystemExit("--lib: the parent commit's libvsom_hip.so is the yardstick")
    kinds = []
    for hook in HOOKS:
        kinds.append((f"{hook}_parent_unset", hook, "unset", os.path.abspath(a.lib)))
        kinds += [(f"{hook}_{case}", hook, case, None) for case in CASES]
    ts = {name: [] for name, _, _, _ in kinds}
    for _ in range(a.rounds):
        for name, hook, case, lib in kinds:
            env = dict(os.environ)
            env.pop("VSOM_LIB", None)
            if lib:
                env["VSOM_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", hook, case, "--rows", str(a.rows),
                                  "--width", str(a.width), "--height", str(a.height), "--epochs", str(a.epochs)],
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            ts[name] += json.loads(out.strip().splitlines()[-1])["us"]
    res = {"shape": f"{a.width}x{a.height}x{J}", "rows": a.rows, "rounds": a.rounds, "epochs": a.epochs, "sigma": SIGMA,
           "step": "vsom_batch_epoch, local search", "parent_lib": "given"}
    for name, v in ts.items():
        res[name + "_us"] = round(float(np.median(v)), 1)
        res[name + "_p10"] = round(float(np.percentile(v, 10)), 1)
        res[name + "_p90"] = round(float(np.percentile(v, 90)), 1)
    for hook in HOOKS:
        for case in CASES:
            res[f"{hook}_{case}_over_parent"] = round(res[f"{hook}_{case}_us"] / res[f"{hook}_parent_unset_us"], 4)
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
