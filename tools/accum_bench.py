#!/usr/bin/env python3
"""The accumulated batch epoch (vsom_batch_accum_begin / _chunk / _end) beside vsom_batch_epoch, on the same state and
rows in the same build; VSOM_SIGMA_MODE=eager throughout, so that the plain epoch runs both chains as the accumulated
one does.  One JSON line (appended to --out, profiles/accum_bench.jsonl by default):

  epoch_us               one vsom_batch_epoch call on the --rows chunk (first epoch: the full search), MSE fetched
  one_chunk_us           begin + chunk + end on the same chunk
  one_chunk_over_epoch
  giant_us               upload of 4 x --rows rows as ONE chunk + vsom_batch_epoch
  split_us               begin + 4 x (upload of --rows rows + chunk) + end on the same rows
  split_over_giant
  giant_peak_bytes, split_peak_bytes   device memory in use after the calls above, beyond what was in use before the context
                         was created (every buffer is grow-only: the figure after the calls is the peak); each measured in
                         a process phase of its own context
  share_bmu, share_cw, share_update, share_finish   of the chunk calls' device time (vsom_get_timing), one_chunk case

128 x 128 x 784 on gen.mnist_like rows.  Before every timed call the map is set back to the same initial state (outside the
timed span).  The calls are warmed up, then timed in rounds -- one call of each kind per round, in turn, each ending in a
blocking call -- and each column is the median over --rounds rounds.  With --lib naming a build without the accumulated
epoch (a parent commit's) only epoch_us and giant_us are reported.

usage: tools/accum_bench.py [--rounds 9] [--rows 4096] [--lib PATH] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, J = 128, 128, 784
SIGMA = 8.0
PARTS = 4


def in_use():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def run(rows, rounds):
    import torch  # noqa: F401  (first: libvsom_hip.so binds to the HIP runtime torch brings)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gen
    import vsom_amd
    from vsom_amd import capi

    if capi.device_count() < 1:
        raise SystemExit("accum_bench.py needs a GPU")
    have = hasattr(capi.lib(), "vsom_batch_accum_begin")
    N = W * H
    X = gen.mnist_like(PARTS * rows, seed=3, dim=J)
    init = (gen.random_map(N, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    res = {"shape": f"{W}x{H}x{J}", "rows": rows, "parts": PARTS, "rounds": rounds, "sigma": SIGMA,
           "lib": os.path.relpath(capi.LIB_PATH, ROOT)}

    def measure(fns, ctx):
        def timed(fn):
            ctx.set_state(map=init)
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0

        for _ in range(2):                             # warm-up: code objects, scratch
            for fn in fns.values():
                timed(fn)
        ts = {k: [] for k in fns}
        for _ in range(rounds):
            for k, fn in fns.items():
                ts[k].append(timed(fn))
        return {k: float(np.median(v)) * 1e6 for k, v in ts.items()}

    # ---- one chunk ----
    base = in_use()
    ctx = vsom_amd.Context(W, H, J)
    ctx.upload_chunk(X[:rows])

    def one_chunk():
        ctx.batch_accum_begin(SIGMA, True, rows)
        ctx.batch_accum_chunk()
        ctx.batch_accum_end()

    fns = {"epoch_us": lambda: ctx.batch_epoch(SIGMA, True)}
    if have:
        fns["one_chunk_us"] = one_chunk
    res.update(measure(fns, ctx))
    if have:
        res["one_chunk_over_epoch"] = res["one_chunk_us"] / res["epoch_us"]
        ctx.set_state(map=init)
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        for _ in range(3):
            ctx.batch_accum_begin(SIGMA, True, rows)
            ctx.batch_accum_chunk()
            ctx.batch_accum_abort()
        t = ctx.get_timing(reset=True)
        ctx.enable_timing(False)
        tot = sum(t[k][0] for k in ("bmu", "cw", "update", "finish"))
        for k in ("bmu", "cw", "update", "finish"):
            res["share_" + k] = t[k][0] / tot if tot > 0 else 0.0
    ctx.close()

    # ---- four chunks accumulated / one giant chunk ----
    def giant_fn(c):
        def fn():
            c.upload_chunk(X)
            c.batch_epoch(SIGMA, True)
        return fn

    def split_fn(c):
        def fn():
            c.batch_accum_begin(SIGMA, True, PARTS * rows)
            for k in range(PARTS):
                c.upload_chunk(X[k * rows:(k + 1) * rows])
                c.batch_accum_chunk()
            c.batch_accum_end()
        return fn

    # peaks first, each on a fresh context; then the interleaved rounds on two contexts that live side by side
    for name, make in (("giant", giant_fn), ("split", split_fn)):
        if name == "split" and not have:
            continue
        c = vsom_amd.Context(W, H, J)
        c.set_state(map=init)
        make(c)()
        c.synchronize()
        res[name + "_peak_bytes"] = int(in_use() - base)
        c.close()
    cg = vsom_amd.Context(W, H, J)
    fns = {"giant_us": giant_fn(cg)}
    cs = None
    if have:
        cs = vsom_amd.Context(W, H, J)
        fns["split_us"] = split_fn(cs)

    def timed2(k, fn):
        c = cg if k == "giant_us" else cs
        c.set_state(map=init)
        c.synchronize()
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0

    for _ in range(2):
        for k, fn in fns.items():
            timed2(k, fn)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed2(k, fn))
    for k, v in ts.items():
        res[k] = float(np.median(v)) * 1e6
    if have:
        res["split_over_giant"] = res["split_us"] / res["giant_us"]
        cs.close()
    cg.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--lib", default=None, help="another build of libvsom_hip.so (a parent commit's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_bench.jsonl"))
    a = ap.parse_args()
    if a.lib:
        os.environ["VSOM_LIB"] = os.path.abspath(a.lib)
    os.environ["VSOM_SIGMA_MODE"] = "eager"           # read when a context is created
    line = json.dumps(run(a.rows, a.rounds))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
