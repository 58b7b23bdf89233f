#!/usr/bin/env python3
"""findRestrictedBmd for a whole chunk: one vsom_bmd_batch call against the per-row loop it replaces.  One JSON line per
shape (appended to --out, profiles/bmd_bench.jsonl by default):

  loop_us        per row: vsom_distances_single, then numpy exp / mask / cumsum / the draw (the host round trip per row
                 that Som::findRestrictedBmd and Som::variationalAutoEncoder make)
  bmd_us         one vsom_bmd_batch call: norm + one draw per row, no probabilities
  bmd_prob_us    the same with the row-major probabilities copied back as well
  exact_bmu_us   vsom_bmu_batch with vsom_set_bmu_mode(VSOM_BMU_EXACT) on the same chunk (the same distance work)
  loop_over_bmd, bmd_over_exact

Every shape is warmed up first; each column is the median wall time of --calls calls, each ending in a synchronise.
The map holds hits from one batch epoch on the chunk (min_hits = 1 masks the nodes without any).  Kernel times come from
a separate `rocprofv3 --kernel-trace --stats` run of this script.

usage: tools/bmd_bench.py [--calls 20] [--shapes small,mid,c3] [--out FILE]"""
import argparse
import ctypes as C
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

SHAPES = {   # name: (W, H, J, rows)
    "small": (10, 10, 9, 20),
    "mid": (100, 100, 100, 1000),
    "c3": (128, 128, 784, 4096),
}


def median_us(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def run(name, calls):
    W, H, J, B = SHAPES[name]
    N = W * H
    L = capi.lib()
    X = gen.mnist_like(B, seed=3, dim=J) if J == 784 else gen.blobs(B, J, 8, 1, 2, sigma=0.3)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=gen.random_map(N, J, seed=42))
    ctx.upload_chunk(X)
    ctx.batch_epoch(max(W, H) / 2.0, True)        # hits of one epoch
    ctx.set_bmu_mode(capi.BMU_EXACT)
    h = ctx._h
    hits = ctx.get_state(map=False, sigma=False, S=False, weight=False)["hits"]
    elig = hits >= np.uint64(1)
    u = np.random.default_rng(1).random(B)
    dp, fp, u64p = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    up = u.ctypes.data_as(dp)
    norm, draw = np.empty(B), np.empty(B, np.uint64)
    prob = np.empty((B, N))
    normp, drawp, probp = norm.ctypes.data_as(dp), draw.ctypes.data_as(u64p), prob.ctypes.data_as(dp)
    idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
    idxp, distp = idx.ctypes.data_as(u64p), dist.ctypes.data_as(fp)
    d = np.empty(N, np.float32)
    dptr = d.ctypes.data_as(fp)
    rows = [np.ascontiguousarray(X[r]) for r in range(B)]
    rowp = [r.ctypes.data_as(fp) for r in rows]
    loop_draw = np.empty(B, np.uint64)

    def loop():
        for r in range(B):
            capi.check(L.vsom_distances_single(h, rowp[r], dptr))
            dd = d.astype(np.float64)
            p = np.where(elig, np.exp(-dd * dd / 2), 0.0)
            cum = np.cumsum(p)
            c = cum[-1]
            if c > 0 and np.isfinite(c):
                i = int(np.searchsorted(cum, u[r] * c, side="right"))
                loop_draw[r] = i if i < N else np.nonzero(p > 0)[0][-1]
            else:
                loop_draw[r] = np.uint64(0xFFFFFFFFFFFFFFFF)

    def bmd():
        capi.check(L.vsom_bmd_batch(h, 1, 0, B, up, drawp, normp, None))

    def bmd_prob():
        capi.check(L.vsom_bmd_batch(h, 1, 0, B, up, drawp, normp, probp))

    def exact():
        capi.check(L.vsom_bmu_batch(h, idxp, distp))

    for fn in (loop, bmd, bmd_prob, exact):     # warm-up: code objects, scratch
        fn()
    same = int((loop_draw == draw).sum())
    res = {"shape": f"{W}x{H}x{J}", "rows": B, "calls": calls,
           "loop_us": median_us(loop, calls),
           "bmd_us": median_us(bmd, calls), "bmd_prob_us": median_us(bmd_prob, calls),
           "exact_bmu_us": median_us(exact, calls), "loop_draws_equal": same}
    res["loop_over_bmd"] = res["loop_us"] / res["bmd_us"]
    res["bmd_over_exact"] = res["bmd_us"] / res["exact_bmu_us"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="small,mid,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bmd_bench.jsonl"))
    a = ap.parse_args()
    for name in a.shapes.split(","):
        line = json.dumps(run(name, a.calls))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
