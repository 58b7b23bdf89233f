#!/usr/bin/env python3
"""The k best matching units of a whole chunk: one vsom_bmu_topk_batch call against the exact BMU search and the per-row
loop it replaces.  One JSON line per shape (appended to --out, profiles/topk_bench.jsonl by default):

  topk{k}_us     one vsom_bmu_topk_batch call over every row, idx and dist copied back, for k = 1, 2, 16, 64
  exact_bmu_us   vsom_bmu_batch with vsom_set_bmu_mode(VSOM_BMU_EXACT) on the same chunk (the same distance work)
  rowloop_us     per row: vsom_distances_row, then np.argpartition + sort of the k = 2 smallest (the host round trip a
                 caller makes without this call); at c3 timed on --loop-rows rows and scaled to the chunk
  topk2_over_exact, topk64_over_exact, rowloop_over_topk2, rowloop_over_topk64

Every shape is warmed up first; each column is the median wall time of --calls calls, each ending in a synchronise.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.

usage: tools/topk_bench.py [--calls 20] [--shapes small,mid,c3] [--loop-rows 1000] [--out FILE]"""
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
KS = (1, 2, 16, 64)


def median_us(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def run(name, calls, loop_rows):
    W, H, J, B = SHAPES[name]
    N = W * H
    L = capi.lib()
    X = gen.mnist_like(B, seed=3, dim=J) if J == 784 else gen.blobs(B, J, 8, 1, 2, sigma=0.3)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=gen.random_map(N, J, seed=42))
    ctx.upload_chunk(X)
    ctx.set_bmu_mode(capi.BMU_EXACT)
    h = ctx._h
    fp, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
    idxp, distp = idx.ctypes.data_as(u64p), dist.ctypes.data_as(fp)
    tk = {k: (np.empty((B, k), np.uint64), np.empty((B, k), np.float32)) for k in KS if k <= N}
    d = np.empty(N, np.float32)
    dptr = d.ctypes.data_as(fp)
    nloop = B if B <= loop_rows else loop_rows
    loop_idx = np.empty((nloop, 2), np.uint64)

    def topk(k):
        i, dd = tk[k]
        return lambda: capi.check(L.vsom_bmu_topk_batch(h, k, 0, B, i.ctypes.data_as(u64p), dd.ctypes.data_as(fp)))

    def exact():
        capi.check(L.vsom_bmu_batch(h, idxp, distp))

    def loop():
        for r in range(nloop):
            capi.check(L.vsom_distances_row(h, r, dptr))
            part = np.argpartition(d, 1)[:2]
            loop_idx[r] = part[np.lexsort((part, d[part]))]

    fns = {k: topk(k) for k in tk}
    for fn in list(fns.values()) + [exact, loop]:     # warm-up: code objects, scratch
        fn()
    same = int((loop_idx == tk[2][0][:nloop]).all(axis=1).sum())
    res = {"shape": f"{W}x{H}x{J}", "rows": B, "calls": calls}
    for k, fn in fns.items():
        res[f"topk{k}_us"] = median_us(fn, calls)
    res["exact_bmu_us"] = median_us(exact, calls)
    res["rowloop_rows"] = nloop
    res["rowloop_us"] = median_us(loop, max(1, min(calls, 5))) * B / nloop
    res["rowloop_top2_equal"] = same
    res["topk2_over_exact"] = res["topk2_us"] / res["exact_bmu_us"]
    if "topk64_us" in res:
        res["topk64_over_exact"] = res["topk64_us"] / res["exact_bmu_us"]
        res["rowloop_over_topk64"] = res["rowloop_us"] / res["topk64_us"]
    res["rowloop_over_topk2"] = res["rowloop_us"] / res["topk2_us"]
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="small,mid,c3")
    ap.add_argument("--loop-rows", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_bench.jsonl"))
    a = ap.parse_args()
    for name in a.shapes.split(","):
        line = json.dumps(run(name, a.calls, a.loop_rows))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
