#!/usr/bin/env python3
"""The search over valid columns of a whole chunk: one vsom_bmu_masked_batch call beside the two existing calls that run
the same exact-order distance tile without a mask, on the same state and rows in the same build.  One JSON line per case
(appended to --out, profiles/masked_bench.jsonl by default):

  masked_us        one vsom_bmu_masked_batch call over every row; bmu, dist and nvalid copied back
  masked_fill_us   the same with the imputed rows (rows x J floats) copied back too
  topk1_us         vsom_bmu_topk_batch(k = 1): idx and dist copied back
  exact_bmu_us     vsom_bmu_batch with vsom_set_bmu_mode(VSOM_BMU_EXACT): idx and dist copied back
  masked_over_topk1, masked_over_exact
  valid_bytes      validity bytes the call uploads (rows x J, or J for a column mask)

Cases: "rows10" 128 x 128 x 784, 4096 rows, a random per-row mask with 10 % invalid; "labels" 128 x 128 x 794, 4096 rows,
a column mask over the last 10 columns (the classification case).

Every case is warmed up first.  The calls are timed in rounds -- one call of each kind per round, in turn, each ending in
a synchronise -- and each column is the median over --rounds rounds; the spread column is (p90 - p10) / median of the
masked call.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--rounds 3).

usage: tools/masked_bench.py [--rounds 30] [--cases rows10,labels] [--rows 4096] [--out FILE]"""
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

CASES = {   # name: (W, H, J, label columns)
    "rows10": (128, 128, 784, 0),
    "labels": (128, 128, 794, 10),
}


def run(name, rows, rounds):
    W, H, J, nlab = CASES[name]
    N, B = W * H, rows
    L = capi.lib()
    X = gen.mnist_like(B, seed=3, dim=784)
    if nlab:
        X = np.concatenate([X, np.eye(nlab, dtype=np.float32)[np.arange(B) % nlab]], axis=1)
    rng = np.random.default_rng(7)
    if nlab:
        valid = np.ones(J, np.uint8)
        valid[J - nlab:] = 0
    else:
        valid = (rng.random((B, J)) >= 0.1).astype(np.uint8)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=(gen.random_map(N, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32),
                  hits=np.ones(N, np.uint64))
    ctx.upload_chunk(X)
    ctx.set_bmu_mode(capi.BMU_EXACT)
    h = ctx._h
    fp, u64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
    tki, tkd = np.empty((B, 1), np.uint64), np.empty((B, 1), np.float32)
    mb, md, mn = np.empty(B, np.uint64), np.empty(B, np.float32), np.empty(B, np.uint32)
    mf = np.empty((B, J), np.float32)
    out, outf = capi.MaskedOut(), capi.MaskedOut()
    for o in (out, outf):
        o.bmu, o.dist, o.nvalid = mb.ctypes.data_as(u64p), md.ctypes.data_as(fp), mn.ctypes.data_as(C.POINTER(C.c_uint32))
    outf.fill = mf.ctypes.data_as(fp)
    vptr, one = valid.ctypes.data_as(u8p), int(valid.ndim == 1)

    fns = {
        "masked_us": lambda: capi.check(L.vsom_bmu_masked_batch(h, 0, 0, B, vptr, one, C.byref(out))),
        "masked_fill_us": lambda: capi.check(L.vsom_bmu_masked_batch(h, 0, 0, B, vptr, one, C.byref(outf))),
        "topk1_us": lambda: capi.check(L.vsom_bmu_topk_batch(h, 1, 0, B, tki.ctypes.data_as(u64p), tkd.ctypes.data_as(fp))),
        "exact_bmu_us": lambda: capi.check(L.vsom_bmu_batch(h, idx.ctypes.data_as(u64p), dist.ctypes.data_as(fp))),
    }
    for _ in range(3):                                 # warm-up: code objects, scratch
        for fn in fns.values():
            fn()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    res = {"case": name, "shape": f"{W}x{H}x{J}", "rows": B, "rounds": rounds, "valid_bytes": int(valid.size),
           "invalid_share": float(1.0 - valid.mean())}
    for k, v in ts.items():
        res[k] = float(np.median(v)) * 1e6
    m = np.array(ts["masked_us"])
    res["masked_spread"] = float((np.percentile(m, 90) - np.percentile(m, 10)) / np.median(m))
    res["masked_over_topk1"] = res["masked_us"] / res["topk1_us"]
    res["masked_over_exact"] = res["masked_us"] / res["exact_bmu_us"]
    # what the calls return on this state: how many rows the mask moves to another unit
    res["rows_moved_by_mask"] = int((mb != idx).sum())
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--cases", default="rows10,labels")
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_bench.jsonl"))
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("masked_bench.py needs a GPU")
    for name in a.cases.split(","):
        line = json.dumps(run(name, a.rows, a.rounds))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
