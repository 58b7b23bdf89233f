#!/usr/bin/env python3
"""vsom_bmu_topk_masked_batch beside the calls it extends, on one state.
One JSON line per (case, k) (appended to --out, profiles/topk_masked_bench.jsonl by default).  Cases, all on a 128 x 128 map
with 4096 rows, each for k = 2, 16, 64:
  allvalid   J = 784, a per-row mask with every entry valid (the price of the mask machinery alone)
  rows10     J = 784, 10 % of the entries invalid (a per-row mask)
  labels10   J = 794, a column mask over the last 10 columns (the one-hot labels)
Per round, one call of each in turn, every one ending in the library's own stream synchronise:
  topk_masked_us        Context.bmu_topk_masked(k): idx, dist, count, nvalid
  topk_masked_blend_us  the same with blend
  topk_us               Context.bmu_topk(k) of the same build on the same rows: the unmasked walk
  bmu_masked_us         Context.bmu_masked(): the same masked tile under the search's epilogue (one key per row)
  topk_parent_us        vsom_bmu_topk_batch of --lib (a build of the parent commit), bound with plain ctypes; absent without --lib
and the ratios x_topk (topk_masked / topk), x_bmu_masked (topk_masked / bmu_masked), x_blend (topk_masked_blend / topk_masked).
In a second pass, so that the events do not sit in the wall times, the library's HIP-event timers of the call with blend:
  topk_masked_dev_us (group "bmu": pack, tile, merge) and blend_dev_us (group "finish": the blend kernel)
Every case is warmed up first; every figure is the median over --rounds rounds with the 10th and 90th percentile beside it
(*_p10, *_p90).  Before anything is timed the masked call is checked: with the all-valid mask against bmu_topk bit for bit,
its column 0 against bmu_masked.

usage: tools/topk_masked_bench.py [--lib FILE] [--tag TEXT] [--rounds 20] [--cases a,b] [--ks 2,16,64] [--out FILE]"""
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

CASES = {   # name: (W, H, J, rows, mask)
    "allvalid": (128, 128, 784, 4096, "all"),
    "rows10": (128, 128, 784, 4096, "rows"),
    "labels10": (128, 128, 794, 4096, "column"),
    "tiny": (12, 10, 37, 70, "rows"),       # a rehearsal size: overheads only
}
MIN_HITS = 0        # every node a candidate, as in the unmasked call beside it


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def put(res, key, ts):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in stats_us(ts))


def state(W, H, J, rows, mask, seed=42):
    """a map in (0, 1), rows near units, the mask, and zeros at the invalid positions (what a loader delivers for NULL)"""
    rs = np.random.RandomState(seed)
    N = W * H
    m = (gen.random_map(N, J, seed=seed) * np.float32(0.45) + np.float32(0.5)).astype(np.float32)
    X = np.clip(m[rs.randint(0, N, rows)] + rs.randn(rows, J).astype(np.float32) * np.float32(0.05), 0, 1).astype(np.float32)
    if mask == "column":
        valid = np.ones(J, np.uint8)
        valid[J - 10:] = 0
    elif mask == "rows":
        valid = (rs.rand(rows, J) >= 0.1).astype(np.uint8)
    else:
        valid = np.ones((rows, J), np.uint8)
    X = np.where(valid != 0, X, np.float32(0)).astype(np.float32)
    return m, X, valid


def bind_parent(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_bmu_topk_batch.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, u64p, fp]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    return L


def run(name, ks, rounds, lib_path):
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    import vsom_amd
    W, H, J, rows, mask = CASES[name]
    m, X, valid = state(W, H, J, rows, mask)
    ctx = vsom_amd.Context(W, H, J, 0)
    ctx.set_state(map=m)
    ctx.upload_chunk(X)
    L = h = None
    if lib_path:
        L = bind_parent(lib_path)
        fp, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64)

        def ok(rc):
            if rc:
                raise RuntimeError(L.vsom_last_error().decode())

        h = C.c_void_p()
        ok(L.vsom_create(C.byref(h), 0, W, H, J, 0))
        ok(L.vsom_set_state(h, m.ctypes.data_as(fp), None, None, None, None))
        ok(L.vsom_upload_chunk(h, X.ctypes.data_as(fp), rows))
    out = []
    for k in ks:
        k = min(k, W * H)
        routes = {
            "topk_masked": lambda: ctx.bmu_topk_masked(k, valid, min_hits=MIN_HITS),
            "topk_masked_blend": lambda: ctx.bmu_topk_masked(k, valid, min_hits=MIN_HITS, blend=True),
            "topk": lambda: ctx.bmu_topk(k),
            "bmu_masked": lambda: ctx.bmu_masked(valid, min_hits=MIN_HITS),
        }
        if h is not None:
            pidx, pdist = np.empty((rows, k), np.uint64), np.empty((rows, k), np.float32)
            routes["topk_parent"] = lambda: ok(L.vsom_bmu_topk_batch(h, k, 0, rows, pidx.ctypes.data_as(u64p),
                                                                     pdist.ctypes.data_as(fp)))
        for _ in range(2):
            for fn in routes.values():
                fn()
        got, (ti, td), bm = routes["topk_masked_blend"](), routes["topk"](), routes["bmu_masked"]()
        assert (got["count"] == k).all() and (got["idx"][:, 0] == bm["bmu"]).all()
        assert (got["dist"][:, 0].view(np.uint32) == bm["dist"].view(np.uint32)).all()
        if mask == "all":
            assert (got["idx"] == ti).all() and (got["dist"].view(np.uint32) == td.view(np.uint32)).all()
        if h is not None:
            assert (pidx == ti).all() and (pdist.view(np.uint32) == td.view(np.uint32)).all()
        ts = {key: [] for key in routes}
        for _ in range(rounds):
            for key, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ts[key].append(time.perf_counter() - t0)
        res = {"case": name, "shape": f"{W}x{H}x{J}", "rows": rows, "k": k, "mask": mask, "min_hits": MIN_HITS,
               "invalid_fraction": round(1.0 - float(np.broadcast_to(valid, (rows, J)).mean()), 4), "rounds": rounds,
               "parent_lib": "given" if lib_path else "none"}
        for key in routes:
            put(res, key, ts[key])
        res["x_topk"] = round(res["topk_masked_us"] / res["topk_us"], 3)
        res["x_bmu_masked"] = round(res["topk_masked_us"] / res["bmu_masked_us"], 3)
        res["x_blend"] = round(res["topk_masked_blend_us"] / res["topk_masked_us"], 3)
        if h is not None:
            res["x_topk_parent"] = round(res["topk_us"] / res["topk_parent_us"], 3)
        ctx.enable_timing(True, groups=["bmu", "finish"])
        ctx.get_timing(reset=True)
        tb, tf = [], []
        for _ in range(rounds):
            routes["topk_masked_blend"]()
            t = ctx.get_timing(reset=True)
            tb.append(t["bmu"][0] * 1e-3)
            tf.append(t["finish"][0] * 1e-3)
        put(res, "topk_masked_dev", tb)
        put(res, "blend_dev", tf)
        ctx.enable_timing(False)
        out.append(res)
    if h is not None:
        L.vsom_destroy(h)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="", help="libvsom_hip.so of a build of the parent commit, for topk_parent_us")
    ap.add_argument("--tag", default="")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--cases", default="allvalid,rows10,labels10")
    ap.add_argument("--ks", default="2,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_masked_bench.jsonl"))
    a = ap.parse_args()
    ks = [int(v) for v in a.ks.split(",")]
    for name in a.cases.split(","):
        for res in run(name, ks, a.rounds, a.lib):
            if a.tag:
                res["tag"] = a.tag
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
