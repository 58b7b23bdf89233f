#!/usr/bin/env python3
"""vsom_bmd_masked_batch / vsom_generate_masked_batch beside the calls they extend, on one state.
One JSON line per case (appended to --out, profiles/bmd_masked_bench.jsonl by default).  Cases, all on a 128 x 128 map with
4096 rows:
  allvalid   J = 784, a per-row mask with every entry valid (the price of the mask machinery alone)
  rows10     J = 784, 10 % of the entries invalid (a per-row mask)
  labels10   J = 794, a column mask over the last 10 columns (the one-hot labels)
Per round, one call of each in turn, every one ending in the library's own stream synchronise:
  bmd_masked_us        Context.restricted_bmd_masked(u): norm and draw, no prob
  bmd_us               Context.restricted_bmd(u) of the same build on the same rows: the unmasked tile under the same epilogue
  bmd_parent_us        vsom_bmd_batch of --lib (a build of the parent commit), bound with plain ctypes; absent without --lib
  bmu_masked_us        Context.bmu_masked(): the same masked tile under the search's epilogue
  generate_masked1_us  Context.generate_masked(draws = 1)       generate_masked16_us  ... (draws = 16)
  generate_us          Context.generate(GENERATE_PER_ROW): one record per row, nothing kept
and in a second pass, so that the events do not sit in the wall times, the library's HIP-event timers of the masked calls:
  bmd_masked_dev_us    group "bmu" of restricted_bmd_masked (pack, tile, row pass)
  generate_masked16_draw_us / _decode_us   groups "bmu" / "finish" of generate_masked(draws = 16)
Every case is warmed up first; every figure is the median over --rounds rounds with the 10th and 90th percentile beside it
(*_p10, *_p90).  Before anything is timed the masked calls are checked: with the all-valid mask against the unmasked ones bit
for bit, and generate_masked's units against restricted_bmd_masked's draws.

usage: tools/bmd_masked_bench.py [--lib FILE] [--tag TEXT] [--rounds 20] [--cases a,b] [--out FILE]"""
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
MIN_HITS = 1
DRAWS = 16


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def put(res, key, ts):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in stats_us(ts))


def state(W, H, J, rows, mask, seed=42):
    """a map in (0, 1), a sigmaMap of a few percent, hit counts of which a third are 0, rows near units that qualify (every row
    has mass), the mask, and zeros at the invalid positions (what a loader delivers for NULL)"""
    rs = np.random.RandomState(seed)
    N = W * H
    m = (gen.random_map(N, J, seed=seed) * np.float32(0.45) + np.float32(0.5)).astype(np.float32)
    s = (rs.rand(N, J) * 0.05).astype(np.float32)
    hits = rs.randint(0, 3, N).astype(np.uint64)
    near = np.flatnonzero(hits >= MIN_HITS)[rs.randint(0, int((hits >= MIN_HITS).sum()), rows)]   # units that qualify
    X = np.clip(m[near] + rs.randn(rows, J).astype(np.float32) * np.float32(0.05), 0, 1).astype(np.float32)
    if mask == "column":
        valid = np.ones(J, np.uint8)
        valid[J - 10:] = 0
    elif mask == "rows":
        valid = (rs.rand(rows, J) >= 0.1).astype(np.uint8)
    else:
        valid = np.ones((rows, J), np.uint8)
    X = np.where(valid != 0, X, np.float32(0)).astype(np.float32)
    return m, s, hits, X, valid


def bind_parent(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    vp, fp, u64p, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_bmd_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, dp, u64p, dp, dp]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    return L


def run(name, rounds, lib_path):
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    import vsom_amd
    from vsom_amd import capi
    W, H, J, rows, mask = CASES[name]
    m, s, hits, X, valid = state(W, H, J, rows, mask)
    ctx = vsom_amd.Context(W, H, J, 0)
    ctx.set_state(map=m, sigma=s, hits=hits)
    ctx.upload_chunk(X)
    rs = np.random.RandomState(7)
    u1, uK = rs.rand(rows), rs.rand(rows, DRAWS)
    l1 = rs.randint(1, 1000, (rows, J)).astype(np.float64) / 1000.0
    lK = rs.randint(1, 1000, (rows, DRAWS, J)).astype(np.float64) / 1000.0

    routes = {
        "bmd_masked": lambda: ctx.restricted_bmd_masked(valid, MIN_HITS, u=u1),
        "bmd": lambda: ctx.restricted_bmd(MIN_HITS, u=u1),
        "bmu_masked": lambda: ctx.bmu_masked(valid, min_hits=MIN_HITS),
        "generate_masked1": lambda: ctx.generate_masked(valid, MIN_HITS, u1, l1),
        "generate_masked16": lambda: ctx.generate_masked(valid, MIN_HITS, uK, lK, draws=DRAWS),
        "generate": lambda: ctx.generate(MIN_HITS, u1, l1, capi.GENERATE_PER_ROW),
    }
    h = None
    if lib_path:
        L = bind_parent(lib_path)
        fp, u64p, dp = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_double)

        def ok(rc):
            if rc:
                raise RuntimeError(L.vsom_last_error().decode())

        h = C.c_void_p()
        ok(L.vsom_create(C.byref(h), 0, W, H, J, 0))
        ok(L.vsom_set_state(h, m.ctypes.data_as(fp), s.ctypes.data_as(fp), None, None, hits.ctypes.data_as(u64p)))
        ok(L.vsom_upload_chunk(h, X.ctypes.data_as(fp), rows))
        pnorm, pdraw = np.empty(rows), np.empty(rows, np.uint64)
        routes["bmd_parent"] = lambda: ok(L.vsom_bmd_batch(h, MIN_HITS, 0, rows, u1.ctypes.data_as(dp), pdraw.ctypes.data_as(u64p),
                                                          pnorm.ctypes.data_as(dp), None))

    for _ in range(2):
        for fn in routes.values():
            fn()
    got, plain = routes["bmd_masked"](), routes["bmd"]()
    assert (got["norm"] > 0).all() and (got["draw"] != capi.NO_UNIT).all()
    g1, gK = routes["generate_masked1"](), routes["generate_masked16"]()
    assert (g1["unit"][:, 0] == got["draw"]).all()
    assert (gK["unit"][:, 3] == ctx.restricted_bmd_masked(valid, MIN_HITS, u=np.ascontiguousarray(uK[:, 3]))["draw"]).all()
    if mask == "all":
        assert (got["norm"].view(np.uint64) == plain["norm"].view(np.uint64)).all() and (got["draw"] == plain["draw"]).all()
    if h is not None:
        routes["bmd_parent"]()
        assert (pnorm.view(np.uint64) == plain["norm"].view(np.uint64)).all() and (pdraw == plain["draw"]).all()

    ts = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    res = {"case": name, "shape": f"{W}x{H}x{J}", "rows": rows, "mask": mask, "min_hits": MIN_HITS,
           "invalid_fraction": round(1.0 - float(np.broadcast_to(valid, (rows, J)).mean()), 4), "rounds": rounds,
           "parent_lib": "given" if lib_path else "none"}
    for k in routes:
        put(res, k, ts[k])
    ctx.enable_timing(True, groups=["bmu", "finish"])
    for key, call in (("bmd_masked", "bmd_masked"), ("generate_masked16", "generate_masked16")):
        ctx.get_timing(reset=True)
        tb, tf = [], []
        for _ in range(rounds):
            routes[call]()
            t = ctx.get_timing(reset=True)
            tb.append(t["bmu"][0] * 1e-3)
            tf.append(t["finish"][0] * 1e-3)
        if key == "bmd_masked":
            put(res, "bmd_masked_dev", tb)
        else:
            put(res, "generate_masked16_draw", tb)
            put(res, "generate_masked16_decode", tf)
    ctx.enable_timing(False)
    if h is not None:
        L.vsom_destroy(h)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="", help="libvsom_hip.so of a build of the parent commit, for bmd_parent_us")
    ap.add_argument("--tag", default="")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--cases", default="allvalid,rows10,labels10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bmd_masked_bench.jsonl"))
    a = ap.parse_args()
    for name in a.cases.split(","):
        res = run(name, a.rounds, a.lib)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
