#!/usr/bin/env python3
"""vsom_similarity_masked_batch / vsom_evaluate_masked_batch against the routes they replace, on one state.
One JSON line per (case, call) (appended to --out, profiles/masked_score_bench.jsonl by default).  Cases, both on a
128 x 128 map:
  rows10     J = 784, 4096 rows, 10 % of the entries invalid (a per-row mask)
  labels10   J = 794, 4096 rows, a column mask over the last 10 columns (the one-hot labels)
Per round, one call of each in turn, every one ending in the library's own stream synchronise:
  new_us       Context.similarity_masked() / Context.evaluate_masked()
  parent_us    what a caller could do before, through symbols the parent commit has, bound with plain ctypes on --lib (a
               build of the parent commit; the library of this tree when none is given -- `parent_lib` says which):
               vsom_bmu_masked_batch, vsom_get_state of map and sigmaMap (evaluate: of map; one vsom_set_state of hits
               between the rounds, outside the timed region, stands for the training step that dirtied a host mirror),
               and the rows x J epilogue in numpy
  unmasked_us  vsom_similarity_batch(min_hits = 1) / vsom_evaluate_batch with valid_host: the search that takes a missing
               field for a measured zero (other units: the price of the masked tile, not the same result)
and in a second pass, so that the events do not sit in the wall times, the library's HIP-event timers of the new call:
  search_us    group "bmu" (validity upload, pack, tile walk, reduction), scoring_us  group "finish" (the scoring kernel)
Every case is warmed up first; every figure is the median over --rounds rounds with the 10th and 90th percentile beside
it (*_p10, *_p90).  The new call's units are checked against the parent route's before anything is timed.

usage: tools/masked_score_bench.py [--lib FILE] [--tag TEXT] [--rounds 30] [--cases a,b] [--out FILE]"""
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

CASES = {   # name: (W, H, J, rows, column mask?)
    "rows10": (128, 128, 784, 4096, False),
    "labels10": (128, 128, 794, 4096, True),
    "tiny": (12, 10, 37, 70, False),        # a rehearsal size: overheads only
}
NUM_SIGMAS = 3
MIN_HITS = 1


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def put(res, key, ts):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in stats_us(ts))


def state(W, H, J, rows, one, seed=42):
    """a map in (0, 1), a sigmaMap around the 1e-5 select, hit counts of which a third are 0, rows near the map, the mask,
    and zeros at the invalid positions (what a loader delivers for NULL)"""
    rs = np.random.RandomState(seed)
    N = W * H
    m = (gen.random_map(N, J, seed=seed) * np.float32(0.45) + np.float32(0.5)).astype(np.float32)
    s = (rs.rand(N, J) * 2e-5).astype(np.float32)
    hits = rs.randint(0, 3, N).astype(np.uint64)
    X = np.clip(m[rs.randint(0, N, rows)] + rs.randn(rows, J).astype(np.float32) * np.float32(0.05), 0, 1).astype(np.float32)
    if one:
        valid = np.ones(J, np.uint8)
        valid[J - 10:] = 0
    else:
        valid = (rs.rand(rows, J) >= 0.1).astype(np.uint8)
    X = np.where(valid != 0, X, np.float32(0)).astype(np.float32)
    binary = np.zeros(J, np.float32)
    binary[::8] = 1                                    # every eighth column binary
    return m, s, hits, X, valid, binary, np.ones(J, np.float32)


def similarity_epilogue(X, m, s, bmu, valid, k):
    """the rows x J walk of Som::measureSimilarity over the valid columns, vectorised"""
    b = bmu.astype(np.int64)
    mm, ss = m[b], s[b]
    v = np.broadcast_to(valid != 0, X.shape)
    with np.errstate(all="ignore"):
        sM = np.where(ss > np.float32(1e-5), np.float32(1e-5), ss)
        delta = np.where(v, (X - mm) / sM / np.float32(k), np.float32(np.nan))
        sk = sM * np.float32(k)
        outside = (v & ((X < mm - sk) | (X > mm + sk))).sum(axis=1)
        dmax = np.nanmax(np.where(v.any(axis=1)[:, None], delta, np.float32(-np.inf)), axis=1)
    return int(np.argmax(dmax)), outside


def evaluate_epilogue(X, m, bmu, dist, valid, binary, continuous):
    """the rows x J walk of Som::evaluate over the valid columns, vectorised, and its running mean"""
    mm = m[bmu.astype(np.int64)]
    cols = np.flatnonzero((binary != 0) & (continuous != 0))
    v = np.broadcast_to(valid != 0, X.shape)[:, cols]
    x, mc = X[:, cols], mm[:, cols]
    with np.errstate(all="ignore"):
        be = np.log(mc) * x + np.log(np.float32(1) - mc) * (np.float32(1) - x)
        be = np.where(np.isfinite(be), be, np.float32(-99999.0))
        t = np.where(v, be * binary[cols] * continuous[cols], np.float32(0))
        bsum = (t * t).sum(axis=1, dtype=np.float32)
    per_row = dist.astype(np.float64) + np.sqrt(bsum.astype(np.float64))
    err = 0.0
    for i, e in enumerate(per_row):
        err += (e - err) / (i + 1.0)
    return err


def bind_parent(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_bmu_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint8), C.c_int, C.c_void_p]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    return L


class ParentOut(C.Structure):
    """vsom_masked_out"""
    _fields_ = [("bmu", C.POINTER(C.c_uint64)), ("dist", C.POINTER(C.c_float)), ("nvalid", C.POINTER(C.c_uint32)),
                ("fill", C.POINTER(C.c_float))]


def run(name, rounds, lib_path):
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    import vsom_amd
    from vsom_amd import capi
    W, H, J, rows, one = CASES[name]
    m, s, hits, X, valid, binary, continuous = state(W, H, J, rows, one)
    ctx = vsom_amd.Context(W, H, J, 0)
    ctx.set_state(map=m, sigma=s, hits=hits)
    ctx.upload_chunk(X)
    full = np.ascontiguousarray(np.broadcast_to(valid, (rows, J)))     # the unmasked calls take rows x J only

    L = bind_parent(lib_path or capi.LIB_PATH)
    fp, u64p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)

    def ok(rc):
        if rc:
            raise RuntimeError(L.vsom_last_error().decode())

    h = C.c_void_p()
    ok(L.vsom_create(C.byref(h), 0, W, H, J, 0))
    ok(L.vsom_set_state(h, m.ctypes.data_as(fp), s.ctypes.data_as(fp), None, None, hits.ctypes.data_as(u64p)))
    ok(L.vsom_upload_chunk(h, X.ctypes.data_as(fp), rows))
    hm, hs = np.empty_like(m), np.empty_like(s)
    bmu, dist = np.empty(rows, np.uint64), np.empty(rows, np.float32)
    pout = ParentOut(bmu.ctypes.data_as(u64p), dist.ctypes.data_as(fp), None, None)

    def parent_search(min_hits):
        ok(L.vsom_bmu_masked_batch(h, min_hits, 0, rows, valid.ctypes.data_as(u8p), int(one), C.byref(pout)))

    def touch():
        ok(L.vsom_set_state(h, None, None, None, None, hits.ctypes.data_as(u64p)))

    calls = {
        "similarity": {
            "new": lambda: ctx.similarity_masked(valid, MIN_HITS, NUM_SIGMAS, capi.SIGMA_AS_WRITTEN),
            "parent": lambda: (parent_search(MIN_HITS),
                               ok(L.vsom_get_state(h, hm.ctypes.data_as(fp), hs.ctypes.data_as(fp), None, None, None)),
                               similarity_epilogue(X, hm, hs, bmu, valid, NUM_SIGMAS)),
            "unmasked": lambda: ctx.similarity(MIN_HITS, NUM_SIGMAS, capi.SIGMA_AS_WRITTEN, valid=full),
        },
        "evaluate": {
            "new": lambda: ctx.evaluate_masked(valid, binary, continuous),
            "parent": lambda: (parent_search(0), ok(L.vsom_get_state(h, hm.ctypes.data_as(fp), None, None, None, None)),
                               evaluate_epilogue(X, hm, bmu, dist, valid, binary, continuous)),
            "unmasked": lambda: ctx.evaluate(binary, continuous, valid=full),
        },
    }
    out = []
    for call, routes in calls.items():
        for _ in range(3):
            for fn in routes.values():
                fn()
        new = routes["new"]()
        routes["parent"]()
        assert (new["bmu"] == bmu).all() and (new["dist"].view(np.uint32) == dist.view(np.uint32)).all()
        ts = {k: [] for k in routes}
        for _ in range(rounds):
            touch()
            for k, fn in routes.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append(time.perf_counter() - t0)
        res = {"case": name, "call": call, "shape": f"{W}x{H}x{J}", "rows": rows, "mask": "column" if one else "rows",
               "invalid_fraction": round(1.0 - float(np.broadcast_to(valid, (rows, J)).mean()), 4), "rounds": rounds,
               "parent_lib": "given" if lib_path else "this tree's"}
        for k in routes:
            put(res, k, ts[k])
        ctx.enable_timing(True, groups=["bmu", "finish"])
        ctx.get_timing(reset=True)
        tb, tf = [], []
        for _ in range(rounds):
            routes["new"]()
            t = ctx.get_timing(reset=True)
            tb.append(t["bmu"][0] * 1e-3)
            tf.append(t["finish"][0] * 1e-3)
        ctx.enable_timing(False)
        put(res, "search", tb)
        put(res, "scoring", tf)
        out.append(res)
    L.vsom_destroy(h)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="", help="libvsom_hip.so of a build of the parent commit, for the parent route")
    ap.add_argument("--tag", default="")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--cases", default="rows10,labels10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "masked_score_bench.jsonl"))
    a = ap.parse_args()
    for name in a.cases.split(","):
        for res in run(name, a.rounds, a.lib):
            if a.tag:
                res["tag"] = a.tag
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
