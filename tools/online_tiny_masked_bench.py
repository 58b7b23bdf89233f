#!/usr/bin/env python3
"""Masked online chunks of tiny maps in one launch against the calls they replace.

The workload is the reference's own smallest scenario (tests/performance/perf_tests.cpp:74-112) with missing fields: a
10x10x9 map on the 20-row fixture, 10 % of the entries invalid, one online chunk at sigma = 3 (the exhaustive search) and at
sigma = 1 (the local walk).  Cases: one context (vsom_train_online_chunk_masked) and ensembles of K in --ks members on one
stream (vsom_ensemble_train_online_chunk_masked).  Three routes per case, one JSON line per case and sigma:

  new_us        the masked chunk call of this build (the one-launch kernel)
  parent_us     what a caller had before it: K vsom_train_online_chunk_masked calls on K separate contexts through --lib (a
                build of the parent commit, whose call is the per-sample loop; the in-tree library when none is given)
  unmasked_us   vsom_train_online_chunk_fetch / vsom_ensemble_train_online_chunk_fetch of this build on the same rows
  *_p10 / *_p90 the 10th and 90th percentile over the timed rounds (the figures above are medians)
  vs_parent     parent_us / new_us;   vs_unmasked   new_us / unmasked_us

--warmup warm-up and --reps timed rounds per route, the routes timed alternately, each round from the same initial maps
(the reset is outside the timed region).  The parent route of a large ensemble runs min(--reps, 3000 // K) timed rounds, at
least 5 (parent_reps in the line).  Every call ends in a host wait and hands back lastBMU and the MSE.  Before any timing
the new route's map, SMap, sigmaMap, weightMap, bmuHits, lastBMU and MSE are compared with the parent route's on the bits; a
difference ends the run.

usage: tools/online_tiny_masked_bench.py [--ks 16,256,1024] [--reps 30] [--warmup 3] [--lib FILE] [--tag TEXT] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen  # noqa: E402

INTREE = os.path.join(ROOT, "variational-self-organizing-maps_amd", "libvsom_hip.so")
W, H, J, B = 10, 10, 9, 20
N = W * H
ETA, EXPONENTIAL = 0.3, 0
vp, fp, dp, u64p, u8p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
ip = C.POINTER(C.c_int)


def bind(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    L.vsom_set_stream.argtypes = [vp, vp]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_set_last_bmu.argtypes = [vp, u64p]
    L.vsom_train_online_chunk_fetch.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int, u64p, fp]
    L.vsom_train_online_chunk_masked.argtypes = [vp, C.c_double, C.c_double, C.c_int, C.c_int, u8p, C.c_int, u64p, fp]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_train_online_chunk_fetch.argtypes = [vp, dp, dp, ip, C.c_int, C.POINTER(u64p), fp]
    if hasattr(L, "vsom_ensemble_train_online_chunk_masked"):
        L.vsom_ensemble_train_online_chunk_masked.argtypes = [vp, dp, dp, ip, C.c_int, C.POINTER(u8p), ip, C.POINTER(u64p), fp]
    return L


def ok(L, rc):
    if rc != 0:
        raise SystemExit(f"libvsom_hip error {rc}: {L.vsom_last_error().decode(errors='replace')}")


def f32(a):
    return a.ctypes.data_as(fp)


class Side:
    """K contexts of one library on one stream, their ensemble (ens: the case is an ensemble), the rows loaded into each"""

    def __init__(self, L, K, ens, stream, X, inits):
        self.L, self.K, self.inits = L, K, inits
        self.h = []
        for k in range(K):
            h = vp()
            ok(L, L.vsom_create(C.byref(h), 0, W, H, J, 0))
            ok(L, L.vsom_set_stream(h, stream))
            ok(L, L.vsom_upload_chunk(h, f32(X), B))
            self.h.append(h)
        self.ens = vp()
        if ens:
            ok(L, L.vsom_ensemble_create(C.byref(self.ens), (vp * K)(*[h.value for h in self.h]), K))
        self.zero_hits = np.zeros(N, np.uint64)
        self.start = (np.arange(B, dtype=np.uint64) * 7) % N       # where the local walk of sigma <= 1 starts
        self.zeros = np.zeros((N, J), np.float32)
        self.zero_w = np.zeros(N, np.float32)
        self.lb = np.zeros((K, B), np.uint64)
        self.mse = np.zeros(K, np.float32)
        self.lbp = (u64p * K)(*[self.lb[k].ctypes.data_as(u64p) for k in range(K)])

    def reset(self):
        for h, init in zip(self.h, self.inits):
            ok(self.L, self.L.vsom_set_state(h, f32(init), f32(self.zeros), f32(self.zeros), f32(self.zero_w),
                                             self.zero_hits.ctypes.data_as(u64p)))
            ok(self.L, self.L.vsom_set_last_bmu(h, self.start.ctypes.data_as(u64p)))

    def state(self):
        out = []
        for k, h in enumerate(self.h):
            m, s, g, w = (np.zeros((N, J), np.float32), np.zeros((N, J), np.float32), np.zeros((N, J), np.float32),
                          np.zeros(N, np.float32))
            hits = np.zeros(N, np.uint64)
            ok(self.L, self.L.vsom_get_state(h, f32(m), f32(g), f32(s), f32(w), hits.ctypes.data_as(u64p)))
            out.append((m, g, s, w, hits, self.lb[k].copy(), self.mse[k:k + 1].copy()))
        return out

    def close(self):
        if self.ens:
            self.L.vsom_ensemble_destroy(self.ens)
        for h in self.h:
            self.L.vsom_destroy(h)


def same_bits(a, b):
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def run(K, ens, sigma, new, old, reps, warmup, hip, tag):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.ascontiguousarray(np.array(fx["rows"], np.float32))
    valid = np.ascontiguousarray(np.random.default_rng(5).random((B, J)) >= 0.1, dtype=np.uint8)
    Xz = np.ascontiguousarray(np.where(valid != 0, X, np.float32(0)))      # a NULL is stored as 0.0f with valid = 0
    inits = [gen.random_map(N, J, seed=100 + k) for k in range(K)]
    stream = vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    a, b, u = (Side(L, K, e, stream, Xz, inits) for L, e in ((new, ens), (old, False), (new, ens)))
    vptr = valid.ctypes.data_as(u8p)
    etas, sigs, fns = (C.c_double * K)(*([ETA] * K)), (C.c_double * K)(*([sigma] * K)), (C.c_int * K)(*([EXPONENTIAL] * K))
    vptrs = (u8p * K)(*([vptr] * K))

    def masked():
        if ens:
            ok(new, new.vsom_ensemble_train_online_chunk_masked(a.ens, etas, sigs, fns, 1, vptrs, None, a.lbp, f32(a.mse)))
        else:
            ok(new, new.vsom_train_online_chunk_masked(a.h[0], ETA, sigma, EXPONENTIAL, 1, vptr, 0, a.lbp[0], f32(a.mse)))

    msep = [f32(b.mse[k:]) for k in range(K)]     # (no bookkeeping in the timed region)

    def parent():
        for k, h in enumerate(b.h):
            ok(old, old.vsom_train_online_chunk_masked(h, ETA, sigma, EXPONENTIAL, 1, vptr, 0, b.lbp[k], msep[k]))

    def unmasked():
        if ens:
            ok(new, new.vsom_ensemble_train_online_chunk_fetch(u.ens, etas, sigs, fns, 1, u.lbp, f32(u.mse)))
        else:
            ok(new, new.vsom_train_online_chunk_fetch(u.h[0], ETA, sigma, EXPONENTIAL, 1, u.lbp[0], f32(u.mse)))

    a.reset()
    b.reset()
    masked()
    parent()
    for k, (sa, sb) in enumerate(zip(a.state(), b.state())):
        for what, x, y in zip(("map", "sigmaMap", "SMap", "weightMap", "bmuHits", "lastBMU", "MSE"), sa, sb):
            if not same_bits(x, y):
                raise SystemExit(f"K={K} sigma={sigma}: {what} of map {k} differs from the parent route's")

    preps = max(5, min(reps, 3000 // K))
    ts = {"new": [], "parent": [], "unmasked": []}
    for rep in range(warmup + reps):
        for side, fn, s in (("new", masked, a), ("parent", parent, b), ("unmasked", unmasked, u)):
            if side == "parent" and rep >= warmup + preps:
                continue
            s.reset()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts[side].append(dt * 1e6)
    res = {"bench": "online_tiny_masked", "tag": tag, "map": f"{W}x{H}x{J}", "rows": B,
           "invalid": round(float((valid == 0).mean()), 3), "sigma": sigma, "case": "ensemble" if ens else "context", "K": K,
           "reps": reps, "parent_reps": preps, "bits_equal": True}
    for side in ("new", "parent", "unmasked"):
        res[f"{side}_us"] = round(float(np.median(ts[side])), 1)
        res[f"{side}_us_p10"] = round(float(np.percentile(ts[side], 10)), 1)
        res[f"{side}_us_p90"] = round(float(np.percentile(ts[side], 90)), 1)
    res["new_per_map_us"] = round(res["new_us"] / K, 3)
    res["vs_parent"] = round(res["parent_us"] / res["new_us"], 2)
    res["vs_unmasked"] = round(res["new_us"] / res["unmasked_us"], 2)
    for s in (a, b, u):
        s.close()
    hip.hipStreamDestroy(stream)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=INTREE, help="the library the parent route runs on (a build of the parent commit)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "online_tiny_masked_bench.jsonl"))
    a = ap.parse_args()
    new = bind(INTREE)
    old = new if os.path.abspath(a.lib) == os.path.abspath(INTREE) else bind(a.lib)
    new.vsom_device_count.restype = C.c_int
    if new.vsom_device_count() < 1:
        raise SystemExit("online_tiny_masked_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    with open(a.out, "w") as out:
        for K, ens in [(1, False)] + [(int(k), True) for k in a.ks.split(",")]:
            for sigma in (3.0, 1.0):
                line = json.dumps(run(K, ens, sigma, new, old, a.reps, a.warmup, hip, a.tag))
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
