#!/usr/bin/env python3
"""Ensembles against one call per map: the reference's training scenario (tests/performance/perf_tests.cpp:74-112:
10x10x9 maps, 20 rows a chunk, Exponential decay, sigma > 1) for K maps at once.  One JSON line per (layout, K):

  online_us / batch_us            one ensemble call (vsom_ensemble_train_online_chunk_fetch / vsom_ensemble_batch_epoch)
                                  for all K maps, median over the timed epochs
  *_us_per_map                    the same divided by K
  seq_online_us / seq_batch_us    K sequential vsom_train_online_chunk_fetch / vsom_batch_epoch calls
  upload_us                       K vsom_upload_chunk calls (the host-side cost of giving every map its rows; not
                                  part of the numbers above)
  ens_upload_us                   one vsom_ensemble_upload_chunks (wait = 1) giving every map its own rows
  ens_upload_shared_us            the same with every map on the same rows (one shared offset)
  score_us / seq_score_us         one vsom_ensemble_bmu_batch / K sequential vsom_bmu_batch calls (idx and dist of
                                  every row handed back)
  upload_speedup / score_speedup  upload_us / ens_upload_us and seq_score_us / score_us

layout "shared": every member on one stream (vsom_set_stream); "separate": each member on its own stream.  The C ABI is
called through ctypes with prebuilt argument arrays, so the numbers hold no per-call Python allocation.

--io-only: the three ensemble I/O columns alone (ens_upload_us, ens_upload_shared_us, score_us), for a kernel trace whose
counts are those calls' (the set-up adds K vsom_upload_chunk calls of its own).

usage: tools/ensemble_bench.py [--ks 1,16,64,256,1024] [--epochs 20] [--warmup 3] [--io-only] [--out FILE]"""
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

W, H, J, B = 10, 10, 9, 20


def median_us(fn, epochs, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(epochs):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6, float(np.max(ts)) * 1e6


def run(K, layout, epochs, warmup, hip, io_only=False):
    L = capi.lib()
    ctxs, Xs = [], []
    stream = C.c_void_p()
    if layout == "shared":
        assert hip.hipStreamCreate(C.byref(stream)) == 0
    for k in range(K):
        c = vsom_amd.Context(W, H, J)
        c.set_state(map=gen.random_map(W * H, J, seed=100 + k))
        if layout == "shared":
            c.set_stream(stream.value)
        X = gen.blobs(B, J, 4, 1 + k, 2 + k, sigma=0.3)
        c.upload_chunk(X)
        ctxs.append(c)
        Xs.append(X)
    ens = vsom_amd.Ensemble(ctxs)
    eta = (C.c_double * K)(*[0.05 + 0.1 * k / K for k in range(K)])
    sigma = (C.c_double * K)(*([3.0] * K))
    fn = (C.c_int * K)(*([capi.EXPONENTIAL] * K))
    lbs = [np.zeros(B, np.uint64) for _ in range(K)]
    lbp = (C.POINTER(C.c_uint64) * K)(*[a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in lbs])
    mse = np.zeros(K, np.float32)
    msep = mse.ctypes.data_as(C.POINTER(C.c_float))
    one = C.c_float()
    hs = [c._h for c in ctxs]
    xp = [X.ctypes.data_as(C.POINTER(C.c_float)) for X in Xs]

    def ens_online():
        capi.check(L.vsom_ensemble_train_online_chunk_fetch(ens._h, eta, sigma, fn, 1, lbp, msep))

    def seq_online():
        for k in range(K):
            capi.check(L.vsom_train_online_chunk_fetch(hs[k], eta[k], 3.0, capi.EXPONENTIAL, 1, lbp[k], C.byref(one)))

    def ens_batch():
        capi.check(L.vsom_ensemble_batch_epoch(ens._h, sigma, 1, msep))

    def seq_batch():
        for k in range(K):
            capi.check(L.vsom_batch_epoch(hs[k], 3.0, 1, C.byref(one)))

    def upload():
        for k in range(K):
            capi.check(L.vsom_upload_chunk(hs[k], xp[k], B))

    allx = np.ascontiguousarray(np.concatenate(Xs), dtype=np.float32)
    allp = allx.ctypes.data_as(C.POINTER(C.c_float))
    offs = (C.c_size_t * K)(*[k * B * J for k in range(K)])
    zero = (C.c_size_t * K)(*([0] * K))
    bs = (C.c_size_t * K)(*([B] * K))

    def ens_upload():
        capi.check(L.vsom_ensemble_upload_chunks(ens._h, allp, allx.size, offs, bs, 1))

    def ens_upload_shared():
        capi.check(L.vsom_ensemble_upload_chunks(ens._h, allp, B * J, zero, bs, 1))

    idx = [np.zeros(B, np.uint64) for _ in range(K)]
    dist = [np.zeros(B, np.float32) for _ in range(K)]
    ip = (C.POINTER(C.c_uint64) * K)(*[a.ctypes.data_as(C.POINTER(C.c_uint64)) for a in idx])
    dp = (C.POINTER(C.c_float) * K)(*[a.ctypes.data_as(C.POINTER(C.c_float)) for a in dist])

    def score():
        capi.check(L.vsom_ensemble_bmu_batch(ens._h, ip, dp))

    def seq_score():
        for k in range(K):
            capi.check(L.vsom_bmu_batch(hs[k], ip[k], dp[k]))

    res = {"bench": "ensemble", "map": f"{W}x{H}x{J}", "rows": B, "K": K, "layout": layout}
    seq_epochs = max(3, min(epochs, 2000 // K))
    cases = (("online", ens_online, epochs), ("seq_online", seq_online, seq_epochs),
             ("batch", ens_batch, epochs), ("seq_batch", seq_batch, seq_epochs), ("upload", upload, seq_epochs),
             ("ens_upload", ens_upload, epochs), ("ens_upload_shared", ens_upload_shared, epochs),
             ("score", score, epochs), ("seq_score", seq_score, seq_epochs))
    if io_only:
        cases = [c for c in cases if c[0] in ("ens_upload", "ens_upload_shared", "score")]
    for name, f, n in cases:
        med, lo, hi = median_us(f, n, warmup)
        res[f"{name}_us"] = round(med, 1)
        res[f"{name}_us_min"] = round(lo, 1)
        res[f"{name}_us_max"] = round(hi, 1)
        res[f"{name}_us_per_map"] = round(med / K, 2)
    if not io_only:
        res["online_speedup"] = round(res["seq_online_us"] / res["online_us"], 1)
        res["batch_speedup"] = round(res["seq_batch_us"] / res["batch_us"], 1)
        res["upload_speedup"] = round(res["upload_us"] / res["ens_upload_us"], 1)
        res["score_speedup"] = round(res["seq_score_us"] / res["score_us"], 1)
    ens.close()
    for c in ctxs:
        c.close()
    if layout == "shared":
        hip.hipStreamDestroy(stream)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,64,256,1024")
    ap.add_argument("--layouts", default="shared,separate")
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--io-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("ensemble_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    out = open(a.out, "w") if a.out else None
    for layout in a.layouts.split(","):
        for K in (int(k) for k in a.ks.split(",")):
            line = json.dumps(run(K, layout, a.epochs, a.warmup, hip, a.io_only))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
