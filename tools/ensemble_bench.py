#!/usr/bin/env python3
"""Ensembles against one call per map: the reference's training scenario (tests/performance/perf_tests.cpp:74-112:
10x10x9 maps, 20 rows a chunk, Exponential decay, sigma > 1) for K maps at once.  One JSON line per (layout, K):

  online_us / batch_us            one ensemble call (vsom_ensemble_train_online_chunk_fetch / vsom_ensemble_batch_epoch)
                                  for all K maps, median over the timed epochs
  *_us_per_map                    the same divided by K
  seq_online_us / seq_batch_us    K sequential vsom_train_online_chunk_fetch / vsom_batch_epoch calls
  upload_us                       K vsom_upload_chunk calls (the host-side cost of giving every map its rows; not
                                  part of the numbers above)

layout "shared": every member on one stream (vsom_set_stream); "separate": each member on its own stream.  The C ABI is
called through ctypes with prebuilt argument arrays, so the numbers hold no per-call Python allocation.

usage: tools/ensemble_bench.py [--ks 1,16,64,256,1024] [--epochs 20] [--warmup 3] [--out FILE]"""
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


def run(K, layout, epochs, warmup, hip):
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

    res = {"bench": "ensemble", "map": f"{W}x{H}x{J}", "rows": B, "K": K, "layout": layout}
    seq_epochs = max(3, min(epochs, 2000 // K))
    for name, f, n in (("online", ens_online, epochs), ("seq_online", seq_online, seq_epochs),
                       ("batch", ens_batch, epochs), ("seq_batch", seq_batch, seq_epochs), ("upload", upload, seq_epochs)):
        med, lo, hi = median_us(f, n, warmup)
        res[f"{name}_us"] = round(med, 1)
        res[f"{name}_us_min"] = round(lo, 1)
        res[f"{name}_us_max"] = round(hi, 1)
        res[f"{name}_us_per_map"] = round(med / K, 2)
    res["online_speedup"] = round(res["seq_online_us"] / res["online_us"], 1)
    res["batch_speedup"] = round(res["seq_batch_us"] / res["batch_us"], 1)
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
            line = json.dumps(run(K, layout, a.epochs, a.warmup, hip))
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
