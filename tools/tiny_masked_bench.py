#!/usr/bin/env python3
"""Masked schedules of tiny maps in one launch against the calls they replace.

The workload is the reference's own smallest scenario (tests/performance/perf_tests.cpp:74-112) with missing fields: a
10x10x9 map on the 20-row fixture, 10 % of the entries invalid, sigma0 = 5 and decay 0.05 (33 epochs run before sigma < 1).
Cases: one context (vsom_batch_schedule_masked) and ensembles of K in --ks members on one stream
(vsom_ensemble_batch_schedule_masked).  Three routes per case, one JSON line per case:

  new_us        the masked schedule call of this build
  parent_us     what a caller had before it: K x 33 vsom_batch_epoch_masked calls through --lib (a build of the parent
                commit; the in-tree library when none is given); reset_bmu = 0, so the loop is those calls and nothing else
  unmasked_us   vsom_batch_schedule / vsom_ensemble_batch_schedule of this build on the same rows, every entry valid
  *_p10 / *_p90 the 10th and 90th percentile over the timed rounds (the figures above are medians)
  vs_parent     parent_us / new_us;   vs_unmasked   new_us / unmasked_us

--warmup warm-up and --reps timed rounds per route, the routes timed alternately, each round from the same initial maps
(the reset is outside the timed region).  The parent route of a large ensemble is tens of thousands of blocking calls a
round: it runs min(--reps, 3000 // K) timed rounds, at least 5 (parent_reps in the line).  Every call ends in a host wait.
Before any timing the new route's map, sigmaMap, weightMap, bmuHits, lastBMU and per-epoch MSEs are compared with the
parent route's on the bits; a difference ends the run.

usage: tools/tiny_masked_bench.py [--ks 1,16,256,1024] [--reps 30] [--warmup 3] [--lib FILE] [--tag TEXT] [--out FILE]"""
import argparse
import ctypes as C
import json
import math
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
EPOCHS, SIGMA0, DECAY = 40, 5.0, 0.05
vp, fp, dp, u64p, u8p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


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
    L.vsom_get_last_bmu.argtypes = [vp, u64p]
    L.vsom_set_last_bmu.argtypes = [vp, u64p]
    L.vsom_batch_epoch_masked.argtypes = [vp, C.c_double, C.c_int, u8p, C.c_int, fp]
    L.vsom_batch_schedule.argtypes = [vp, dp, C.c_size_t, C.c_int, fp]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_batch_schedule.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(fp)]
    if hasattr(L, "vsom_batch_schedule_masked"):
        L.vsom_batch_schedule_masked.argtypes = [vp, dp, C.c_size_t, C.c_int, u8p, C.c_int, fp]
        L.vsom_ensemble_batch_schedule_masked.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(u8p),
                                                          C.POINTER(C.c_int), C.POINTER(fp)]
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
        self.zero_lb = np.zeros(B, np.uint64)
        self.zeros = np.zeros((N, J), np.float32)
        self.zero_w = np.zeros(N, np.float32)

    def reset(self):
        for h, init in zip(self.h, self.inits):
            ok(self.L, self.L.vsom_set_state(h, f32(init), f32(self.zeros), None, f32(self.zero_w),
                                             self.zero_hits.ctypes.data_as(u64p)))
            ok(self.L, self.L.vsom_set_last_bmu(h, self.zero_lb.ctypes.data_as(u64p)))

    def state(self):
        out = []
        for h in self.h:
            m, s, w = np.zeros((N, J), np.float32), np.zeros((N, J), np.float32), np.zeros(N, np.float32)
            hits, lb = np.zeros(N, np.uint64), np.zeros(B, np.uint64)
            ok(self.L, self.L.vsom_get_state(h, f32(m), f32(s), None, f32(w), hits.ctypes.data_as(u64p)))
            ok(self.L, self.L.vsom_get_last_bmu(h, lb.ctypes.data_as(u64p)))
            out.append((m, s, w, hits, lb))
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


def run(K, ens, new, old, reps, warmup, hip, tag):
    sig = []
    for i in range(EPOCHS):
        s = SIGMA0 * math.exp(-DECAY * i)
        if s < 1.0:             # trainBatchSom's stop (Som.cpp:729-730)
            break
        sig.append(s)
    E = len(sig)
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.ascontiguousarray(np.array(fx["rows"], np.float32))
    valid = np.ascontiguousarray(np.random.default_rng(5).random((B, J)) >= 0.1, dtype=np.uint8)
    Xz = np.ascontiguousarray(np.where(valid != 0, X, np.float32(0)))      # a NULL is stored as 0.0f with valid = 0
    inits = [gen.random_map(N, J, seed=100 + k) for k in range(K)]
    stream = vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    a, b, u = (Side(L, K, e, stream, Xz, inits) for L, e in ((new, ens), (old, False), (new, ens)))
    sg = (C.c_double * E)(*sig)
    vptr = valid.ctypes.data_as(u8p)
    mse_a, mse_u = np.zeros((K, E), np.float32), np.zeros((K, E), np.float32)
    sigs = (dp * K)(*[C.cast(sg, dp)] * K)
    outs_a = (fp * K)(*[mse_a[k].ctypes.data_as(fp) for k in range(K)])
    outs_u = (fp * K)(*[mse_u[k].ctypes.data_as(fp) for k in range(K)])
    cnt = (C.c_size_t * K)(*([E] * K))
    vptrs = (u8p * K)(*([vptr] * K))
    mse_b = np.zeros((K, E), np.float32)     # the loop's calls store straight into it: no bookkeeping in the timed region
    slots = [[mse_b[k, ep:].ctypes.data_as(fp) for ep in range(E)] for k in range(K)]

    def masked():
        if ens:
            ok(new, new.vsom_ensemble_batch_schedule_masked(a.ens, sigs, cnt, 0, vptrs, None, outs_a))
        else:
            ok(new, new.vsom_batch_schedule_masked(a.h[0], sg, E, 0, vptr, 0, outs_a[0]))

    def parent():
        for ep in range(E):
            for k, h in enumerate(b.h):
                ok(old, old.vsom_batch_epoch_masked(h, sig[ep], 1 if ep == 0 else 0, vptr, 0, slots[k][ep]))

    def unmasked():
        if ens:
            ok(new, new.vsom_ensemble_batch_schedule(u.ens, sigs, cnt, 0, outs_u))
        else:
            ok(new, new.vsom_batch_schedule(u.h[0], sg, E, 0, outs_u[0]))

    a.reset()
    b.reset()
    masked()
    parent()
    if not same_bits(mse_a, mse_b):
        raise SystemExit(f"K={K}: the per-epoch MSEs differ from the parent route's")
    for k, (sa, sb) in enumerate(zip(a.state(), b.state())):
        for what, x, y in zip(("map", "sigmaMap", "weightMap", "bmuHits", "lastBMU"), sa, sb):
            if not same_bits(x, y):
                raise SystemExit(f"K={K}: {what} of map {k} differs from the parent route's")

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
    res = {"bench": "tiny_masked", "tag": tag, "map": f"{W}x{H}x{J}", "rows": B, "invalid": round(float((valid == 0).mean()), 3),
           "epochs": E, "case": "ensemble" if ens else "context", "K": K, "reps": reps, "parent_reps": preps, "bits_equal": True}
    for side in ("new", "parent", "unmasked"):
        res[f"{side}_us"] = round(float(np.median(ts[side])), 1)
        res[f"{side}_us_p10"] = round(float(np.percentile(ts[side], 10)), 1)
        res[f"{side}_us_p90"] = round(float(np.percentile(ts[side], 90)), 1)
    res["new_per_map_epoch_us"] = round(res["new_us"] / E / K, 3)
    res["vs_parent"] = round(res["parent_us"] / res["new_us"], 2)
    res["vs_unmasked"] = round(res["new_us"] / res["unmasked_us"], 2)
    for s in (a, b, u):
        s.close()
    hip.hipStreamDestroy(stream)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=INTREE, help="the library the parent route runs on (a build of the parent commit)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiny_masked_bench.jsonl"))
    a = ap.parse_args()
    new = bind(INTREE)
    old = new if os.path.abspath(a.lib) == os.path.abspath(INTREE) else bind(a.lib)
    new.vsom_device_count.restype = C.c_int
    if new.vsom_device_count() < 1:
        raise SystemExit("tiny_masked_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    with open(a.out, "w") as out:
        for K, ens in [(1, False)] + [(int(k), True) for k in a.ks.split(",")]:
            line = json.dumps(run(K, ens, new, old, a.reps, a.warmup, hip, a.tag))
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
