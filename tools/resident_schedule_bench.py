#!/usr/bin/env python3
"""A whole batch schedule in one call against the loop of single-epoch calls it replaces.

The workload is the reference's own smallest scenario (tests/performance/perf_tests.cpp:74-112): a 10x10x9 map on the
20-row fixture, sigma0 = 5.  Two schedules: decay 0.05 (33 epochs run before sigma < 1) and decay 0.005 (200 epochs).
For K in --ks maps on one shared stream, one JSON line per (schedule, K):

  schedule_us        one vsom_batch_schedule (K = 1) or vsom_ensemble_batch_schedule call for the whole schedule
  loop_us            the calls it replaces: one vsom_batch_epoch (K = 1) or vsom_ensemble_batch_epoch per epoch, through
                     --lib (the in-tree library, or a build of the parent commit); reset_bmu = 0, so the loop is those calls
                     and nothing else
  *_min / *_max      the spread over --reps repetitions (the figures above are medians)
  *_per_epoch_us     divided by the epochs;  *_per_map_epoch_us  divided by epochs * K
  speedup            loop_us / schedule_us

Every call ends in a host wait.  Both sides are driven through ctypes with prebuilt argument arrays; what remains of
Python in the loop side is one ctypes call per epoch (well under a microsecond), which a C caller would not pay.  The
two sides are timed alternately, each repetition from the same initial maps (the
reset is outside the timed region).  Before any timing the two results are compared on the bits, for reset_bmu 0 and 1
(map, sigmaMap, weightMap, bmuHits, lastBMU, every epoch's MSE); a difference ends the run.

usage: tools/resident_schedule_bench.py [--ks 1,16,64,256,1024] [--reps 15] [--warmup 2] [--lib FILE] [--tag TEXT] [--out FILE]"""
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
SCHEDULES = {"33_epochs": (40, 5.0, 0.05), "200_epochs": (200, 5.0, 0.005)}
vp, fp, dp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint64)


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
    L.vsom_batch_epoch.argtypes = [vp, C.c_double, C.c_int, fp]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_batch_epoch.argtypes = [vp, dp, C.c_int, fp]
    if hasattr(L, "vsom_batch_schedule"):
        L.vsom_batch_schedule.argtypes = [vp, dp, C.c_size_t, C.c_int, fp]
        L.vsom_ensemble_batch_schedule.argtypes = [vp, C.POINTER(dp), C.POINTER(C.c_size_t), C.c_int, C.POINTER(fp)]
    return L


def ok(L, rc):
    if rc != 0:
        raise SystemExit(f"libvsom_hip error {rc}: {L.vsom_last_error().decode(errors='replace')}")


def f32(a):
    return a.ctypes.data_as(fp)


class Side:
    """K contexts of one library on one stream, their ensemble, and the fixture rows loaded into each"""

    def __init__(self, L, K, stream, X, inits):
        self.L, self.K, self.inits = L, K, inits
        self.h = []
        for k in range(K):
            h = vp()
            ok(L, L.vsom_create(C.byref(h), 0, W, H, J, 0))
            ok(L, L.vsom_set_stream(h, stream))
            ok(L, L.vsom_upload_chunk(h, f32(X), B))
            self.h.append(h)
        self.ens = vp()
        if K > 1:
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
        if self.K > 1:
            self.L.vsom_ensemble_destroy(self.ens)
        for h in self.h:
            self.L.vsom_destroy(h)


def same_bits(a, b):
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def run(name, K, new, old, reps, warmup, hip, tag):
    epochs, sigma0, decay = SCHEDULES[name]
    sig = []
    for i in range(epochs):
        s = sigma0 * math.exp(-decay * i)
        if s < 1.0:             # trainBatchSom's stop (Som.cpp:729-730)
            break
        sig.append(s)
    E = len(sig)
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.ascontiguousarray(np.array(fx["rows"], np.float32))
    inits = [gen.random_map(N, J, seed=100 + k) for k in range(K)]
    stream = vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    a, b = Side(new, K, stream, X, inits), Side(old, K, stream, X, inits)
    sg = (C.c_double * E)(*sig)
    mse_a = np.zeros((K, E), np.float32)
    sigs = (dp * K)(*[C.cast(sg, dp)] * K)
    outs = (fp * K)(*[mse_a[k].ctypes.data_as(fp) for k in range(K)])
    cnt = (C.c_size_t * K)(*([E] * K))
    per_epoch = [(C.c_double * K)(*([s] * K)) for s in sig]
    mse_b = np.zeros((E, K), np.float32)     # the loop's calls store straight into it: no bookkeeping in the timed region
    rows = [mse_b[ep].ctypes.data_as(fp) for ep in range(E)]
    zero_lb = np.zeros(B, np.uint64).ctypes.data_as(u64p)

    def schedule(reset_bmu):
        if K == 1:
            ok(new, new.vsom_batch_schedule(a.h[0], sg, E, reset_bmu, outs[0]))
        else:
            ok(new, new.vsom_ensemble_batch_schedule(a.ens, sigs, cnt, reset_bmu, outs))

    def loop(reset_bmu):
        for ep in range(E):
            if ep > 0 and reset_bmu:
                for h in b.h:
                    ok(old, old.vsom_set_last_bmu(h, zero_lb))
            if K == 1:
                ok(old, old.vsom_batch_epoch(b.h[0], sig[ep], 1 if ep == 0 else 0, rows[ep]))
            else:
                ok(old, old.vsom_ensemble_batch_epoch(b.ens, per_epoch[ep], 1 if ep == 0 else 0, rows[ep]))

    for reset_bmu in (1, 0):
        a.reset()
        b.reset()
        schedule(reset_bmu)
        loop(reset_bmu)
        if not same_bits(mse_a, np.ascontiguousarray(mse_b.T)):
            raise SystemExit(f"{name} K={K} reset_bmu={reset_bmu}: the per-epoch MSEs differ")
        for k, (sa, sb) in enumerate(zip(a.state(), b.state())):
            for what, x, y in zip(("map", "sigmaMap", "weightMap", "bmuHits", "lastBMU"), sa, sb):
                if not same_bits(x, y):
                    raise SystemExit(f"{name} K={K} reset_bmu={reset_bmu}: {what} of map {k} differs")

    ts = {"schedule": [], "loop": []}
    for rep in range(warmup + reps):
        for side, fn, s in (("schedule", schedule, a), ("loop", loop, b)):
            s.reset()
            t0 = time.perf_counter()
            fn(0)
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts[side].append(dt * 1e6)
    res = {"bench": "resident_schedule", "tag": tag, "map": f"{W}x{H}x{J}", "rows": B, "schedule": name, "epochs": E, "K": K,
           "reps": reps, "bits_equal": True}
    for side in ("schedule", "loop"):
        med = float(np.median(ts[side]))
        res[f"{side}_us"] = round(med, 1)
        res[f"{side}_us_min"] = round(float(np.min(ts[side])), 1)
        res[f"{side}_us_max"] = round(float(np.max(ts[side])), 1)
        res[f"{side}_per_epoch_us"] = round(med / E, 2)
        res[f"{side}_per_map_epoch_us"] = round(med / E / K, 3)
    res["speedup"] = round(res["loop_us"] / res["schedule_us"], 2)
    a.close()
    b.close()
    hip.hipStreamDestroy(stream)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,16,64,256,1024")
    ap.add_argument("--schedules", default="33_epochs,200_epochs")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib", default=INTREE, help="the library the loop runs on (a build of the parent commit)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_schedule_bench.jsonl"))
    a = ap.parse_args()
    new = bind(INTREE)
    old = new if os.path.abspath(a.lib) == os.path.abspath(INTREE) else bind(a.lib)
    new.vsom_device_count.restype = C.c_int
    if new.vsom_device_count() < 1:
        raise SystemExit("resident_schedule_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    with open(a.out, "w") as out:
        for name in a.schedules.split(","):
            for K in (int(k) for k in a.ks.split(",")):
                reps = max(5, min(a.reps, 3000 // K))
                line = json.dumps(run(name, K, new, old, reps, a.warmup, hip, a.tag))
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
