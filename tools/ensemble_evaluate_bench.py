#!/usr/bin/env python3
"""The ensemble's evaluate calls against the calls they replace.

The workload is the reference's own smallest scenario (tests/performance/perf_tests.cpp:74-112): K 10x10x9 maps, each with
the 20-row fixture loaded, K in --ks, all members on one stream, two binary columns (the first and the last; every column
continuous).  The masked routes see about 12 % of the entries invalid (a NULL is stored as 0.0f with valid = 0) and
min_hits = 2.  One JSON line per K:

  plain_new_us / masked_new_us        vsom_ensemble_evaluate_batch / vsom_ensemble_evaluate_masked_batch of this build
  plain_parent_us / masked_parent_us  what a caller had before them: K vsom_evaluate_batch / vsom_evaluate_masked_batch calls
                                      on K separate contexts through --lib (a build of the parent commit; the in-tree
                                      library when none is given)
  bmu_us / bmu_masked_us              vsom_ensemble_bmu_batch / vsom_ensemble_bmu_masked_batch of this build on the same rows
                                      (the search alone)
  *_p10 / *_p90                       the 10th and 90th percentile over the timed rounds (the figures above are medians)
  plain_vs_parent, masked_vs_parent   parent / new;   plain_vs_bmu, masked_vs_bmu   new / the search alone

Every call ends in a host wait and hands its results back, so the host clock around a call times the whole call.  --warmup
warm-up and --reps timed rounds per route, the routes timed alternately.  The parent routes of a large ensemble run
min(--reps, 3000 // K) timed rounds, at least 5 (parent_reps in the line).  Before any timing every output of the new
routes is compared with the parent routes' on the bits; a difference ends the run.  The one condition the issue sets --
at K = 16 the one call is not slower than the 16 single calls -- is recorded as k16_not_slower in that line.

usage: tools/ensemble_evaluate_bench.py [--ks 16,256,1024] [--reps 30] [--warmup 3] [--lib FILE] [--tag TEXT] [--out FILE]"""
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
MIN_HITS = 2
vp, fp, u64p, u8p, u32p = (C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
                           C.POINTER(C.c_uint32))
ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)


class EvaluateOut(C.Structure):
    _fields_ = [("bmu", u64p), ("dist", fp), ("bsum", fp), ("nrepl", u32p), ("error", dp)]


class EvaluateMaskedOut(C.Structure):
    _fields_ = EvaluateOut._fields_ + [("nvalid", u32p)]


class MaskedOut(C.Structure):
    _fields_ = [("bmu", u64p), ("dist", fp), ("nvalid", u32p), ("fill", fp)]


def bind(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    L.vsom_set_stream.argtypes = [vp, vp]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_evaluate_batch.argtypes = [vp, C.c_size_t, C.c_size_t, fp, fp, u8p, C.POINTER(EvaluateOut)]
    L.vsom_evaluate_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, fp, fp, u8p, C.c_int,
                                             C.POINTER(EvaluateMaskedOut)]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_bmu_batch.argtypes = [vp, C.POINTER(u64p), C.POINTER(fp)]
    L.vsom_ensemble_bmu_masked_batch.argtypes = [vp, u64p, C.POINTER(u8p), ip, C.POINTER(MaskedOut)]
    if hasattr(L, "vsom_ensemble_evaluate_batch"):
        L.vsom_ensemble_evaluate_batch.argtypes = [vp, C.POINTER(fp), C.POINTER(fp), C.POINTER(u8p), C.POINTER(EvaluateOut)]
        L.vsom_ensemble_evaluate_masked_batch.argtypes = [vp, u64p, C.POINTER(fp), C.POINTER(fp), C.POINTER(u8p), ip,
                                                          C.POINTER(EvaluateMaskedOut)]
    return L


def ok(L, rc):
    if rc != 0:
        raise SystemExit(f"libvsom_hip error {rc}: {L.vsom_last_error().decode(errors='replace')}")


def f32(a):
    return a.ctypes.data_as(fp)


FIELDS = {"bmu": np.uint64, "dist": np.float32, "bsum": np.float32, "nrepl": np.uint32, "nvalid": np.uint32}


class Side:
    """K contexts of one library on one stream with the rows loaded, their ensemble (ens), and the output arrays of both
    routes with one structure per member over them"""

    def __init__(self, L, K, ens, stream, X, state):
        self.L, self.K = L, K
        self.h = []
        for k in range(K):
            h = vp()
            ok(L, L.vsom_create(C.byref(h), 0, W, H, J, 0))
            ok(L, L.vsom_set_stream(h, stream))
            m, hits = state[k]
            ok(L, L.vsom_set_state(h, f32(m), None, None, None, hits.ctypes.data_as(u64p)))
            ok(L, L.vsom_upload_chunk(h, f32(X), B))
            self.h.append(h)
        self.ens = vp()
        if ens:
            ok(L, L.vsom_ensemble_create(C.byref(self.ens), (vp * K)(*[h.value for h in self.h]), K))
        self.res = {what: dict({name: np.zeros((K, B), t) for name, t in FIELDS.items()}, error=np.zeros(K, np.float64))
                    for what in ("plain", "masked")}
        self.outs = {"plain": (EvaluateOut * K)(), "masked": (EvaluateMaskedOut * K)()}
        for what, outs in self.outs.items():
            for m in range(K):
                for name, ct in outs[m]._fields_:
                    arr = self.res[what][name]
                    setattr(outs[m], name, arr[m:m + 1].ctypes.data_as(ct) if name == "error" else arr[m].ctypes.data_as(ct))

    def close(self):
        if self.ens:
            self.L.vsom_ensemble_destroy(self.ens)
        for h in self.h:
            self.L.vsom_destroy(h)


def same_bits(a, b):
    if a.dtype.kind == "f":
        u = np.uint32 if a.dtype == np.float32 else np.uint64
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def run(K, new, old, reps, warmup, hip, tag):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.ascontiguousarray(np.array(fx["rows"], np.float32))
    valid = np.ascontiguousarray(np.random.default_rng(5).random((B, J)) >= 0.12, dtype=np.uint8)
    Xz = np.ascontiguousarray(np.where(valid != 0, X, np.float32(0)))      # a NULL is stored as 0.0f with valid = 0
    binary = np.zeros(J, np.float32)
    binary[[0, J - 1]] = 1                                                 # two binary columns
    continuous = np.ones(J, np.float32)
    rng = np.random.default_rng(7)
    # maps in (0, 1): the binary error is a finite number, as on a trained map of [0, 1] data
    state = [(np.ascontiguousarray(np.clip(gen.random_map(N, J, seed=100 + k), 0.02, 0.98), dtype=np.float32),
              rng.integers(0, 6, N).astype(np.uint64)) for k in range(K)]
    stream = vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    a, b = Side(new, K, True, stream, Xz, state), Side(old, K, False, stream, Xz, state)
    vptr, bptr, cptr = valid.ctypes.data_as(u8p), f32(binary), f32(continuous)
    vptrs = (u8p * K)(*([vptr] * K))
    bptrs, cptrs = (fp * K)(*([bptr] * K)), (fp * K)(*([cptr] * K))
    mh = (C.c_uint64 * K)(*([MIN_HITS] * K))
    idx, dist, nv = np.zeros((K, B), np.uint64), np.zeros((K, B), np.float32), np.zeros((K, B), np.uint32)
    idxp = (u64p * K)(*[idx[m].ctypes.data_as(u64p) for m in range(K)])
    distp = (fp * K)(*[f32(dist[m]) for m in range(K)])
    bmo = (MaskedOut * K)()
    for m in range(K):
        bmo[m].bmu, bmo[m].dist, bmo[m].nvalid = idxp[m], distp[m], nv[m].ctypes.data_as(u32p)
    po, mo = b.outs["plain"], b.outs["masked"]

    def plain_new():
        ok(new, new.vsom_ensemble_evaluate_batch(a.ens, bptrs, cptrs, None, a.outs["plain"]))

    def masked_new():
        ok(new, new.vsom_ensemble_evaluate_masked_batch(a.ens, mh, bptrs, cptrs, vptrs, None, a.outs["masked"]))

    def plain_parent():
        for m, h in enumerate(b.h):
            ok(old, old.vsom_evaluate_batch(h, 0, B, bptr, cptr, None, C.byref(po[m])))

    def masked_parent():
        for m, h in enumerate(b.h):
            ok(old, old.vsom_evaluate_masked_batch(h, MIN_HITS, 0, B, bptr, cptr, vptr, 0, C.byref(mo[m])))

    def bmu():
        ok(new, new.vsom_ensemble_bmu_batch(a.ens, idxp, distp))

    def bmu_masked():
        ok(new, new.vsom_ensemble_bmu_masked_batch(a.ens, mh, vptrs, None, bmo))

    routes = (("plain_new", plain_new), ("plain_parent", plain_parent), ("masked_new", masked_new),
              ("masked_parent", masked_parent), ("bmu", bmu), ("bmu_masked", bmu_masked))
    for _, fn in routes:
        fn()
    for what, names in (("plain", ("bmu", "dist", "bsum", "nrepl", "error")),
                        ("masked", ("bmu", "dist", "bsum", "nrepl", "nvalid", "error"))):
        for name in names:
            if not same_bits(a.res[what][name], b.res[what][name]):
                raise SystemExit(f"K={K}: {what}.{name} differs from the parent route's")
    if not (a.res["plain"]["bsum"] > 0).any() or not np.isfinite(a.res["plain"]["error"]).all():
        raise SystemExit(f"K={K}: the workload scores nothing")

    preps = max(5, min(reps, 3000 // K))
    ts = {name: [] for name, _ in routes}
    for rep in range(warmup + reps):
        for name, fn in routes:
            if name.endswith("parent") and rep >= warmup + preps:
                continue
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if rep >= warmup:
                ts[name].append(dt * 1e6)
    res = {"bench": "ensemble_evaluate", "tag": tag, "map": f"{W}x{H}x{J}", "rows": B, "binary_columns": 2,
           "invalid": round(float((valid == 0).mean()), 3), "K": K, "min_hits": MIN_HITS, "reps": reps,
           "parent_reps": preps, "bits_equal": True}
    for name, _ in routes:
        res[f"{name}_us"] = round(float(np.median(ts[name])), 1)
        res[f"{name}_us_p10"] = round(float(np.percentile(ts[name], 10)), 1)
        res[f"{name}_us_p90"] = round(float(np.percentile(ts[name], 90)), 1)
    res["plain_new_per_map_us"] = round(res["plain_new_us"] / K, 3)
    res["masked_new_per_map_us"] = round(res["masked_new_us"] / K, 3)
    res["plain_vs_parent"] = round(res["plain_parent_us"] / res["plain_new_us"], 2)
    res["masked_vs_parent"] = round(res["masked_parent_us"] / res["masked_new_us"], 2)
    res["plain_vs_bmu"] = round(res["plain_new_us"] / res["bmu_us"], 2)
    res["masked_vs_bmu"] = round(res["masked_new_us"] / res["bmu_masked_us"], 2)
    if K == 16:
        res["k16_not_slower"] = bool(res["plain_new_us"] <= res["plain_parent_us"] and
                                     res["masked_new_us"] <= res["masked_parent_us"])
    for s in (a, b):
        s.close()
    hip.hipStreamDestroy(stream)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,256,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=INTREE, help="the library the parent routes run on (a build of the parent commit)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_evaluate_bench.jsonl"))
    a = ap.parse_args()
    new = bind(INTREE)
    old = new if os.path.abspath(a.lib) == os.path.abspath(INTREE) else bind(a.lib)
    new.vsom_device_count.restype = C.c_int
    if new.vsom_device_count() < 1:
        raise SystemExit("ensemble_evaluate_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    failed = False
    with open(a.out, "w") as out:
        for K in (int(k) for k in a.ks.split(",")):
            res = run(K, new, old, a.reps, a.warmup, hip, a.tag)
            line = json.dumps(res)
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            failed = failed or res.get("k16_not_slower") is False
    if failed:
        raise SystemExit("at K = 16 the one call is slower than the 16 single calls of --lib")


if __name__ == "__main__":
    main()
