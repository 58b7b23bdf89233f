#!/usr/bin/env python3
"""The ensemble's top-k calls against the calls they replace.

The workload is the reference's own smallest scenario (tests/performance/perf_tests.cpp:74-112): K 10x10x9 maps, each with
the 20-row fixture loaded, K in --ks, k in --topk, all members on one stream.  The masked routes see about 12 % of the
entries invalid (a NULL is stored as 0.0f with valid = 0) and min_hits = 2.  One JSON line per (K, k):

  plain_new_us / masked_new_us        vsom_ensemble_bmu_topk_batch / vsom_ensemble_bmu_topk_masked_batch of this build
  plain_parent_us / masked_parent_us  what a caller had before them: K vsom_bmu_topk_batch / vsom_bmu_topk_masked_batch calls
                                      on K separate contexts through --lib (a build of the parent commit; the in-tree
                                      library when none is given)
  bmu_us                              vsom_ensemble_bmu_batch of this build on the same rows (the search without the lists)
  *_p10 / *_p90                       the 10th and 90th percentile over the timed rounds (the figures above are medians)
  plain_vs_parent, masked_vs_parent   parent / new;   plain_vs_bmu   plain_new_us / bmu_us

Every call ends in a host wait and hands its results back, so the host clock around a call times the whole call.  --warmup
warm-up and --reps timed rounds per route, the routes timed alternately.  The parent routes of a large ensemble run
min(--reps, 3000 // K) timed rounds, at least 5 (parent_reps in the line).  Before any timing every output of the new
routes is compared with the parent routes' on the bits; a difference ends the run.

usage: tools/ensemble_topk_bench.py [--ks 16,256,1024] [--topk 2,16] [--reps 30] [--warmup 3] [--lib FILE] [--tag TEXT]
                                    [--out FILE]"""
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


class TopkMaskedOut(C.Structure):
    _fields_ = [("idx", u64p), ("dist", fp), ("count", u32p), ("nvalid", u32p), ("blend", dp)]


class EnsembleTopkOut(C.Structure):
    _fields_ = [("idx", u64p), ("dist", fp), ("count", u32p), ("nvalid", u32p)]


def bind(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    L.vsom_set_stream.argtypes = [vp, vp]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_bmu_topk_batch.argtypes = [vp, C.c_uint32, C.c_size_t, C.c_size_t, u64p, fp]
    L.vsom_bmu_topk_masked_batch.argtypes = [vp, C.c_uint32, C.c_uint64, C.c_size_t, C.c_size_t, u8p, C.c_int,
                                             C.POINTER(TopkMaskedOut)]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_bmu_batch.argtypes = [vp, C.POINTER(u64p), C.POINTER(fp)]
    if hasattr(L, "vsom_ensemble_bmu_topk_batch"):
        L.vsom_ensemble_bmu_topk_batch.argtypes = [vp, u32p, C.POINTER(EnsembleTopkOut)]
        L.vsom_ensemble_bmu_topk_masked_batch.argtypes = [vp, u32p, u64p, C.POINTER(u8p), ip, C.POINTER(EnsembleTopkOut)]
    return L


def ok(L, rc):
    if rc != 0:
        raise SystemExit(f"libvsom_hip error {rc}: {L.vsom_last_error().decode(errors='replace')}")


def f32(a):
    return a.ctypes.data_as(fp)


class Side:
    """K contexts of one library on one stream with the rows loaded, and their ensemble (ens)"""

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

    def outputs(self, k):
        """the arrays of both routes (plain, masked) for lists of k, and the structures over them"""
        self.res = {what: {"idx": np.zeros((self.K, B, k), np.uint64), "dist": np.zeros((self.K, B, k), np.float32),
                           "count": np.zeros((self.K, B), np.uint32), "nvalid": np.zeros((self.K, B), np.uint32)}
                    for what in ("plain", "masked")}
        self.ens_outs, self.single_outs = {}, {}
        for what, arrs in self.res.items():
            eo, so = (EnsembleTopkOut * self.K)(), [TopkMaskedOut() for _ in range(self.K)]
            for m in range(self.K):
                for o in (eo[m], so[m]):
                    for name, ct in EnsembleTopkOut._fields_:
                        setattr(o, name, arrs[name][m].ctypes.data_as(ct))
            self.ens_outs[what], self.single_outs[what] = eo, so

    def close(self):
        if self.ens:
            self.L.vsom_ensemble_destroy(self.ens)
        for h in self.h:
            self.L.vsom_destroy(h)


def same_bits(a, b):
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def run(K, topk, new, old, reps, warmup, hip, tag):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.ascontiguousarray(np.array(fx["rows"], np.float32))
    valid = np.ascontiguousarray(np.random.default_rng(5).random((B, J)) >= 0.12, dtype=np.uint8)
    Xz = np.ascontiguousarray(np.where(valid != 0, X, np.float32(0)))      # a NULL is stored as 0.0f with valid = 0
    rng = np.random.default_rng(7)
    state = [(gen.random_map(N, J, seed=100 + k), rng.integers(0, 6, N).astype(np.uint64)) for k in range(K)]
    stream = vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    a, b = Side(new, K, True, stream, Xz, state), Side(old, K, False, stream, Xz, state)
    vptr = valid.ctypes.data_as(u8p)
    vptrs = (u8p * K)(*([vptr] * K))
    mh = (C.c_uint64 * K)(*([MIN_HITS] * K))
    idx, dist = np.zeros((K, B), np.uint64), np.zeros((K, B), np.float32)
    idxp = (u64p * K)(*[idx[m].ctypes.data_as(u64p) for m in range(K)])
    distp = (fp * K)(*[f32(dist[m]) for m in range(K)])
    for k in topk:
        a.outputs(k)
        b.outputs(k)
        ks = (C.c_uint32 * K)(*([k] * K))
        pi, pd = b.res["plain"]["idx"], b.res["plain"]["dist"]
        pidx = [pi[m].ctypes.data_as(u64p) for m in range(K)]             # (no bookkeeping in the timed region)
        pdist = [f32(pd[m]) for m in range(K)]
        mo = b.single_outs["masked"]

        def plain_new():
            ok(new, new.vsom_ensemble_bmu_topk_batch(a.ens, ks, a.ens_outs["plain"]))

        def masked_new():
            ok(new, new.vsom_ensemble_bmu_topk_masked_batch(a.ens, ks, mh, vptrs, None, a.ens_outs["masked"]))

        def plain_parent():
            for m, h in enumerate(b.h):
                ok(old, old.vsom_bmu_topk_batch(h, k, 0, B, pidx[m], pdist[m]))

        def masked_parent():
            for m, h in enumerate(b.h):
                ok(old, old.vsom_bmu_topk_masked_batch(h, k, MIN_HITS, 0, B, vptr, 0, C.byref(mo[m])))

        def bmu():
            ok(new, new.vsom_ensemble_bmu_batch(a.ens, idxp, distp))

        routes = (("plain_new", plain_new), ("plain_parent", plain_parent), ("masked_new", masked_new),
                  ("masked_parent", masked_parent), ("bmu", bmu))
        for _, fn in routes:
            fn()
        for what, names in (("plain", ("idx", "dist")), ("masked", ("idx", "dist", "count", "nvalid"))):
            for name in names:
                if not same_bits(a.res[what][name], b.res[what][name]):
                    raise SystemExit(f"K={K}, k={k}: {what}.{name} differs from the parent route's")

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
        res = {"bench": "ensemble_topk", "tag": tag, "map": f"{W}x{H}x{J}", "rows": B,
               "invalid": round(float((valid == 0).mean()), 3), "K": K, "k": k, "min_hits": MIN_HITS, "reps": reps,
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
        yield res
    for s in (a, b):
        s.close()
    hip.hipStreamDestroy(stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="16,256,1024")
    ap.add_argument("--topk", default="2,16")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lib", default=INTREE, help="the library the parent routes run on (a build of the parent commit)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_topk_bench.jsonl"))
    a = ap.parse_args()
    new = bind(INTREE)
    old = new if os.path.abspath(a.lib) == os.path.abspath(INTREE) else bind(a.lib)
    new.vsom_device_count.restype = C.c_int
    if new.vsom_device_count() < 1:
        raise SystemExit("ensemble_topk_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    topk = [int(k) for k in a.topk.split(",")]
    with open(a.out, "w") as out:
        for K in (int(k) for k in a.ks.split(",")):
            for res in run(K, topk, new, old, a.reps, a.warmup, hip, a.tag):
                line = json.dumps(res)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
