#!/usr/bin/env python3
"""The ensemble's masked queries against the calls they replace.

The workload is the reference's own smallest scenario (tests/performance/perf_tests.cpp:74-112) with missing fields: K
10x10x9 maps, each with the 20-row fixture loaded, about 11 % of the entries invalid (a NULL is stored as 0.0f with
valid = 0), K in --ks, all members on one stream.  Both queries ask for their dense output (fill, delta).  One JSON line
per K:

  bmu_new_us / sim_new_us        vsom_ensemble_bmu_masked_batch / vsom_ensemble_similarity_masked_batch of this build
  bmu_parent_us / sim_parent_us  what a caller had before them: K vsom_bmu_masked_batch / vsom_similarity_masked_batch calls
                                 on K separate contexts through --lib (a build of the parent commit; the in-tree library
                                 when none is given)
  unmasked_us                    vsom_ensemble_bmu_batch of this build on the same rows (a missing field taken for a zero)
  *_p10 / *_p90                  the 10th and 90th percentile over the timed rounds (the figures above are medians)
  bmu_vs_parent, sim_vs_parent   parent / new;   bmu_vs_unmasked   bmu_new_us / unmasked_us

Every call ends in a host wait and hands its results back, so the host clock around a call times the whole call.  --warmup
warm-up and --reps timed rounds per route, the routes timed alternately.  The parent routes of a large ensemble run
min(--reps, 3000 // K) timed rounds, at least 5 (parent_reps in the line).  Before any timing every output of the new
routes is compared with the parent routes' on the bits; a difference ends the run.

usage: tools/ensemble_masked_query_bench.py [--ks 16,256,1024] [--reps 30] [--warmup 3] [--lib FILE] [--tag TEXT] [--out FILE]"""
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
MIN_HITS, NUM_SIGMAS, SIGMA_FLOOR = 2, 3, 1
vp, fp, u64p, u8p, u32p = (C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8),
                           C.POINTER(C.c_uint32))
ip = C.POINTER(C.c_int)


class MaskedOut(C.Structure):
    _fields_ = [("bmu", u64p), ("dist", fp), ("nvalid", u32p), ("fill", fp)]


class SimilarityMaskedOut(C.Structure):
    _fields_ = [("bmu", u64p), ("dist", fp), ("dmax", fp), ("dmax_col", u32p), ("first", fp), ("amax", fp), ("amax_col", u32p),
                ("outside", u32p), ("delta", fp), ("nvalid", u32p)]


SHAPES = {"bmu": (), "dist": (), "nvalid": (), "fill": (J,), "dmax": (), "dmax_col": (), "first": (), "amax": (),
          "amax_col": (), "outside": (), "delta": (J,)}
DTYPES = {u64p: np.uint64, fp: np.float32, u32p: np.uint32}


def bind(path):
    L = C.CDLL(path)
    L.vsom_last_error.restype = C.c_char_p
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None
    L.vsom_set_stream.argtypes = [vp, vp]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_bmu_masked_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, u8p, C.c_int, C.POINTER(MaskedOut)]
    L.vsom_similarity_masked_batch.argtypes = [vp, C.c_uint64, C.c_int, C.c_int, C.c_size_t, C.c_size_t, u8p, C.c_int,
                                               C.POINTER(SimilarityMaskedOut)]
    L.vsom_ensemble_create.argtypes = [C.POINTER(vp), C.POINTER(vp), C.c_size_t]
    L.vsom_ensemble_destroy.argtypes = [vp]
    L.vsom_ensemble_destroy.restype = None
    L.vsom_ensemble_bmu_batch.argtypes = [vp, C.POINTER(u64p), C.POINTER(fp)]
    if hasattr(L, "vsom_ensemble_bmu_masked_batch"):
        L.vsom_ensemble_bmu_masked_batch.argtypes = [vp, u64p, C.POINTER(u8p), ip, C.POINTER(MaskedOut)]
        L.vsom_ensemble_similarity_masked_batch.argtypes = [vp, u64p, ip, C.c_int, C.POINTER(u8p), ip,
                                                            C.POINTER(SimilarityMaskedOut)]
    return L


def ok(L, rc):
    if rc != 0:
        raise SystemExit(f"libvsom_hip error {rc}: {L.vsom_last_error().decode(errors='replace')}")


def f32(a):
    return a.ctypes.data_as(fp)


class Side:
    """K contexts of one library on one stream with the rows loaded, their ensemble (ens), and the output arrays of both
    queries: an array of K structures whose pointers name rows of one numpy array per field"""

    def __init__(self, L, K, ens, stream, X, state):
        self.L, self.K = L, K
        self.h = []
        for k in range(K):
            h = vp()
            ok(L, L.vsom_create(C.byref(h), 0, W, H, J, 0))
            ok(L, L.vsom_set_stream(h, stream))
            m, s, hits = state[k]
            ok(L, L.vsom_set_state(h, f32(m), f32(s), None, None, hits.ctypes.data_as(u64p)))
            ok(L, L.vsom_upload_chunk(h, f32(X), B))
            self.h.append(h)
        self.ens = vp()
        if ens:
            ok(L, L.vsom_ensemble_create(C.byref(self.ens), (vp * K)(*[h.value for h in self.h]), K))
        self.res, self.outs = {}, {}
        for what, struct in (("bmu", MaskedOut), ("sim", SimilarityMaskedOut)):
            arrs = {name: np.zeros((K, B) + SHAPES[name], DTYPES[ct]) for name, ct in struct._fields_}
            outs = (struct * K)()
            for k in range(K):
                for name, ct in struct._fields_:
                    setattr(outs[k], name, arrs[name][k].ctypes.data_as(ct))
            self.res[what], self.outs[what] = arrs, outs
        self.idx, self.dist = np.zeros((K, B), np.uint64), np.zeros((K, B), np.float32)
        self.idxp = (u64p * K)(*[self.idx[k].ctypes.data_as(u64p) for k in range(K)])
        self.distp = (fp * K)(*[f32(self.dist[k]) for k in range(K)])

    def close(self):
        if self.ens:
            self.L.vsom_ensemble_destroy(self.ens)
        for h in self.h:
            self.L.vsom_destroy(h)


def same_bits(a, b):
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def run(K, new, old, reps, warmup, hip, tag):
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.ascontiguousarray(np.array(fx["rows"], np.float32))
    valid = np.ascontiguousarray(np.random.default_rng(5).random((B, J)) >= 0.11, dtype=np.uint8)
    Xz = np.ascontiguousarray(np.where(valid != 0, X, np.float32(0)))      # a NULL is stored as 0.0f with valid = 0
    rng = np.random.default_rng(7)
    state = [(gen.random_map(N, J, seed=100 + k), np.ascontiguousarray(rng.random((N, J)) * 0.2, dtype=np.float32),
              rng.integers(0, 6, N).astype(np.uint64)) for k in range(K)]
    stream = vp()
    assert hip.hipStreamCreate(C.byref(stream)) == 0
    a, b = Side(new, K, True, stream, Xz, state), Side(old, K, False, stream, Xz, state)
    vptr = valid.ctypes.data_as(u8p)
    vptrs = (u8p * K)(*([vptr] * K))
    mh = (C.c_uint64 * K)(*([MIN_HITS] * K))
    ns = (C.c_int * K)(*([NUM_SIGMAS] * K))
    bo, so = [b.outs["bmu"][k] for k in range(K)], [b.outs["sim"][k] for k in range(K)]     # (no bookkeeping in the timed region)

    def bmu_new():
        ok(new, new.vsom_ensemble_bmu_masked_batch(a.ens, mh, vptrs, None, a.outs["bmu"]))

    def sim_new():
        ok(new, new.vsom_ensemble_similarity_masked_batch(a.ens, mh, ns, SIGMA_FLOOR, vptrs, None, a.outs["sim"]))

    def bmu_parent():
        for k, h in enumerate(b.h):
            ok(old, old.vsom_bmu_masked_batch(h, MIN_HITS, 0, B, vptr, 0, C.byref(bo[k])))

    def sim_parent():
        for k, h in enumerate(b.h):
            ok(old, old.vsom_similarity_masked_batch(h, MIN_HITS, NUM_SIGMAS, SIGMA_FLOOR, 0, B, vptr, 0, C.byref(so[k])))

    def unmasked():
        ok(new, new.vsom_ensemble_bmu_batch(a.ens, a.idxp, a.distp))

    routes = (("bmu_new", bmu_new), ("bmu_parent", bmu_parent), ("sim_new", sim_new), ("sim_parent", sim_parent),
              ("unmasked", unmasked))
    for _, fn in routes:
        fn()
    for what in ("bmu", "sim"):
        for name in a.res[what]:
            if not same_bits(a.res[what][name], b.res[what][name]):
                raise SystemExit(f"K={K}: {what}.{name} differs from the parent route's")

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
    res = {"bench": "ensemble_masked_query", "tag": tag, "map": f"{W}x{H}x{J}", "rows": B,
           "invalid": round(float((valid == 0).mean()), 3), "K": K, "min_hits": MIN_HITS, "reps": reps, "parent_reps": preps,
           "bits_equal": True}
    for name, _ in routes:
        res[f"{name}_us"] = round(float(np.median(ts[name])), 1)
        res[f"{name}_us_p10"] = round(float(np.percentile(ts[name], 10)), 1)
        res[f"{name}_us_p90"] = round(float(np.percentile(ts[name], 90)), 1)
    res["bmu_new_per_map_us"] = round(res["bmu_new_us"] / K, 3)
    res["sim_new_per_map_us"] = round(res["sim_new_us"] / K, 3)
    res["bmu_vs_parent"] = round(res["bmu_parent_us"] / res["bmu_new_us"], 2)
    res["sim_vs_parent"] = round(res["sim_parent_us"] / res["sim_new_us"], 2)
    res["bmu_vs_unmasked"] = round(res["bmu_new_us"] / res["unmasked_us"], 2)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_masked_query_bench.jsonl"))
    a = ap.parse_args()
    new = bind(INTREE)
    old = new if os.path.abspath(a.lib) == os.path.abspath(INTREE) else bind(a.lib)
    new.vsom_device_count.restype = C.c_int
    if new.vsom_device_count() < 1:
        raise SystemExit("ensemble_masked_query_bench needs a GPU")
    hip = C.CDLL("libamdhip64.so")          # the runtime libvsom_hip.so runs on (its streams)
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamDestroy.argtypes = [vp]
    with open(a.out, "w") as out:
        for K in (int(k) for k in a.ks.split(",")):
            line = json.dumps(run(K, new, old, a.reps, a.warmup, hip, a.tag))
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
