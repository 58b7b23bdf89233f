#!/usr/bin/env python3
"""Som::measureSimilarity's per-row report on the device: one vsom_similarity_batch call against the route it replaces.
One JSON line per (shape, min_hits) (appended to --out, profiles/similarity_bench.jsonl by default):

  --route new     call_us        Context.similarity(): search, scoring kernel, per-row results back, one synchronise
                  kernel_us      the scoring kernel's own time: the library's HIP-event timer around it (group "finish"),
                                 in a second pass, so that the events do not sit in call_us
                  copy_fraction  the algorithmic bytes (12 C rows + 36 rows) over kernel_us as a fraction of the measured
                                 6.29 TB/s copy rate -- reported, not gated: a gather of this size sits well below it
  --route parent  what Som::measureSimilarity cost before, through symbols the parent commit has, bound here with plain
                  ctypes on --lib (a build of the parent commit): vsom_bmu_restricted_batch, then
                  dirty_us   vsom_get_state of map and sigma (one vsom_set_state of hits between calls, outside the timed
                             region, stands for the training step that dirtied the host mirror) + the B x C epilogue in numpy
                  clean_us   the same without the download (the host mirror is current)

Every shape is warmed up first; every figure is the median wall time of --calls calls with the 10th and 90th percentile
beside it (*_p10, *_p90).

usage: tools/similarity_bench.py [--route new|parent] [--lib FILE] [--tag TEXT] [--calls 30] [--shapes a,b] [--out FILE]"""
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

COPY_RATE = 6.29e12     # bytes / s: the device-to-device copy rate measured on MI355X
SHAPES = {   # name: (W, H, J, rows)
    "ref20": (100, 100, 9, 20),            # the reference's own scenario: 100 x 100 x 9 over 20 rows
    "mid": (64, 64, 784, 4096),
    "c3": (128, 128, 784, 4096),
}
NUM_SIGMAS = 3


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def timed(fn, calls, between=None):
    ts = []
    for _ in range(calls):
        if between:
            between()
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats_us(ts)


def put(res, key, st):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in st)


def state(W, H, J, rows, seed=42):
    """a map, a sigmaMap around the 1e-5 select, hit counts of which a third are 0, and rows near the map"""
    rs = np.random.RandomState(seed)
    N = W * H
    m = gen.random_map(N, J, seed=seed)
    s = (rs.rand(N, J) * 2e-5).astype(np.float32)
    hits = (rs.randint(0, 3, N)).astype(np.uint64)
    X = (m[rs.randint(0, N, rows)] + rs.randn(rows, J).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    return m, s, hits, X


def epilogue(X, m, s, bmu, k):
    """the B x C walk of the earlier Som::measureSimilarity, vectorised: delta, the interval test, the running maximum"""
    b = bmu.astype(np.int64)
    mm, ss = m[b], s[b]
    with np.errstate(all="ignore"):
        sM = np.where(ss > np.float32(1e-5), np.float32(1e-5), ss)
        delta = (X - mm) / sM / np.float32(k)
        sk = sM * np.float32(k)
        outside = ((X < mm - sk) | (X > mm + sk)).sum(axis=1)
        dmax = np.nanmax(delta, axis=1)
    return int(np.argmax(dmax)), outside


def run_parent(name, min_hits, calls, lib_path):
    W, H, J, rows = SHAPES[name]
    L = C.CDLL(lib_path)
    L.vsom_last_error.restype = C.c_char_p
    vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
    L.vsom_bmu_restricted_batch.argtypes = [vp, C.c_uint64, u64p, fp]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None

    def ok(rc):
        if rc:
            raise RuntimeError(L.vsom_last_error().decode())

    m, s, hits, X = state(W, H, J, rows)
    h = vp()
    ok(L.vsom_create(C.byref(h), 0, W, H, J, 0))
    ok(L.vsom_set_state(h, m.ctypes.data_as(fp), s.ctypes.data_as(fp), None, None, hits.ctypes.data_as(u64p)))
    ok(L.vsom_upload_chunk(h, X.ctypes.data_as(fp), rows))
    hm, hs = np.empty_like(m), np.empty_like(s)
    bmu = np.empty(rows, np.uint64)

    def clean():
        ok(L.vsom_bmu_restricted_batch(h, min_hits, bmu.ctypes.data_as(u64p), None))
        return epilogue(X, hm, hs, bmu, NUM_SIGMAS)

    def dirty():
        ok(L.vsom_bmu_restricted_batch(h, min_hits, bmu.ctypes.data_as(u64p), None))
        ok(L.vsom_get_state(h, hm.ctypes.data_as(fp), hs.ctypes.data_as(fp), None, None, None))
        return epilogue(X, hm, hs, bmu, NUM_SIGMAS)

    def touch():
        ok(L.vsom_set_state(h, None, None, None, None, hits.ctypes.data_as(u64p)))

    for _ in range(3):
        dirty()
    res = {"shape": f"{W}x{H}x{J}", "rows": rows, "min_hits": min_hits, "route": "parent", "calls": calls}
    put(res, "dirty", timed(dirty, calls, touch))
    put(res, "clean", timed(clean, calls))
    L.vsom_destroy(h)
    return res


def run_new(name, min_hits, calls):
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    import vsom_amd
    from vsom_amd import capi
    W, H, J, rows = SHAPES[name]
    m, s, hits, X = state(W, H, J, rows)
    ctx = vsom_amd.Context(W, H, J, 0)
    ctx.set_state(map=m, sigma=s, hits=hits)
    ctx.upload_chunk(X)

    def call():
        return ctx.similarity(min_hits, NUM_SIGMAS, capi.SIGMA_AS_WRITTEN)

    for _ in range(3):
        call()
    res = {"shape": f"{W}x{H}x{J}", "rows": rows, "min_hits": min_hits, "route": "new", "calls": calls}
    put(res, "call", timed(call, calls))
    ctx.enable_timing(True, groups=["finish"])
    ctx.get_timing(reset=True)
    ts = []
    for _ in range(calls):
        call()
        ms, cnt = ctx.get_timing(reset=True)["finish"]
        assert cnt == 1
        ts.append(ms * 1e-3)
    ctx.enable_timing(False)
    put(res, "kernel", stats_us(ts))
    Cc = min(J, ctx.depth)
    nbytes = 12 * Cc * rows + 36 * rows
    res["bytes"] = nbytes
    res["copy_fraction"] = round(nbytes / COPY_RATE / (res["kernel_us"] * 1e-6), 4)
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="new", choices=["new", "parent"])
    ap.add_argument("--lib", default=os.path.join(ROOT, "variational-self-organizing-maps_amd", "libvsom_hip.so"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--shapes", default="ref20,mid,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity_bench.jsonl"))
    a = ap.parse_args()
    for name in a.shapes.split(","):
        for min_hits in (0, 1):
            res = run_new(name, min_hits, a.calls) if a.route == "new" else run_parent(name, min_hits, a.calls, a.lib)
            if a.tag:
                res["tag"] = a.tag
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
