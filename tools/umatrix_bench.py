#!/usr/bin/env python3
"""Som::updateUMatrix on the device: one vsom_umatrix call against the route it replaces.  One JSON line per shape
(appended to --out, profiles/umatrix_bench.jsonl by default):

  --route new     call_us        Context.umatrix(): one launch, the N doubles back, one synchronise
                  kernel_us      the kernel's own time: HIP events around the enqueue-only form
                  copy_fraction  the algorithmic bytes (2 N pitch 4 + 8 N) over kernel_us as a fraction of the measured
                                 6.29 TB/s copy rate
                  ensemble shape (the members share one stream): call_us = 256 Context.umatrix() calls,
                  ensemble_call_us = one Ensemble.umatrix()
  --route pairs   pairs_us       vsom_distances_raw over the (node, neighbour) pair list, built once outside the timed
                                 region: the C-ABI part of the earlier route (its host combination is not in it).
                                 --lib names the library to time it on (a build of the parent commit), bound here with
                                 plain ctypes: only symbols the parent has.  ensemble shape: 256 such calls.

Every shape is warmed up first; every figure is the median wall time of --calls calls, each ending in a synchronise,
with the 10th and 90th percentile beside it (*_p10, *_p90).  Kernel traces come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.

usage: tools/umatrix_bench.py [--route new|pairs] [--lib FILE] [--tag TEXT] [--calls 50] [--shapes a,b] [--out FILE]"""
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
SHAPES = {   # name: (W, H, J, transform, members)
    "small": (10, 10, 9, 0, 1),
    "clr72": (100, 100, 9, 2, 1),          # the reference's own scenario: a 100 x 100 CLR map of depth 72
    "mid": (64, 64, 784, 0, 1),
    "c3": (128, 128, 784, 0, 1),
    "ensemble": (10, 10, 9, 0, 256),
}


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return stats_us(ts)


def put(res, key, st):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in st)


def state(W, H, J, tr, seed):
    D = J * (J - 1) if tr == 2 else J
    rs = np.random.RandomState(seed)
    return gen.random_map(W * H, D, seed=seed), (rs.rand(W * H, D) * 0.5 + 0.01).astype(np.float32)


def pair_list(W, H):
    DI, DJ = (0, 0, 1, -1, -1, 1, -1, 1), (-1, 1, 0, 0, -1, -1, 1, 1)
    nodes, nbrs = [], []
    for i in range(H):
        for j in range(W):
            for k in range(8):
                ni, nj = i + DI[k], j + DJ[k]
                if 0 <= ni < H and 0 <= nj < W:
                    nodes.append(i * W + j)
                    nbrs.append(ni * W + nj)
    return np.array(nodes, np.uint64), np.array(nbrs, np.uint64)


def label(W, H, J, tr):
    return f"{W}x{H}x{J}" + (f" clr (depth {J * (J - 1)})" if tr == 2 else "")


def run_pairs(name, calls, lib_path):
    W, H, J, tr, members = SHAPES[name]
    L = C.CDLL(lib_path)
    L.vsom_last_error.restype = C.c_char_p
    vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
    L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
    L.vsom_distances_raw.argtypes = [vp, u64p, u64p, C.c_size_t, C.c_int, fp]
    L.vsom_destroy.argtypes = [vp]
    L.vsom_destroy.restype = None

    def ok(rc):
        if rc:
            raise RuntimeError(L.vsom_last_error().decode())

    nodes, nbrs = pair_list(W, H)
    d = np.empty(nodes.size, np.float32)
    np_, bp, dp = nodes.ctypes.data_as(u64p), nbrs.ctypes.data_as(u64p), d.ctypes.data_as(fp)
    hs = []
    for k in range(members):
        h = vp()
        ok(L.vsom_create(C.byref(h), 0, W, H, J, tr))
        m, s = state(W, H, J, tr, 42 + k)
        ok(L.vsom_set_state(h, m.ctypes.data_as(fp), s.ctypes.data_as(fp), None, None, None))
        hs.append(h)

    def call():
        for h in hs:
            ok(L.vsom_distances_raw(h, np_, bp, nodes.size, 1, dp))

    for _ in range(3):
        call()
    res = {"shape": label(W, H, J, tr), "members": members, "route": "pairs", "pairs": int(nodes.size), "calls": calls}
    put(res, "pairs", timed(call, calls))
    for h in hs:
        L.vsom_destroy(h)
    return res


def run_new(name, calls):
    import torch
    import vsom_amd
    W, H, J, tr, members = SHAPES[name]
    ctxs = []
    for k in range(members):
        ctx = vsom_amd.Context(W, H, J, tr)
        m, s = state(W, H, J, tr, 42 + k)
        ctx.set_state(map=m, sigma=s)
        ctxs.append(ctx)
    c0 = ctxs[0]
    stream = torch.cuda.Stream()
    if members > 1:          # the ensemble's fast form: every member on ONE stream (include/vsom_hip.h)
        for c in ctxs:
            c.set_stream(stream.cuda_stream)
    res = {"shape": label(W, H, J, tr), "members": members, "route": "new", "calls": calls}

    def singles():
        for c in ctxs:
            c.umatrix()

    for _ in range(3):
        singles()
    put(res, "call", timed(singles, calls))
    if members > 1:
        ens = vsom_amd.Ensemble(ctxs)
        for _ in range(3):
            ens.umatrix()
        put(res, "ensemble_call", timed(ens.umatrix, calls))
        res["singles_over_ensemble"] = round(res["call_us"] / res["ensemble_call_us"], 2)
        ens.close()
        for c in ctxs:
            c.synchronize()
            c.set_stream(None)
    else:
        c0.set_stream(stream.cuda_stream)
        ts = []
        for _ in range(calls + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            c0.umatrix(fetch=False)
            b.record(stream)
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3)
        put(res, "kernel", stats_us(ts[3:]))
        c0.synchronize()
        c0.set_stream(None)
        nbytes = 2 * W * H * c0.pitch * 4 + 8 * W * H
        res["bytes"] = nbytes
        res["copy_fraction"] = round(nbytes / COPY_RATE / (res["kernel_us"] * 1e-6), 4)
    for c in ctxs:
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="new", choices=["new", "pairs"])
    ap.add_argument("--lib", default=os.path.join(ROOT, "variational-self-organizing-maps_amd", "libvsom_hip.so"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--shapes", default="small,clr72,mid,c3,ensemble")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umatrix_bench.jsonl"))
    a = ap.parse_args()
    for name in a.shapes.split(","):
        res = run_new(name, a.calls) if a.route == "new" else run_pairs(name, a.calls, a.lib)
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
