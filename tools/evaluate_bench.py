#!/usr/bin/env python3
"""Som::evaluate on the device: one vsom_evaluate_batch call against the route it replaces.
One JSON line per shape (appended to --out, profiles/evaluate_bench.jsonl by default), rounds alternating between the routes
named in --route so that both see the same machine state:

  new     call_us    Context.evaluate(): search, scoring kernel, per-row results back, the running mean, one synchronise
          kernel_us  the scoring kernel's own time: the library's HIP-event timer around it (group "finish"), in a second
                     pass, so that the events do not sit in call_us
  parent  what Som::evaluate of the C++ mirror cost before, through symbols every earlier build has, bound with plain
          ctypes on --lib (the in-tree library, or a build of the parent commit): vsom_bmu_batch, vsom_get_state of the map
          (the mirror's refreshHost() downloads more: this is the least it could do), and the rows x C epilogue in numpy
          parent_us  all of it;  search_us  vsom_bmu_batch alone

Each shape runs with 10 columns flagged binary (all of them when J < 10).  Every shape is warmed up first; every figure is
the median wall time over --calls rounds with the 10th and 90th percentile beside it (*_p10, *_p90).

usage: tools/evaluate_bench.py [--route new,parent] [--lib FILE] [--tag TEXT] [--calls 30] [--shapes a,b] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {   # name: (W, H, J, rows)
    "ref20": (100, 100, 9, 20),            # the reference's own scenario: 100 x 100 x 9 over 20 rows
    "c3": (128, 128, 784, 4096),
}
NBINARY = 10


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def put(res, key, ts):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in stats_us(ts))


def state(W, H, J, rows, seed=42):
    """a map in (0,1), rows in [0,1] near it, NBINARY columns flagged binary, validity at 0.9"""
    rs = np.random.RandomState(seed)
    N = W * H
    m = rs.uniform(0.02, 0.98, (N, J)).astype(np.float32)
    X = np.clip(m[rs.randint(0, N, rows)] + rs.randn(rows, J).astype(np.float32) * np.float32(0.05), 0, 1).astype(np.float32)
    binary = np.zeros(J, np.float32)
    binary[rs.permutation(J)[:NBINARY]] = 1
    X[:, binary != 0] = np.round(X[:, binary != 0])
    valid = (rs.rand(rows, J) < 0.9).astype(np.uint8)
    return m, X, binary, np.ones(J, np.float32), valid


def epilogue(X, m, bmu, dist, binary, continuous, valid):
    """the rows x C walk of the earlier Som::evaluate, vectorised"""
    mm = m[bmu.astype(np.int64)]
    with np.errstate(all="ignore"):
        be = np.log(mm) * X + np.log(np.float32(1) - mm) * (np.float32(1) - X)
        be = np.where(np.isfinite(be), be, np.float32(-99999.0))
        t = be * binary * (valid * continuous)
        s = np.sqrt((t * t).sum(axis=1, dtype=np.float32).astype(np.float64))
    err = 0.0
    for i in range(X.shape[0]):
        err += 1.0 / (i + 1.0) * (float(dist[i]) + s[i] - err)
    return err


class Parent:
    def __init__(self, name, lib_path):
        W, H, J, rows = SHAPES[name]
        L = self.L = C.CDLL(lib_path)
        L.vsom_last_error.restype = C.c_char_p
        vp, fp, u64p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64)
        L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
        L.vsom_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
        L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
        L.vsom_bmu_batch.argtypes = [vp, u64p, fp]
        L.vsom_destroy.argtypes = [vp]
        L.vsom_destroy.restype = None
        self.m, self.X, self.binary, self.continuous, self.valid = state(W, H, J, rows)
        self.h = vp()
        self.ok(L.vsom_create(C.byref(self.h), 0, W, H, J, 0))
        self.ok(L.vsom_set_state(self.h, self.m.ctypes.data_as(fp), None, None, None, None))
        self.ok(L.vsom_upload_chunk(self.h, self.X.ctypes.data_as(fp), rows))
        self.hm = np.empty_like(self.m)
        self.bmu, self.dist = np.empty(rows, np.uint64), np.empty(rows, np.float32)
        self.fp, self.u64p = fp, u64p
        self.valf = self.valid.astype(np.float32)

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.vsom_last_error().decode())

    def search(self):
        self.ok(self.L.vsom_bmu_batch(self.h, self.bmu.ctypes.data_as(self.u64p), self.dist.ctypes.data_as(self.fp)))

    def call(self):
        self.search()
        self.ok(self.L.vsom_get_state(self.h, self.hm.ctypes.data_as(self.fp), None, None, None, None))
        return epilogue(self.X, self.hm, self.bmu, self.dist, self.binary, self.continuous, self.valf)

    def close(self):
        self.L.vsom_destroy(self.h)


class New:
    def __init__(self, name):
        import vsom_amd
        W, H, J, rows = SHAPES[name]
        self.m, self.X, self.binary, self.continuous, self.valid = state(W, H, J, rows)
        self.ctx = vsom_amd.Context(W, H, J, 0)
        self.ctx.set_state(map=self.m)
        self.ctx.upload_chunk(self.X)

    def call(self):
        return self.ctx.evaluate(self.binary, self.continuous, valid=self.valid)["error"]

    def kernel_times(self, calls):
        ctx = self.ctx
        ctx.enable_timing(True, groups=["finish"])
        ctx.get_timing(reset=True)
        ts = []
        for _ in range(calls):
            self.call()
            ms, cnt = ctx.get_timing(reset=True)["finish"]
            assert cnt == 1
            ts.append(ms * 1e-3)
        ctx.enable_timing(False)
        return ts

    def close(self):
        self.ctx.close()


def wall(fn):
    t0 = time.perf_counter()
    v = fn()
    return time.perf_counter() - t0, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="new,parent")
    ap.add_argument("--lib", default=os.path.join(ROOT, "variational-self-organizing-maps_amd", "libvsom_hip.so"))
    ap.add_argument("--tag", default="")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--shapes", default="ref20,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate_bench.jsonl"))
    a = ap.parse_args()
    routes = a.route.split(",")
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    for name in a.shapes.split(","):
        W, H, J, rows = SHAPES[name]
        new = New(name) if "new" in routes else None
        par = Parent(name, a.lib) if "parent" in routes else None
        res = {"shape": f"{W}x{H}x{J}", "rows": rows, "binary_columns": min(NBINARY, J), "routes": routes, "calls": a.calls}
        for _ in range(3):
            for r in (new, par):
                if r:
                    r.call()
        ts = {"call": [], "parent": [], "search": []}
        vals = {}
        for _ in range(a.calls):                       # the routes alternate
            if new:
                t, vals["new"] = wall(new.call)
                ts["call"].append(t)
            if par:
                t, vals["parent"] = wall(par.call)
                ts["parent"].append(t)
                ts["search"].append(wall(par.search)[0])
        for k, v in ts.items():
            if v:
                put(res, k, v)
        if new:
            put(res, "kernel", new.kernel_times(a.calls))
        res.update({"error_" + k: v for k, v in vals.items()})
        for r in (new, par):
            if r:
                r.close()
        if a.tag:
            res["tag"] = a.tag
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
