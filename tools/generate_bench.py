#!/usr/bin/env python3
"""Som::autoEncoder's records on the device: one vsom_generate_batch call against the route the earlier library offers.
One JSON line per shape (appended to --out, profiles/generate_bench.jsonl by default), rounds alternating between the routes
named in --route so that both see the same machine state:

  new     call_us    Context.generate(GENERATE_AS_WRITTEN): the last row's distribution, one draw per row, the decode, units
                     and records back, one synchronise (the chunk is staged once, outside the timing, as Som::autoEncoder's
                     one upload is a vsom_upload_chunk both routes know)
          draw_us, decode_us  the draw launches' and the decode kernel's own time: the library's HIP-event timers (groups
                     "bmu" and "finish"), in a second pass, so that the events do not sit in call_us
  parent  what Som::autoEncoder of the C++ mirror did before, through symbols every earlier build has, bound with plain
          ctypes on --lib (the in-tree library, or a build of the parent commit): per row one vsom_upload_chunk of the last
          row and one vsom_bmd_batch on it, then ONE vsom_get_state of map and sigmaMap (the mirror's refreshHost()
          downloads once and keeps it) and the rows x C epilogue in numpy
          parent_us  all of it

Every shape is warmed up first; every figure is the median wall time over --calls rounds with the 10th and 90th percentile
beside it (*_p10, *_p90).  --parent-calls limits the rounds of the parent route (its per-row calls make it slow).

usage: tools/generate_bench.py [--route new,parent] [--lib FILE] [--tag TEXT] [--calls 30] [--parent-calls 5] [--shapes a,b]
                               [--out FILE]"""
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
MIN_HITS = 1


def stats_us(ts):
    ts = np.asarray(ts) * 1e6
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def put(res, key, ts):
    res[key + "_us"], res[key + "_p10"], res[key + "_p90"] = (round(v, 2) for v in stats_us(ts))


def state(W, H, J, rows, seed=42):
    """a map in (0,1) with rows near it (scaled so that a row keeps mass on many nodes), sigma, hits, uniforms and L"""
    rs = np.random.RandomState(seed)
    N = W * H
    scale = np.float32(1.0 / np.sqrt(J))
    m = (rs.uniform(0.02, 0.98, (N, J)) * scale).astype(np.float32)
    X = (m[rs.randint(0, N, rows)] + rs.randn(rows, J).astype(np.float32) * np.float32(0.05) * scale).astype(np.float32)
    s = rs.uniform(0.05, 0.3, (N, J)).astype(np.float32)
    hits = rs.randint(0, 5, N).astype(np.uint64)
    u = rs.rand(rows)
    L = rs.randint(1, 1000, (rows, J)).astype(np.float64) / 1000.0
    return m, s, hits, X, u, L


class Parent:
    def __init__(self, name, lib_path):
        W, H, J, rows = SHAPES[name]
        L = self.L = C.CDLL(lib_path)
        L.vsom_last_error.restype = C.c_char_p
        vp, fp, u64p, dp = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        L.vsom_create.argtypes = [C.POINTER(vp), C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.vsom_set_state.argtypes = [vp, fp, fp, fp, fp, u64p]
        L.vsom_get_state.argtypes = [vp, fp, fp, fp, fp, u64p]
        L.vsom_upload_chunk.argtypes = [vp, fp, C.c_size_t]
        L.vsom_bmd_batch.argtypes = [vp, C.c_uint64, C.c_size_t, C.c_size_t, dp, u64p, dp, dp]
        L.vsom_destroy.argtypes = [vp]
        L.vsom_destroy.restype = None
        self.m, self.s, self.hits, self.X, self.u, self.Lg = state(W, H, J, rows)
        self.h = vp()
        self.ok(L.vsom_create(C.byref(self.h), 0, W, H, J, 0))
        self.ok(L.vsom_set_state(self.h, self.m.ctypes.data_as(fp), self.s.ctypes.data_as(fp), None, None,
                                 self.hits.ctypes.data_as(u64p)))
        self.hm, self.hs = np.empty_like(self.m), np.empty_like(self.s)
        self.last = np.ascontiguousarray(self.X[-1:])
        self.rows, self.fp, self.u64p, self.dp = rows, fp, u64p, dp

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.L.vsom_last_error().decode())

    def call(self):
        L, fp, u64p, dp = self.L, self.fp, self.u64p, self.dp
        unit = np.empty(self.rows, np.uint64)
        d = C.c_uint64()
        for i in range(self.rows):          # Som::variationalAutoEncoder, once per row
            self.ok(L.vsom_upload_chunk(self.h, self.last.ctypes.data_as(fp), 1))
            uu = C.c_double(self.u[i])
            self.ok(L.vsom_bmd_batch(self.h, MIN_HITS, 0, 1, C.byref(uu), C.byref(d), None, None))
            unit[i] = d.value
        self.ok(L.vsom_get_state(self.h, self.hm.ctypes.data_as(fp), self.hs.ctypes.data_as(fp), None, None, None))
        b = np.where(unit == np.uint64(2 ** 64 - 1), np.uint64(0), unit).astype(np.int64)
        with np.errstate(all="ignore"):
            rec = np.log(self.Lg / (1 - self.Lg)) / 1.6 * self.hs[b] + self.hm[b]
        return unit, rec

    def close(self):
        self.L.vsom_destroy(self.h)


class New:
    def __init__(self, name):
        import vsom_amd
        from vsom_amd import capi
        W, H, J, rows = SHAPES[name]
        self.m, self.s, self.hits, self.X, self.u, self.Lg = state(W, H, J, rows)
        self.rule = capi.GENERATE_AS_WRITTEN
        self.ctx = vsom_amd.Context(W, H, J, 0)
        self.ctx.set_state(map=self.m, sigma=self.s, hits=self.hits)
        self.ctx.upload_chunk(self.X)

    def call(self):
        r = self.ctx.generate(MIN_HITS, self.u, self.Lg, self.rule)
        return r["unit"], r["record"]

    def kernel_times(self, calls):
        ctx = self.ctx
        ctx.enable_timing(True, groups=["bmu", "finish"])
        ctx.get_timing(reset=True)
        draw, decode = [], []
        for _ in range(calls):
            self.call()
            t = ctx.get_timing(reset=True)
            draw.append(t["bmu"][0] * 1e-3)
            decode.append(t["finish"][0] * 1e-3)
        ctx.enable_timing(False)
        return draw, decode

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
    ap.add_argument("--parent-calls", type=int, default=5)
    ap.add_argument("--shapes", default="ref20,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_bench.jsonl"))
    a = ap.parse_args()
    routes = a.route.split(",")
    import torch  # noqa: F401  (first: one HIP runtime in the process)
    for name in a.shapes.split(","):
        W, H, J, rows = SHAPES[name]
        new = New(name) if "new" in routes else None
        par = Parent(name, a.lib) if "parent" in routes else None
        res = {"shape": f"{W}x{H}x{J}", "rows": rows, "rule": "as_written", "routes": routes, "calls": a.calls,
               "parent_calls": a.parent_calls if par else 0}
        vals = {}
        if new:
            for _ in range(3):
                new.call()
        if par:
            par.call()
        ts = {"call": [], "parent": []}
        for k in range(a.calls):                       # the routes alternate
            if new:
                t, vals["new"] = wall(new.call)
                ts["call"].append(t)
            if par and k < a.parent_calls:
                t, vals["parent"] = wall(par.call)
                ts["parent"].append(t)
        for k, v in ts.items():
            if v:
                put(res, k, v)
        if new:
            draw, decode = new.kernel_times(a.calls)
            put(res, "draw", draw)
            put(res, "decode", decode)
        if new and par:
            un, rn = vals["new"]
            up, rp = vals["parent"]
            res["units_equal"] = bool((un == up).all())
            ok = up != np.uint64(2 ** 64 - 1)
            res["rows_with_mass"] = int(ok.sum())
            with np.errstate(all="ignore"):
                res["max_abs_record_diff"] = float(np.nanmax(np.abs(rn[ok] - rp[ok]))) if ok.any() else None
            res["speedup"] = round(res["parent_us"] / res["call_us"], 2)
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
