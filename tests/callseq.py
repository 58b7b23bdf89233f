"""Seeded random walks over the single-context C ABI (include/vsom_hip.h), checked against the CPU oracle.

Imported by tests/test_gpu_call_sequences.py (the real library) and tests/test_call_sequences_model.py (fake contexts
backed by a second oracle, some of them wrong on purpose).  A walk is a list of ops -- plain tuples (name, params) that
print as Python literals -- whose first entry names the configuration and the seed; `replay(ops)` reruns a printed list.

The model is an oracle.pyoracle.OracleSom plus a record of what the header promises about the rest of the context: the
current chunk and its lastBMU, the pending (prefetched / device-staged) chunk, the last MSE and the online running
accumulator.  Every accepted call must return the model's values bit for bit (NaN == NaN); a call that reads the staged
rows while a chunk is pending may instead be refused (VSOM_ERR_INVALID naming the commit), which changes nothing.
"""
import ctypes as C

import numpy as np

import gen
from oracle import pyoracle as po

VSOM_ERR_INVALID = -1
EXPONENTIAL, INVERSE_PROPORTIONAL = 0, 1
BMU_AUTO, BMU_EXACT, BMU_SHORTLIST = 0, 1, 2
NTHREADS = 16
VSOM_CHAIN_MAX_WAVES = 448           # csrc/vsom_internal.hpp

# configuration: map, transformation, chunks (size, kind); kinds: "u8" uint8-valued, "f" the same / 255, "dense" blobs,
# "clr" correlated columns
CONFIGS = {
    "std48": dict(W=48, H=48, J=196, tr=po.STANDARD, custom=False,
                  chunks=[(1100, "u8"), (1280, "f"), (77, "u8"), (1500, "dense"), (4500, "u8"), (1024, "f")]),
    "med48": dict(W=48, H=48, J=196, tr=po.MEDIAN, custom=False,
                  chunks=[(1100, "u8"), (300, "dense"), (1536, "f"), (4500, "u8"), (1024, "u8")]),
    "std12": dict(W=12, H=12, J=24, tr=po.STANDARD, custom=False,
                  chunks=[(300, "dense"), (128, "dense"), (77, "dense"), (1500, "dense")]),
    "clr12": dict(W=12, H=12, J=6, tr=po.CLR, custom=False,
                  chunks=[(300, "clr"), (128, "clr"), (77, "clr"), (700, "clr")]),
    "custom12": dict(W=12, H=12, J=24, tr=po.STANDARD, custom=True,
                     chunks=[(200, "dense"), (64, "dense"), (301, "dense")]),
}

# ops that read the staged rows of the current chunk: the ones a pending chunk staged ahead may refuse
READS_ROWS = {"bmu", "bmu_local", "bmu_restricted", "distances", "distances_row", "p1", "p2", "epoch", "epoch_async",
              "online"}
OBSERVE = {"get_state", "get_last_bmu", "get_sqres", "get_mse"}
# what a custom context refuses (include/vsom_hip.h, vsom_create_custom)
CUSTOM_REFUSED = {"stage", "p1", "finish", "p2", "bmu_restricted", "distances_row"}


def chunk_data(cfg_name, seed, scale=1):
    cfg = CONFIGS[cfg_name]
    out = []
    for i, (b, kind) in enumerate(cfg["chunks"]):
        b = max(8, b // scale)
        s = 1000 * seed + 17 * i + 3
        if kind == "u8":
            x = gen.mnist_like(b, seed=s, dim=cfg["J"])
        elif kind == "f":
            x = (gen.mnist_like(b, seed=s, dim=cfg["J"]) / np.float32(255)).astype(np.float32)
        elif kind == "clr":
            x = gen.correlated(b, cfg["J"], seed=s)
        else:
            x = gen.blobs(b, cfg["J"], 5, s, s + 1, sigma=0.4)
        out.append(np.ascontiguousarray(x, np.float32))
    return out


def chain_max_nodes(cfg):
    """The largest phase-2 node range that takes the small-map chain kernel, which reads the staged rows themselves
    (csrc/vsom_update.hip, vsom_use_chain: ceil(n / 64) * ceil(D / 14) <= VSOM_CHAIN_MAX_WAVES); a larger range takes
    the lane = node kernels, which record the rows-are-free event a later prefetch may stage ahead behind.  None where
    nothing is staged ahead (CLR, custom contexts)."""
    if cfg["custom"] or cfg["tr"] == po.CLR:
        return None
    D = po.length(cfg["tr"], cfg["J"])
    return 64 * (VSOM_CHAIN_MAX_WAVES // ((D + 13) // 14))


def stages_ahead(cfg):
    """whether a whole-map phase 2 takes the lane = node kernels, so that a prefetch right behind it stages ahead"""
    c = chain_max_nodes(cfg)
    return c is not None and cfg["W"] * cfg["H"] > c


def initial_map(cfg_name, seed):
    cfg = CONFIGS[cfg_name]
    D = po.length(cfg["tr"], cfg["J"])
    m = gen.random_map(cfg["W"] * cfg["H"], D, seed=seed)
    if cfg["J"] >= 100:                  # in the range of the uint8-valued chunks
        m = (m * np.float32(100) + np.float32(100)).astype(np.float32)
    if cfg["tr"] == po.CLR:
        m = (m * np.float32(0.2)).astype(np.float32)
    return m


# ---- generator ---------------------------------------------------------------------------------------------------------
class _Gen:
    def __init__(self, cfg_name, seed, scale):
        self.cfg = CONFIGS[cfg_name]
        self.rs = np.random.RandomState(seed)
        self.sizes = [max(8, b // scale) for b, _ in self.cfg["chunks"]]
        self.N = self.cfg["W"] * self.cfg["H"]
        self.B = self.sizes[0]
        self.pending = None                # index of the pending chunk
        self.chain = False                 # an online chunk may continue the running MSE (first_chunk = 0)
        self.ops = []

    def r(self, n):
        return int(self.rs.randint(n))

    def sigma(self):
        return float(self.rs.choice([0.7, 1.0, 2.5, 6.0, 12.0]))

    def emit(self, name, **p):
        self.ops.append((name, p))
        if name == "upload":
            self.B = self.sizes[p["chunk"]]
        elif name in ("prefetch", "stage"):
            self.pending = p["chunk"]
        elif name == "commit" and self.pending is not None:
            self.B = self.sizes[self.pending]
            self.pending = None
        if name == "online":
            self.chain = self.pending is None       # (with a chunk pending the call may be refused)
        elif name in ("single", "epoch", "epoch_async", "p1", "finish", "p2"):
            self.chain = False

    def next_chunk(self):
        return self.r(len(self.sizes))

    def give(self, chunk=None):
        """a prefetch from pinned or pageable memory, or a chunk handed over in HBM"""
        src = ["pinned", "pageable", "device"][self.r(3)]
        chunk = self.next_chunk() if chunk is None else chunk
        if src == "device":
            self.emit("stage", chunk=chunk)
        else:
            self.emit("prefetch", chunk=chunk, src=src)

    def online(self, mode=None):
        mode = mode or ["null", "mse", "fetch"][self.r(3)]
        first = True if not self.chain else bool(self.r(2))
        self.emit("online", eta=float(self.rs.choice([0.05, 0.2])), sigma=self.sigma(),
                  decay=self.r(2), first=first, mode=mode)

    def split(self, interleave=False, end_with_commit=False):
        """phase 1 over a random partition of the rows, finish, phase 2 over a random partition of the nodes"""
        if interleave and stages_ahead(self.cfg):
            self.emit("upload", chunk=0, asynchronous=False)     # (not the short chunk staged ahead below)
        first = bool(self.r(2))
        cuts = sorted(set([0, self.B] + [self.r(self.B + 1) for _ in range(self.r(3))]))
        ranges = list(zip(cuts[:-1], cuts[1:]))
        self.rs.shuffle(ranges)
        for s0, s1 in ranges:
            self.emit("p1", s0=int(s0), s1=int(s1), first=first)
        self.emit("finish")
        sg = self.sigma()
        if interleave and stages_ahead(self.cfg):
            # a range large enough for the lane = node kernels, a short next chunk staged ahead behind it, then ranges
            # small enough for the chain kernel, which must not read the rows that staging overwrote
            c = chain_max_nodes(self.cfg)
            big = c + 1 + self.r(min(64, self.N - c - 1))
            sg = 12.0                       # (a wide neighbourhood: every node of the chain ranges feels every sample)
            cuts = sorted(set([big, self.N] + [big + self.r(self.N - big) for _ in range(self.r(3))]))
            rest = list(zip(cuts[:-1], cuts[1:]))
            self.rs.shuffle(rest)
            self.emit("p2", sigma=sg, n0=0, n1=int(big))
            self.give(chunk=int(np.argmin(self.sizes)))
            for n0, n1 in rest:
                self.emit("p2", sigma=sg, n0=int(n0), n1=int(n1))
        else:
            cuts = sorted(set([0, self.N, 1 + self.r(self.N - 1)] + [self.r(self.N + 1) for _ in range(self.r(3))]))
            ranges = list(zip(cuts[:-1], cuts[1:]))
            self.rs.shuffle(ranges)
            for k, (n0, n1) in enumerate(ranges):
                self.emit("p2", sigma=sg, n0=int(n0), n1=int(n1))
                if interleave and k == 0:
                    self.give()
        if end_with_commit:
            self.emit("commit")

    def random_op(self):
        cfg = self.cfg
        choices = ["upload", "give", "commit", "epoch_async", "epoch", "split", "online", "single", "bmu", "bmu_local",
                   "bmu_restricted", "distances", "distances_row", "set_last_bmu", "get_last_bmu", "get_sqres",
                   "get_mse", "bmu_mode", "set_state", "get_state"]
        w = np.array([3, 4, 4, 4, 3, 2, 5, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1], np.float64)
        if cfg["custom"]:
            w[choices.index("bmu_mode")] = 0
        what = choices[int(self.rs.choice(len(choices), p=w / w.sum()))]
        if what == "upload":
            self.emit("upload", chunk=self.next_chunk(), asynchronous=bool(self.r(2)))
        elif what == "give":
            self.give()
        elif what == "commit":
            self.emit("commit")
        elif what in ("epoch_async", "epoch"):
            self.emit(what, sigma=self.sigma(), first=bool(self.r(2)))
        elif what == "split":
            if self.pending is None:       # (a refusal inside phase 1 would leave a half-searched chunk to the finish)
                self.split()
        elif what == "online":
            self.online()
        elif what == "single":
            self.emit("single", seed=self.r(1 << 30), eta=0.1, sigma=self.sigma(), decay=self.r(2),
                      last=self.r(self.N))
        elif what == "bmu_restricted":
            if self.B <= 1100:
                self.emit(what, min_hits=int(self.rs.choice([0, 1, 3])))
        elif what == "distances":
            self.emit(what, seed=self.r(1 << 30), count=1 + self.r(300))
        elif what == "distances_row":
            self.emit(what, row=self.r(self.B))
        elif what == "set_last_bmu":
            self.emit(what, seed=self.r(1 << 30))
        elif what == "bmu_mode":
            self.emit(what, mode=self.r(3))
        elif what == "set_state":
            self.emit(what, seed=self.r(1 << 30), parts=["map", "msw", "all"][self.r(3)])
        else:
            self.emit(what)


def generate(cfg_name, seed, n_ops=40, scale=1):
    """A walk of about n_ops ops.  By construction it holds each of these runs with no synchronising call inside:
    async epoch -> online chunk (mse NULL) -> prefetch / stage_next_device -> commit;
    phase-2 range -> prefetch -> phase-2 range(s) -> commit (where a prefetch stages ahead: a lane = node range, a short
    chunk staged behind it, chain-kernel ranges);
    async epoch -> prefetch -> prefetch (an abandoned stage-ahead) -> search -> commit."""
    g = _Gen(cfg_name, seed, scale)
    g.ops.append(("config", {"name": cfg_name, "seed": seed, "scale": scale}))
    g.emit("set_state", seed=seed, parts="init")
    g.emit("upload", chunk=0, asynchronous=False)
    slots = sorted(g.rs.choice(np.arange(2, n_ops - 8), 3, replace=False))
    runs = list(g.rs.permutation(3))
    k = 2
    while k < n_ops:
        if slots and k >= slots[0]:
            slots.pop(0)
            run = runs.pop(0)
            if g.pending is not None:
                g.emit("commit")
            if run == 0:
                # a long online chunk (the per-sample scan over the first chunk's rows) and a short next chunk that fits
                # the staged-row buffers: staged ahead, its staging would land inside the online chunk
                g.emit("upload", chunk=0, asynchronous=False)
                if not g.cfg["custom"]:
                    g.emit("bmu_mode", mode=BMU_EXACT)
                g.emit("epoch_async", sigma=g.sigma(), first=bool(g.r(2)))
                g.online(mode="null")
                g.give(chunk=int(np.argmin(g.sizes)))
                g.emit("commit")
            elif run == 1:
                g.split(interleave=True, end_with_commit=True)
            else:
                g.emit("epoch_async", sigma=g.sigma(), first=bool(g.r(2)))
                g.give()
                g.give()
                search = ["bmu", "bmu_local", "distances_row"][g.r(3)]
                if search == "distances_row":
                    g.emit(search, row=g.r(g.B))
                else:
                    g.emit(search)
                g.emit("commit")
            g.emit("get_state")     # (after the run: before a later epoch rewrites what the run left)
            k += 4
            continue
        g.random_op()
        k += 1
    g.emit("get_state")
    return g.ops


# ---- the model ---------------------------------------------------------------------------------------------------------
class Refused(Exception):
    pass


def _rand_state(cfg_name, seed, parts, N, D):
    rs = np.random.RandomState(seed)
    st = {"map": initial_map(cfg_name, seed)}
    if parts in ("msw", "all"):
        st["sigma"] = (rs.rand(N, D) * 0.5).astype(np.float32)
        st["S"] = (rs.rand(N, D) * 2).astype(np.float32)
        st["weight"] = (rs.rand(N) * 10).astype(np.float32)
        if parts == "msw":
            st["sigma"][...] = 0
            st["S"][...] = 0
    if parts == "all":
        st["hits"] = rs.randint(0, 5, size=N).astype(np.uint64)
    return st


def materialize(op, model):
    """the concrete arguments of an op in the model's current state (the same for every backend)"""
    name, p = op
    cfg = CONFIGS[model.cfg_name]
    N, B = model.N, model.B
    if name in ("upload", "prefetch", "stage"):
        return {"X": model.chunks[p["chunk"]]}
    if name == "single":
        rs = np.random.RandomState(p["seed"])
        X = model.chunks[rs.randint(len(model.chunks))]
        return {"v": np.ascontiguousarray(X[rs.randint(X.shape[0])])}
    if name == "distances":
        rs = np.random.RandomState(p["seed"])
        return {"nodes": rs.randint(0, N, size=p["count"]).astype(np.uint64),
                "rows": rs.randint(0, max(B, 1), size=p["count"]).astype(np.uint64)}
    if name == "set_last_bmu":
        return {"idx": np.random.RandomState(p["seed"]).randint(0, N, size=B).astype(np.uint64)}
    if name == "set_state":
        return _rand_state(model.cfg_name, p["seed"], p["parts"], N, po.length(cfg["tr"], cfg["J"]))
    return {}


class Model:
    """what the header says the context holds after each call"""

    def __init__(self, cfg_name, seed, scale=1):
        cfg = CONFIGS[cfg_name]
        self.cfg_name, self.cfg = cfg_name, cfg
        self.som = po.OracleSom(cfg["W"], cfg["H"], cfg["J"], cfg["tr"])
        self.N = cfg["W"] * cfg["H"]
        self.chunks = chunk_data(cfg_name, seed, scale)
        self.X = None
        self.lb = np.zeros(0, np.uint64)
        self.sq = np.zeros(0, np.float32)      # the oracle's per-sample residuals of the last phase 1 (the finish sums them)
        self.sqres = None                      # what vsom_get_sqres returns, when a search has defined it
        self.pending = None
        self.mse = None                        # last MSE (None: nothing has written one yet)
        self.run = None                        # online running accumulator after the last online chunk

    @property
    def B(self):
        return 0 if self.X is None else self.X.shape[0]

    def close(self):
        self.som.close()

    def _load(self, X):
        self.X = X
        self.lb = np.zeros(X.shape[0], np.uint64)
        self.sq = np.zeros(X.shape[0], np.float32)
        self.sqres = None

    def _dist(self, nodes, rows):
        return np.array([self.som.dist(int(n), self.X[int(r)]) for n, r in zip(nodes, rows)], np.float32)

    def refusal_allowed(self, name):
        return name in READS_ROWS and self.pending is not None

    def apply(self, op, a):
        """the op's effect; returns the outputs the call must give"""
        name, p = op
        s = self.som
        if name == "upload":
            self._load(a["X"])
        elif name in ("prefetch", "stage"):
            self.pending = a["X"]
        elif name == "commit":
            if self.pending is None:
                raise Refused("nothing pending")
            self._load(self.pending)
            self.pending = None
        elif name in ("epoch", "epoch_async"):
            self.mse = s.batch_epoch(self.X, self.lb, p["sigma"], p["first"], nthreads=NTHREADS)
            self.sqres = None
            return {"mse": self.mse} if name == "epoch" else {}
        elif name == "p1":
            s.batch_phase1_range(self.X, p["s0"], p["s1"], self.lb, self.sq, p["first"], nthreads=NTHREADS)
            self.sqres = None
        elif name == "finish":
            self.mse = s.batch_phase1_finish(self.lb, self.sq)
        elif name == "p2":
            s.batch_phase2_range(self.X, self.lb, p["sigma"], p["n0"], p["n1"], nthreads=NTHREADS)
        elif name == "online":
            start = 0.0 if p["first"] else self.run
            self.run = s.train_online_chunk(self.X, self.lb, p["eta"], p["sigma"], p["decay"], mse_start=start)
            self.mse = self.run
            self.sqres = None
            if p["mode"] == "mse":
                return {"mse": self.run}
            if p["mode"] == "fetch":
                return {"mse": self.run, "lb": self.lb.copy()}
        elif name == "single":
            bmu, res, dist, lb = s.train_single(a["v"], p["eta"], p["sigma"], p["last"], p["decay"])
            return {"bmu": bmu, "res": res, "dist": dist, "last": lb}
        elif name in ("bmu", "bmu_local"):
            s.batch_phase1_range(self.X, 0, self.B, self.lb, self.sq, name == "bmu", nthreads=NTHREADS)
            self.sqres = self._dist(self.lb, np.arange(self.B))
            return {"idx": self.lb.copy(), "dist": self.sqres.copy()}
        elif name == "bmu_restricted":
            self.lb[:] = [s.find_restricted_bmu(x, p["min_hits"]) for x in self.X]
            self.sqres = self._dist(self.lb, np.arange(self.B))
            return {"idx": self.lb.copy(), "dist": self.sqres.copy()}
        elif name == "distances":
            return {"d": self._dist(a["nodes"], a["rows"])}
        elif name == "distances_row":
            return {"d": self._dist(np.arange(self.N), np.full(self.N, p["row"]))}
        elif name == "set_last_bmu":
            self.lb[:] = a["idx"]
        elif name == "get_last_bmu":
            return {"lb": self.lb.copy()}
        elif name == "get_sqres":
            return {"sq": None if self.sqres is None else self.sqres.copy()}
        elif name == "get_mse":
            return {"mse": self.mse}
        elif name == "set_state":
            s.set_state(**a)
        elif name == "get_state":
            return self.state()
        return {}

    def state(self):
        s = self.som
        return {"map": s.map.copy(), "sigma": s.sigma.copy(), "S": s.S.copy(), "weight": s.weight.copy(),
                "hits": s.hits.copy()}


# ---- comparison --------------------------------------------------------------------------------------------------------
def first_difference(got, exp):
    """None when got equals exp bit for bit (floats: NaN == NaN), else a description of the first differing element"""
    if exp is None:
        return None                        # (nothing defined to compare with)
    g, e = np.asarray(got), np.asarray(exp)
    if g.shape != e.shape:
        return f"shape {g.shape} != {e.shape}"
    if e.dtype.kind == "f":
        g32, e32 = g.astype(np.float32), e.astype(np.float32)
        same = (g32.view(np.uint32) == e32.view(np.uint32)) | (np.isnan(g32) & np.isnan(e32))
    else:
        same = g == e
    if same.all():
        return None
    at = np.unravel_index(int(np.argmin(same.reshape(-1))), same.shape) if same.ndim else ()
    return f"element {tuple(int(i) for i in at)}: got {g[at]!r}, expected {e[at]!r} ({int((~same).sum())} differ)"


class WalkFailure(AssertionError):
    pass


def run_walk(ops, make_backend):
    """Run `ops` on the backend make_backend(cfg_name, model) returns and on the model; raises WalkFailure with the seed,
    the ops up to the failing one and the first differing element.  Returns counts of what happened."""
    name0, cfg = ops[0]
    assert name0 == "config", ops[0]
    model = Model(cfg["name"], cfg["seed"], cfg.get("scale", 1))
    be = make_backend(cfg["name"], model)
    stats = {"ops": 0, "refused": 0}
    done = [ops[0]]

    def fail(msg):
        raise WalkFailure(f"call-sequence walk {cfg['name']} seed {cfg['seed']}: {msg}\n"
                          f"replay(ops) with ops = {done!r}")

    def check_outputs(what, got, exp):
        for k, e in exp.items():
            d = first_difference(got.get(k), e)
            if d:
                fail(f"{what}: output {k!r} differs from the oracle at {d}")

    def check_all(what):
        got = be.observe()
        exp = model.state()
        exp.update(lb=model.lb, mse=model.mse)
        check_outputs(f"{what} (full state)", got, exp)

    try:
        for op in ops[1:]:
            done.append(op)
            name, p = op
            a = materialize(op, model)
            rc, msg, out = be.call(op, a)
            stats["ops"] += 1
            if model.cfg["custom"] and name in CUSTOM_REFUSED:
                if rc != VSOM_ERR_INVALID:
                    fail(f"{name} on a custom context returned {rc}, not VSOM_ERR_INVALID")
                continue
            if name == "commit" and model.pending is None:
                if rc != VSOM_ERR_INVALID:
                    fail(f"commit with nothing pending returned {rc}")
                continue
            if rc != 0:
                if rc == VSOM_ERR_INVALID and "commit" in msg and model.refusal_allowed(name):
                    stats["refused"] += 1
                    continue
                fail(f"{name} failed: {rc} {msg}")
            exp = model.apply(op, a)
            check_outputs(name, out, exp)
            if name in OBSERVE:
                check_all(name)
        check_all("end of walk")
    finally:
        be.close()
        model.close()
    return stats


# ---- the real library --------------------------------------------------------------------------------------------------
class GpuBackend:
    """the C ABI of libvsom_hip.so, called directly (the Python wrapper synchronises where the walk must not)"""

    def __init__(self, cfg_name, model):
        import vsom_amd
        from vsom_amd import capi
        import custom_hooks
        self.capi = capi
        self.L = capi.lib()
        cfg = CONFIGS[cfg_name]
        if cfg["custom"]:
            depth, rlen = custom_hooks.shape("standard", cfg["J"])
            self.ctx = capi.Context(cfg["W"], cfg["H"], cfg["J"], capi.CUSTOM, source=custom_hooks.STANDARD,
                                    depth=depth, residual_len=rlen)
        else:
            self.ctx = vsom_amd.Context(cfg["W"], cfg["H"], cfg["J"], cfg["tr"])
        self.h = self.ctx._h
        self.N, self.D = self.ctx.n_nodes, self.ctx.depth
        # pinned and device copies of every chunk, made up front: an allocation inside the walk (hipHostMalloc,
        # hipMalloc + hipMemcpy) would synchronise the device and hide the asynchrony the walk is about
        self.hip = C.CDLL("libamdhip64.so")
        self.pinned, self.dev = [], []
        for X in model.chunks:
            pb = capi.PinnedBuffer(X.shape)
            pb.array[...] = X
            self.pinned.append(pb)
            ptr = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(ptr), C.c_size_t(max(X.nbytes, 4))) == 0
            assert self.hip.hipMemcpy(ptr, X.ctypes.data_as(C.c_void_p), C.c_size_t(X.nbytes), C.c_int(1)) == 0
            self.dev.append(ptr)

    def close(self):
        self.ctx.close()
        for pb in self.pinned:
            pb.free()
        for p in self.dev:
            self.hip.hipFree(p)

    def B(self):
        return int(self.L.vsom_chunk_size(self.h))

    def call(self, op, a):
        L, h, capi = self.L, self.h, self.capi
        f, u = capi._f, capi._u
        name, p = op
        out = {}
        if name == "upload":
            X = a["X"]
            if p["asynchronous"]:
                X = self.pinned[p["chunk"]].array
                rc = L.vsom_upload_chunk_async(h, f(X), X.shape[0])
            else:
                rc = L.vsom_upload_chunk(h, f(X), X.shape[0])
        elif name == "prefetch":
            X = a["X"] if p["src"] == "pageable" else self.pinned[p["chunk"]].array
            rc = L.vsom_prefetch_chunk(h, f(X), X.shape[0])
        elif name == "stage":
            rc = L.vsom_stage_next_device(h, C.c_void_p(self.dev[p["chunk"]].value), a["X"].shape[0])
        elif name == "commit":
            rc = L.vsom_commit_chunk(h)
        elif name == "epoch_async":
            rc = L.vsom_batch_epoch_async(h, p["sigma"], int(p["first"]))
        elif name == "epoch":
            m = C.c_float()
            rc = L.vsom_batch_epoch(h, p["sigma"], int(p["first"]), C.byref(m))
            out["mse"] = np.float32(m.value)
        elif name == "p1":
            rc = L.vsom_batch_phase1_async(h, p["s0"], p["s1"], int(p["first"]))
        elif name == "finish":
            rc = L.vsom_batch_finish_async(h)
        elif name == "p2":
            rc = L.vsom_batch_phase2_async(h, p["sigma"], p["n0"], p["n1"])
        elif name == "online":
            m = C.c_float()
            if p["mode"] == "fetch":
                lb = np.zeros(self.B(), np.uint64)
                rc = L.vsom_train_online_chunk_fetch(h, p["eta"], p["sigma"], p["decay"], int(p["first"]), u(lb),
                                                     C.byref(m))
                out["lb"] = lb
            else:
                rc = L.vsom_train_online_chunk_acc(h, p["eta"], p["sigma"], p["decay"], int(p["first"]),
                                                   C.byref(m) if p["mode"] == "mse" else None)
            out["mse"] = np.float32(m.value)
        elif name == "single":
            res = np.empty(int(L.vsom_residual_len(h)), np.float32)
            lb, bmu, dist = C.c_uint64(p["last"]), C.c_uint64(), C.c_float()
            rc = L.vsom_train_single(h, f(a["v"]), p["eta"], p["sigma"], C.byref(lb), p["decay"], f(res),
                                     C.byref(dist), C.byref(bmu))
            out.update(bmu=int(bmu.value), res=res, dist=np.float32(dist.value), last=int(lb.value))
        elif name in ("bmu", "bmu_local", "bmu_restricted"):
            B = self.B()
            idx, dist = np.empty(B, np.uint64), np.empty(B, np.float32)
            if name == "bmu":
                rc = L.vsom_bmu_batch(h, u(idx), f(dist))
            elif name == "bmu_local":
                rc = L.vsom_bmu_local_batch(h, u(idx), f(dist))
            else:
                rc = L.vsom_bmu_restricted_batch(h, p["min_hits"], u(idx), f(dist))
            out.update(idx=idx, dist=dist)
        elif name == "distances":
            d = np.empty(a["nodes"].size, np.float32)
            rc = L.vsom_distances(h, u(a["nodes"]), u(a["rows"]), a["nodes"].size, f(d))
            out["d"] = d
        elif name == "distances_row":
            d = np.empty(self.N, np.float32)
            rc = L.vsom_distances_row(h, p["row"], f(d))
            out["d"] = d
        elif name == "set_last_bmu":
            rc = L.vsom_set_last_bmu(h, u(a["idx"]))
        elif name == "get_last_bmu":
            lb = np.empty(self.B(), np.uint64)
            rc = L.vsom_get_last_bmu(h, u(lb))
            out["lb"] = lb
        elif name == "get_sqres":
            sq = np.empty(self.B(), np.float32)
            rc = L.vsom_get_sqres(h, f(sq))
            out["sq"] = sq
        elif name == "get_mse":
            m = C.c_float()
            rc = L.vsom_get_mse(h, C.byref(m))
            out["mse"] = np.float32(m.value)
        elif name == "bmu_mode":
            rc = L.vsom_set_bmu_mode(h, p["mode"])
        elif name == "set_state":
            g = lambda k: a.get(k)
            rc = L.vsom_set_state(h, f(g("map")), f(g("sigma")), f(g("S")), f(g("weight")), u(g("hits")))
        elif name == "get_state":
            out = self._state()
            rc = 0 if out is not None else -1
        else:
            raise ValueError(name)
        msg = "" if rc == 0 else L.vsom_last_error().decode(errors="replace")
        return rc, msg, out

    def _state(self):
        N, D = self.N, self.D
        st = {"map": np.empty((N, D), np.float32), "sigma": np.empty((N, D), np.float32),
              "S": np.empty((N, D), np.float32), "weight": np.empty(N, np.float32), "hits": np.empty(N, np.uint64)}
        f, u = self.capi._f, self.capi._u
        self.capi.check(self.L.vsom_get_state(self.h, f(st["map"]), f(st["sigma"]), f(st["S"]), f(st["weight"]),
                                              u(st["hits"])))
        return st

    def observe(self):
        st = self._state()
        lb = np.empty(self.B(), np.uint64)
        self.capi.check(self.L.vsom_get_last_bmu(self.h, self.capi._u(lb)))
        m = C.c_float()
        self.capi.check(self.L.vsom_get_mse(self.h, C.byref(m)))
        st.update(lb=lb, mse=np.float32(m.value))
        return st


def replay(ops):
    """rerun a printed op list against the real library"""
    return run_walk(ops, GpuBackend)
