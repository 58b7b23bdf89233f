"""CPU self-test of the call-sequence walk (tests/callseq.py): the same walks as tests/test_gpu_call_sequences.py, run
against fake contexts backed by a second oracle.  The faithful fake must pass; each mutant -- a fake with one of the
ingest bugs the walk exists to find -- must be caught by at least one seed.  This shows, without a GPU, that the walk
can see that class of bug.

The sigma profile's walks run against the same fake, which then also models the pending sigmaMap: a deferred epoch computes
the whole epoch and withholds the new sigmaMap / S rows, keeping what the library's record keeps (the epoch's rows, its
lastBMU, its sigma); a materialisation computes them from that record, a drop discards it.  Mutants e-k break that
bookkeeping the ways an entry point wrongly listed as keeping the record -- or a record made from the wrong operands --
would.  The ingest walks themselves are pinned by digest: the generator's new ops must never enter their draws."""
import ast
import copy
import functools
import hashlib

import numpy as np
import pytest

import callseq as cs
from oracle import pyoracle as po

SEEDS = (1, 2, 3)
SCALE = 8            # chunks of 1/8 the GPU walk's rows: the oracle runs twice per op here (model and fake)


class FakeBackend:
    """A context as the header describes it, on a second oracle.  Like the library it stages a prefetched chunk ahead
    (over the current chunk's rows) when the prefetch directly follows an asynchronous epoch or a lane = node phase-2
    range (callseq.stages_ahead / chain_max_nodes), and then refuses what reads the rows until the commit.  `mutant`
    breaks it:
      a  an online chunk enqueued without a wait, then a prefetch: the samples from B/2 on train on the pending rows
      b  a chain-kernel phase-2 range after a chunk was staged ahead is not refused and reads the pending rows
      c  the commit does not zero lastBMU
      d  a refused call has already changed the model
    and, in the sigma profile (the pending sigmaMap):
      e  a partial phase-2 range does not materialise first
      f  the materialisation takes the context's current lastBMU, not the epoch's
      g  the materialisation takes the current chunk, not the epoch's
      h  a weight-only vsom_set_state is treated as keeping the record (the materialisation then divides by the new weight)
      i  AUTO defers after one unread epoch
      j  an empty-chunk epoch forgets the drop
      k  vsom_set_last_bmu / vsom_get_mse count as a read"""

    def __init__(self, cfg_name, model, mutant=None):
        self.m = cs.Model(model.cfg_name, 0)
        self.m.chunks = model.chunks
        self.cfg = cs.CONFIGS[cfg_name]
        self.mutant = mutant
        self.stage_ok = cs.stages_ahead(self.cfg)
        self.chain_max = cs.chain_max_nodes(self.cfg)
        self.rows_free = False
        self.ahead_rows = False
        self.deferred = None
        # the pending sigmaMap (sigma profile only: the ingest walks run the fake they always ran)
        self.sigma_profile = model.profile == "sigma"
        self.can_defer = cs.stages_ahead(self.cfg) and po.length(self.cfg["tr"], self.cfg["J"]) % 4 == 0
        self.mode = cs.SIGMA_AUTO
        self.unread = 0
        self.rec = None                     # (rows, lastBMU, sigma) of the deferred epoch
        self.counts = [0, 0, 0]             # deferred, dropped, materialised

    def close(self):
        self.m.close()

    # ---- pending sigmaMap ----
    def _materialise(self):
        X, lb, sigma = self.rec
        self.rec = None
        self.counts[2] += 1
        m, cfg = self.m, self.cfg
        if self.mutant == "f":
            lb = np.resize(m.lb, lb.shape)
        if self.mutant == "g":
            X = m.X
            lb = np.resize(lb, X.shape[0])
        t = po.OracleSom(cfg["W"], cfg["H"], cfg["J"], cfg["tr"])
        t.batch_phase2_range(X, np.ascontiguousarray(lb, np.uint64), sigma, 0, m.N, nthreads=cs.NTHREADS)
        sig = t.sigma.copy()
        if self.mutant == "h":              # raw S over the weight in place now, not the epoch's -- bit-exact where the
            changed = t.weight.view(np.uint32) != m.som.weight.view(np.uint32)        # two are the same weight
            with np.errstate(all="ignore"):
                wrong = np.sqrt(np.abs(sig * sig * t.weight[:, None] / m.som.weight[:, None])).astype(np.float32)
            sig = np.where(changed[:, None], wrong, sig)
        t.close()
        m.som.set_state(sigma=sig)

    def _read(self):
        self.unread = 0
        if self.rec is not None:
            self._materialise()

    def _keeps(self, op):
        name, p = op
        if self.mutant == "k" and name in ("set_last_bmu", "get_mse"):
            return False
        if self.mutant == "h" and name == "set_state" and p["parts"] == "weight_only":
            return True
        return name in cs.SIGMA_KEEP

    def _whole(self, op):
        name, p = op
        return name in ("epoch", "epoch_async") or (name == "p2" and p["n0"] == 0 and p["n1"] == self.m.N)

    def _apply(self, op, a):
        """m.apply(op, a) with the pending-sigmaMap bookkeeping of an accepted call around it"""
        m = self.m
        if not self.sigma_profile:
            return m.apply(op, a)
        name, p = op
        if name == "sigma_mode":
            self.mode = cs.SIGMA_MODES[p["mode"]]
        if not self._whole(op):
            if name == "p2" and self.rec is not None and self.mutant != "e":
                self._materialise()
            return m.apply(op, a)
        if self.rec is not None and not (self.mutant == "j" and m.B == 0):
            self.rec = None
            self.counts[1] += 1
        need = 1 if self.mutant == "i" else 2
        defer = self.can_defer and m.B > 0 and (self.mode == cs.SIGMA_LAZY or
                                                (self.mode == cs.SIGMA_AUTO and self.unread >= need))
        old = (m.som.sigma.copy(), m.som.S.copy())
        out = m.apply(op, a)
        if defer:
            self.rec = (m.X, m.lb.copy(), p["sigma"])
            self.counts[0] += 1
            m.som.set_state(sigma=old[0], S=old[1])
        self.unread += 1
        return out

    def call(self, op, a):
        if self.sigma_profile and not self._keeps(op):
            late = self._flush(op[0])           # (an online chunk enqueued before this call comes first)
            assert late is None
            self._read()                        # the entry check: before anything can refuse the call
        rc, msg, out = self._call(op, a)
        if self.sigma_profile:
            out["sigma_stats"] = tuple(self.counts) + (int(self.rec is not None),)
        return rc, msg, out

    def _mixed(self):
        """the current rows with those from B/2 on (or the first ones: mutant b) taken from the pending chunk"""
        X = self.m.X.copy()
        P = self.m.pending
        if self.mutant == "a":
            for i in range(X.shape[0] // 2, X.shape[0]):
                X[i] = P[i % P.shape[0]]
        else:
            k = min(X.shape[0], P.shape[0])
            X[:k] = P[:k]
        return X

    def _flush(self, next_name=None):
        if self.deferred is None:
            return
        op, a = self.deferred
        self.deferred = None
        if self.mutant == "a" and next_name in ("prefetch", "stage"):
            return ("mixed", op, a)
        self.m.apply(op, a)
        return None

    def _refuse(self, name):
        if self.mutant == "d":              # a partial step of the refused call
            s = self.m.som
            s.train_single(self.m.X[0], 0.1, 1.0, 0, 0)
        return cs.VSOM_ERR_INVALID, f"{name}: the next chunk is staged ahead: vsom_commit_chunk first", {}

    def _call(self, op, a):
        name, p = op
        late = self._flush(name)
        m = self.m
        if self.cfg["custom"] and name in cs.CUSTOM_REFUSED:
            return cs.VSOM_ERR_INVALID, "not for a custom context", {}
        if self.cfg["tr"] == po.CLR and name in cs.CLR_REFUSED:
            return cs.VSOM_ERR_INVALID, "CLR contexts are not supported", {}
        if name == "commit" and m.pending is None:
            return cs.VSOM_ERR_INVALID, "no prefetched chunk to commit", {}
        keep_free = False
        if name in ("prefetch", "stage"):
            if self.rows_free and self.stage_ok:
                self.ahead_rows = True
            keep_free = True
        elif name == "commit" or name == "upload":
            self.ahead_rows = False
        lane_node = name == "p2" and self.stage_ok and p["n1"] - p["n0"] > self.chain_max
        reads = name in cs.READS_ROWS and not lane_node
        mixed_p2 = False
        if self.ahead_rows and reads:
            if self.mutant == "b" and name == "p2":
                mixed_p2 = True
            else:
                return self._refuse(name)
        if late is not None:                # mutant a: the online chunk ran beside the prefetch's staging
            _, oop, oa = late
            X = m.X
            m.pending = a["X"]
            m.X = self._mixed()
            m.apply(oop, oa)
            m.X = X
            m.pending = None
        if name == "online" and p["mode"] == "null":
            self.deferred = (op, a)
            self.rows_free = False
            return 0, "", {}
        old_lb = m.lb.copy()
        if mixed_p2:
            X = m.X
            m.X = self._mixed()
            out = m.apply(op, a)
            m.X = X
        else:
            out = self._apply(op, a)
        if name == "commit" and self.mutant == "c":
            m.lb[:] = np.resize(old_lb, m.lb.shape) if old_lb.size else 0
        if name == "epoch_async" and self.stage_ok:
            self.rows_free = True
        elif lane_node:
            self.rows_free = True
        elif not keep_free:
            self.rows_free = False
        return 0, "", {k: v for k, v in out.items() if v is not None}

    def observe(self):
        self._flush()
        if self.sigma_profile:
            self._read()                        # (vsom_get_state)
        st = self.m.state()
        st.update(lb=self.m.lb.copy(), mse=self.m.mse)
        return st


def _walks():
    return [(c, s) for c in cs.CONFIGS for s in SEEDS]


MODES = ("lazy", "auto")
DEFERRING = ("std48", "med48", "std80")
GPU_SEEDS = (1, 2)   # tests/test_gpu_call_sequences.py, test_sigma_walk_matches_oracle


def _sigma_walks():
    return [(c, m, s) for c in cs.CONFIGS for m in MODES for s in SEEDS]


def _run_sigma(cfg, mode, seed, mutant=None, scale=SCALE):
    ops = cs.generate(cfg, seed, scale=scale, profile="sigma", mode=mode)
    return cs.run_walk(ops, lambda name, model: FakeBackend(name, model, mutant))


@functools.lru_cache(maxsize=None)
def _faithful_sigma(cfg, mode, seed):
    return _run_sigma(cfg, mode, seed)


# sha256(repr(generate(cfg, seed, scale=scale))) of the ingest walks, recorded before the sigma profile existed
INGEST_DIGESTS = {
    ("std48", 1, 1): "6ca8ce5c7f14532593df46da71209d47eae46e873028c54b79ee9d7d82dbf06b",
    ("std48", 2, 1): "bcdb2f4c9566d5a18ac9424b65e312dfb730adf9e32773a2ee1d48d8a4f2ad08",
    ("std48", 3, 1): "4ba52b8ac3159c08ed53aba5683e02d797e6491ef6efdfa32dbe0641f8cb20e4",
    ("med48", 1, 1): "dba54c78b4d16b2f7c07e580eb9385f0ec0181bfa1f4cc72ea73ea6e85aa80ce",
    ("med48", 2, 1): "2296c41d7252961d74f1e173179f2801fe7b07f82e557de009ad95c2b7a0a9c7",
    ("med48", 3, 1): "15938ee5d6985559f92bf8efaecab73226ee14c0d1302592b9dfb01082b71b5c",
    ("std12", 1, 1): "77871d5371b9d88157abce6e2d14b483425c46f3fe1e74fd1cdacec3b16475b1",
    ("std12", 2, 1): "12597d16c777d7fead90ecf5ae2dad2cba108e1f4c258af0f1186e096eb4e083",
    ("std12", 3, 1): "db8af9b281ad0d904988e645659bf99509916e022a43fe82ae95e3133ae4247c",
    ("clr12", 1, 1): "7b76adc0f0b87904020c8ce373aef14e9204de439f877043a98d3c24608ec060",
    ("clr12", 2, 1): "f231a37f5f4bc98b63017140b23b60ec293f3286e76894b19d726ad389d4abba",
    ("clr12", 3, 1): "6578068c51f4928f9b4169d88cd0d5072e4c1a998c164de4b0ff7023c835de1f",
    ("custom12", 1, 1): "477f59cabaccf75f196118996e119deb8e856a7872ce1eb02ae2c8f00d4caa46",
    ("custom12", 2, 1): "c57dc5e70cc025f13767367af2ca1ed7ca8a57a17fd05a21e90020cc5f3c9bae",
    ("custom12", 3, 1): "88f12e47c365a94dc059e2450b27261bd7ce1d12444feb97045353f1a7295ed4",
    ("std48", 1, 8): "3fd1467f235102a5bc7c44c5ff205f16b94d7cc304addc2c55e8e22918fe85fe",
    ("std48", 2, 8): "a1ea8c3af573632e0cde662f628334c5500ea933841d9026108d5af91b46d00c",
    ("std48", 3, 8): "ba8e291a6d9d269d3ebe6c977819a977563a8f9cd4f2a340fe235521b4dde663",
    ("med48", 1, 8): "52adc53a96608690b6bd297d3a65fc593f1a47cd02a5ecf948d7c56147b543c0",
    ("med48", 2, 8): "acb65666a35776bac6c0c73e53130b8e5c1884778bc53d8c682c0d6f0cdd4048",
    ("med48", 3, 8): "3f9d14ba925e2cf834fa184068b1e8eadefff3e7893c6cbb5e97972061912c3d",
    ("std12", 1, 8): "412cf0ed959bfc6be0602c9cb7e0293002c4edb9bae6f2c402dce1fccfc6cadf",
    ("std12", 2, 8): "a1ce3c51268dd7b3343458160f178e13fc8cc13de6d8b324eeabfab0144bb751",
    ("std12", 3, 8): "5d43878b3b4e632a66a1d66ac7a5da45138496da45fa8d30f622f4d50d4f5569",
    ("clr12", 1, 8): "a23a5bedb2616edb7fa36776c41f1648ab49109114a0339327d6e6bafa3eb7c7",
    ("clr12", 2, 8): "895fa83d99017d275d69d6ed233728af34ea34f710b4ff96b055c596e9c3a044",
    ("clr12", 3, 8): "c225f2d9628446fc9c658592e2315ef1f648d7d45e08c0bb0c86c36ba59bd085",
    ("custom12", 1, 8): "e228bdb84762c0432609aab6132701c6344280a68b38646309635973a196e0fa",
    ("custom12", 2, 8): "80a7de420654ad867a07c5d22b8aaac0fc46b39db69d748e80dddb67aa0d4736",
    ("custom12", 3, 8): "6037053f0d9363d1fcf7d487b2b37546838ea7fd5392c194667b5e5d77aef54f",
}


@pytest.mark.parametrize("key", list(INGEST_DIGESTS), ids=lambda k: "-".join(str(v) for v in k))
def test_ingest_walks_are_unchanged(key):
    cfg, seed, scale = key
    ops = cs.generate(cfg, seed, scale=scale)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == INGEST_DIGESTS[key]
    assert ops == cs.generate(cfg, seed, scale=scale, profile="ingest")


def _run(cfg, seed, mutant=None):
    ops = cs.generate(cfg, seed, scale=SCALE)
    return cs.run_walk(ops, lambda name, model: FakeBackend(name, model, mutant))


@pytest.mark.parametrize("cfg,seed", _walks())
def test_faithful_fake_passes(cfg, seed):
    stats = _run(cfg, seed)
    assert stats["ops"] >= 30


def test_walks_hold_the_required_runs():
    """each walk contains the three runs without a synchronising call inside (callseq.generate); each sigma walk the runs
    of callseq.generate_sigma"""
    for cfg, seed in _walks():
        names = [op[0] for op in cs.generate(cfg, seed, scale=SCALE)]
        text = " ".join(names)
        assert "epoch_async online" in text and ("online prefetch commit" in text or "online stage commit" in text)
        assert any(f"epoch_async {a} {b}" in text for a in ("prefetch", "stage") for b in ("prefetch", "stage"))
        assert any(names[i] == "p2" and names[i + 1] in ("prefetch", "stage") and names[i + 2] == "p2"
                   for i in range(len(names) - 2))
        nulls = [op for op in cs.generate(cfg, seed, scale=SCALE) if op[0] == "online" and op[1]["mode"] == "null"]
        assert nulls
        if cs.stages_ahead(cs.CONFIGS[cfg]):
            # a lane = node range, a prefetch staged ahead behind it, a chain-kernel range
            c = cs.chain_max_nodes(cs.CONFIGS[cfg])
            ops = cs.generate(cfg, seed, scale=SCALE)
            span = lambda op: op[1]["n1"] - op[1]["n0"]
            assert any(ops[i][0] == "p2" and span(ops[i]) > c and ops[i + 1][0] in ("prefetch", "stage") and
                       ops[i + 2][0] == "p2" and 0 < span(ops[i + 2]) <= c for i in range(len(ops) - 2)), (cfg, seed)
    _sigma_walks_hold_the_required_runs()


@pytest.mark.parametrize("mutant", ["a", "b", "c", "d"])
def test_mutants_are_caught(mutant):
    caught = []
    for cfg, seed in _walks():
        try:
            _run(cfg, seed, mutant)
        except cs.WalkFailure as e:
            caught.append((cfg, seed, str(e).splitlines()[0]))
    assert caught, f"mutant {mutant} was not caught by any walk"


def test_failure_report_names_seed_ops_and_element():
    with pytest.raises(cs.WalkFailure) as e:
        _run("std12", 2, "c")
    text = str(e.value)
    assert "seed 2" in text and "replay(ops) with ops = [('config'" in text and "element" in text


# ---- the sigma profile -------------------------------------------------------------------------------------------------
NEW_OPS = {"sigma_mode", "sigma_flush", "compaction", "upload_empty", "epoch_masked", "topk", "bmd", "bmu_masked"} | set(cs.READERS)


def test_new_ops_stay_out_of_the_ingest_walks():
    for cfg in cs.CONFIGS:
        for seed in SEEDS:
            for scale in (1, SCALE):
                ops = cs.generate(cfg, seed, scale=scale)
                assert not NEW_OPS & {op[0] for op in ops}
                assert not any(op[0] == "set_state" and op[1]["parts"] in ("map_only", "weight_only") for op in ops)


def test_std80_reaches_the_two_quad_launch():
    """100 node groups x 7 column blocks: more than two thirds of a round of 1024 workgroups, with the compaction (the
    compacted pitch, the depth rounded up to 32 columns) and without; the older configurations stay on the one-quad form"""
    cfg = cs.CONFIGS["std80"]
    D = po.length(cfg["tr"], cfg["J"])
    groups = (cfg["W"] * cfg["H"] + 63) // 64
    dense, compacted = ((D + 3) // 4 + 7) // 8, ((D + 31) // 32 * 32 // 4 + 7) // 8
    assert (groups, dense, compacted) == (100, 7, 7)
    assert cs.two_quad_launch(cfg) == (700, True) and 3 * groups * compacted > 2 * 1024
    assert D % 4 == 0 and cs.defers(cfg)
    for name in ("std48", "med48"):
        assert cs.defers(cs.CONFIGS[name]) and not cs.two_quad_launch(cs.CONFIGS[name])[1]
    for name in ("std12", "clr12", "custom12"):
        assert not cs.SigmaRecord(cs.CONFIGS[name]).can_defer


@pytest.mark.parametrize("cfg,mode,seed", _sigma_walks())
def test_faithful_fake_passes_sigma_walks(cfg, mode, seed):
    stats = _faithful_sigma(cfg, mode, seed)
    assert stats["ops"] >= 40
    if cfg not in DEFERRING:
        assert stats["sigma"] == (0, 0, 0, 0)       # the header's "always eager"


@pytest.mark.parametrize("cfg", DEFERRING)
@pytest.mark.parametrize("mode", MODES)
def test_gpu_seeds_defer_drop_and_materialise(cfg, mode):
    """what test_sigma_walk_matches_oracle asserts of the library's counters holds for the walks it runs: a condition on
    the inputs.  The generator draws some ops by the chunk's size (the online op, the similarity's min_hits), so a walk at
    this file's scale need not be the GPU test's walk: the second half below traces the GPU test's own walks, at its scale,
    through the contract alone."""
    for seed in GPU_SEEDS:
        deferred, dropped, materialised, _ = _faithful_sigma(cfg, mode, seed)["sigma"]
        assert min(deferred, dropped, materialised) >= 1, (seed, deferred, dropped, materialised)
        # ... and at the GPU test's scale, from the contract alone (no oracle): every op accepted
        ops = cs.generate(cfg, seed, profile="sigma", mode=mode)
        pending = [p for _, p in _pending_trace(cfg, ops)]
        names = [op[0] for op in ops[1:]]
        whole = [n in ("epoch", "epoch_async") for n in names]
        assert any(pending), seed                                                          # deferred
        assert any(p and w for p, w in zip(pending, whole)), seed                          # dropped
        assert any(p and n in cs.READERS + ("sigma_flush", "get_state") for p, n in zip(pending, names)), seed   # materialised


def _pending_trace(cfg, ops):
    """(op, a record is pending when the op is called) along a walk whose calls are all accepted, from the contract alone"""
    rec = cs.SigmaRecord(cs.CONFIGS[cfg])
    g = cs._Gen(cfg, 0, ops[0][1]["scale"])
    out = []
    for op in ops[1:]:
        out.append((op, rec.pending))
        rec.accepted(op, g.B, g.N)
        g.emit(op[0], **op[1])
    return out


def _sigma_walks_hold_the_required_runs():
    """each sigma walk of a deferring configuration holds the runs of callseq.generate_sigma, the record pending from the
    run's epoch to its last call; the others hold the same calls"""
    give = ("prefetch", "stage")
    for cfg, mode, seed in _sigma_walks():
        ops = cs.generate(cfg, seed, scale=SCALE, profile="sigma", mode=mode)
        assert ops[1] == ("sigma_mode", {"mode": mode})       # the first op after the config
        tr = _pending_trace(cfg, ops)
        names = [op[0] for op, _ in tr]
        pend = [p for _, p in tr]
        need = cfg in DEFERRING
        N = cs.CONFIGS[cfg]["W"] * cs.CONFIGS[cfg]["H"]
        whole = lambda op: op[0] in ("epoch", "epoch_async") or (op[0] == "p2" and (op[1]["n0"], op[1]["n1"]) == (0, N))

        def found(pattern, extra=lambda i: True, held=None):
            """a whole-map epoch followed by calls named by `pattern` (each a name or a tuple of names), the record
            pending when each of the first `held` of them (default: all) is called (deferring configurations)"""
            held = len(pattern) if held is None else held
            for i in range(len(tr) - len(pattern)):
                if not whole(tr[i][0]):
                    continue
                if all(names[i + 1 + k] in (q if isinstance(q, tuple) else (q,)) for k, q in enumerate(pattern)) and \
                        (not need or all(pend[i + 1 + k] for k in range(held))) and extra(i):
                    return True
            return False

        where = (cfg, mode, seed)
        assert found([give, "commit", cs.READERS]), where
        assert found(["set_last_bmu", "p2"], lambda i: not whole(tr[i + 2][0]) and
                     tr[i + 2][0][1]["sigma"] != tr[i][0][1]["sigma"]), where
        largest = int(np.argmax([b for b, _ in cs.CONFIGS[cfg]["chunks"]]))
        assert found(["upload", "sigma_flush"], lambda i: tr[i + 1][0][1]["chunk"] == largest), where
        assert found(["upload_empty", ("epoch", "epoch_async"), "get_state"], held=2), where      # (the epoch drops it)
        assert found(["online", "get_state"], lambda i: tr[i + 1][0][1]["mode"] == "null", held=1), where
        assert found(["set_state", "get_state"], lambda i: tr[i + 1][0][1]["parts"] == "weight_only", held=1), where
        # three whole-map epochs with only keep-class calls between them, then a reader: the third defers under AUTO
        ok = False
        for i, (op, p) in enumerate(tr):
            if op[0] in cs.READERS and (p or not need):
                k, epochs = i - 1, 0
                while k >= 0 and names[k] in cs.SIGMA_KEEP and (names[k] != "p2" or whole(tr[k][0])):
                    epochs += whole(tr[k][0])
                    k -= 1
                ok = ok or epochs >= 3
        assert ok, where
        if cs.stages_ahead(cs.CONFIGS[cfg]):
            # the prefetch of the first run directly follows an asynchronous epoch or a whole-map range: staged ahead
            assert any(names[i] in give and names[i + 1] == "commit" and names[i + 2] in cs.READERS and
                       names[i - 1] in ("epoch_async", "p2") and (pend[i] or not need) for i in range(1, len(tr) - 2)), where


@pytest.mark.parametrize("mutant", ["e", "f", "g", "h", "i", "j", "k"])
def test_sigma_mutants_are_caught(mutant):
    caught = []
    for cfg, mode, seed in _sigma_walks():
        if cfg not in DEFERRING:
            continue
        try:
            _run_sigma(cfg, mode, seed, mutant)
        except cs.WalkFailure as e:
            caught.append((cfg, mode, seed, str(e).splitlines()[0]))
            break
    assert caught, f"mutant {mutant} was not caught by any walk"


def _failing_ops(failure):
    """the op list a WalkFailure prints: the last one is the op that failed"""
    return ast.literal_eval(str(failure).split("replay(ops) with ops = ", 1)[1])


@pytest.mark.parametrize("mutant", ["f", "g"])
def test_operand_mutants_are_caught_by_the_state_alone(mutant):
    """f and g keep the counters right: it is the materialised sigmaMap that differs from the oracle's"""
    with pytest.raises(cs.WalkFailure) as e:
        for mode in MODES:
            _run_sigma("std48", mode, 1, mutant)
    first = str(e.value).splitlines()[0]
    assert "output 'sigma' differs" in first and "vsom_sigma_stats" not in first


@pytest.mark.parametrize("cfg,mode,seed", [(c, m, 1) for c in DEFERRING for m in MODES])
def test_mutant_h_is_caught_at_the_weight_only_set_state(cfg, mode, seed):
    """h is exact until a weight-only vsom_set_state meets a pending record: every walk passes up to that call, where the
    record that should have been materialised is still pending.  Left pending (the counters not compared), the record is
    later materialised over the new weight: a sigmaMap that is not the oracle's."""
    with pytest.raises(cs.WalkFailure) as e:
        _run_sigma(cfg, mode, seed, "h")
    assert "vsom_sigma_stats" in str(e.value).splitlines()[0]
    ops = _failing_ops(e.value)
    assert ops[-1][0] == "set_state" and ops[-1][1]["parts"] == "weight_only", ops[-1]
    # the same walk, the counters left out of the comparison: the state alone catches it, behind that call
    ops = cs.generate(cfg, seed, scale=SCALE, profile="sigma", mode=mode)
    blind = lambda name, model: _NoStats(name, model, "h")
    with pytest.raises(cs.WalkFailure) as e:
        cs.run_walk(ops, blind)
    assert "output 'sigma' differs" in str(e.value).splitlines()[0]
    done = _failing_ops(e.value)
    assert any(op[0] == "set_state" and op[1]["parts"] == "weight_only" for op in done[:-1]), done[-1]


class _NoStats(FakeBackend):
    """the fake reporting the model's own counters: only the state can tell it from the library"""

    def __init__(self, name, model, mutant):
        super().__init__(name, model, mutant)
        self.model = model

    def call(self, op, a):
        rc, msg, out = super().call(op, a)
        if rc == 0:
            rec = copy.copy(self.model.sig)
            rec.accepted(op, self.model.B, self.model.N)
            out["sigma_stats"] = rec.stats()
        else:
            out["sigma_stats"] = self.model.sig.stats()
        return rc, msg, out
