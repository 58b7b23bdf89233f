"""CPU self-test of the call-sequence walk (tests/callseq.py): the same walks as tests/test_gpu_call_sequences.py, run
against fake contexts backed by a second oracle.  The faithful fake must pass; each mutant -- a fake with one of the
ingest bugs the walk exists to find -- must be caught by at least one seed.  This shows, without a GPU, that the walk
can see that class of bug.

The sigma profile's walks run against the same fake, which then also models the pending sigmaMap: a deferred epoch computes
the whole epoch and withholds the new sigmaMap / S rows, keeping what the library's record keeps (the epoch's rows, its
lastBMU, its sigma); a materialisation computes them from that record, a drop discards it.  Mutants e-k break that
bookkeeping the ways an entry point wrongly listed as keeping the record -- or a record made from the wrong operands --
would.  The ingest walks themselves are pinned by digest: the generator's new ops must never enter their draws.

The accum profile's walks (the accumulated batch epoch) run against the same fake, which keeps what the model keeps -- the
open epoch's rows, validity and lastBMU -- on its own oracle.  Mutants l-r break it the ways hand-kept host state can be
wrong between calls that do not block.  The sigma walks are pinned by digest too, and what the GPU test asserts of its
walks' counts is checked here as a condition on the inputs.

The ensemble profile's walks (callseq.generate_ensemble) run against FakeEnsemble, the members and ensembles on a second set
of oracles.  The faithful fake passes the walks the GPU test runs and meets the conditions it asserts
(callseq.ens_conditions); the walks are pinned by digest; each of the eight mutants -- the ways an ensemble call can differ
from the single calls on its members in turn -- is caught by one of them."""
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
      k  vsom_set_last_bmu / vsom_get_mse count as a read
    and, in the accum profile (the accumulated epoch):
      l  the accumulators restart with every chunk, so end gives the last chunk's batch map (what the reference does)
      m  abort writes the partial accumulators as end would
      n  the running MSE divides by the chunk's rows, not by total_rows
      o  a plain chunk behind a masked one does not walk the columns dirty so far: those columns drop its rows
      p  a refused end (rows missing) closes the epoch
      q  the masked chunk reads its validity after the call returned, and sees the zeros the caller wrote there
      r  begin does not clear the ever-dirty list: the next end writes those columns from the previous epoch's side
         buffers
      s  a chunk call does not look whether the next chunk is staged ahead over the current rows"""

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
        self.sigma_profile = model.profile in ("sigma", "accum")
        self.stale = None                   # mutant r: (columns, their map and sigmaMap values) the last epoch left
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
        return name in cs.SIGMA_KEEP or name in cs.ACCUM_KEEP

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
        if self.cfg["tr"] == po.CLR and name == "distances_raw" and not p["from_map"]:
            return cs.VSOM_ERR_UNSUPPORTED, "needs depth == sample length", {}
        if name == "commit" and m.pending is None:
            return cs.VSOM_ERR_INVALID, "no prefetched chunk to commit", {}
        if name in cs.ACCUM_OPS:
            return self._accum(op, a)
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

    # ---- the accumulated epoch ----
    @staticmethod
    def _dirty(parts):
        """the columns that had an invalid entry in these chunks"""
        if not parts:
            return np.zeros(0, np.int64)
        return np.flatnonzero(~np.concatenate([v for _, v, _ in parts]).all(axis=0))

    def _accum(self, op, a):
        name, p = op
        m = self.m
        self.rows_free = False
        why = m.accum_refusal(op, staged=self.ahead_rows and self.mutant != "s")
        if why is not None:
            if self.mutant == "p" and why == "rows accumulated":
                m.acc = None
            if self.mutant == "d":
                m.som.train_single(m.chunks[0][0], 0.1, 1.0, 0, 0)
            return cs.VSOM_ERR_INVALID, f"{name}: {why}", {}
        chunk = name in ("accum_chunk", "accum_chunk_masked") and m.B > 0
        if chunk and self.mutant == "l":
            m.acc["parts"].clear()
        if chunk and self.mutant == "n":
            m.acc["divisor"] = m.B
        if name == "accum_chunk_masked" and self.mutant == "q":
            a = {"valid": np.zeros_like(a["valid"])}
        if name == "accum_abort" and self.mutant == "m":
            newmap, newsig, weight = m.accum_phase2(m.acc)
            m.som.set_state(map=newmap, sigma=newsig, weight=weight)
        stale = self.stale
        if name in ("accum_end", "accum_abort") and self.mutant == "r":
            dirty = self._dirty(m.acc["parts"])
            if dirty.size:
                newmap, newsig, _ = m.accum_phase2(m.acc)
                self.stale = (dirty, newmap[:, dirty], newsig[:, dirty])
        dirty_so_far = self._dirty(m.acc["parts"]) if name == "accum_chunk" and chunk else ()
        out = self._apply(op, a)
        if len(dirty_so_far) and self.mutant == "o":
            X, v, lb = m.acc["parts"][-1]
            v = v.copy()
            v[:, dirty_so_far] = False
            m.acc["parts"][-1] = (X, v, lb)
        if name == "accum_end" and self.mutant == "r" and stale is not None:
            cols, oldmap, oldsig = stale
            newmap, newsig = m.som.map.copy(), m.som.sigma.copy()
            newmap[:, cols] = oldmap
            newsig[:, cols] = oldsig
            m.som.set_state(map=newmap, sigma=newsig)
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


# sha256(repr(generate(cfg, seed, scale=scale, profile="sigma", mode=mode))) of the sigma walks, recorded before the accum
# profile existed
SIGMA_DIGESTS = {
    ("std48", "lazy", 1, 1): "c5d42f13acfaa377e9a00984095e92b18d819da7c647f5aa00ca06983bdaa68a",
    ("std48", "lazy", 2, 1): "ea71f358828c84e15a4d9b5341edc720c2d76f0378a050237ed218032b74f9be",
    ("std48", "lazy", 3, 1): "1ccde8ea17863066e4ab9a5c0f3586bd3ab7e458f89cb2c55f37528dd69c7427",
    ("std48", "auto", 1, 1): "e0e5337a98450315b41ad3d72c9bcd71cb33e78c5cb8fa64ac2beff89f27be20",
    ("std48", "auto", 2, 1): "c3730d82aaeddf32ec4365cf329fc666de31f970619feae9be3a617f9c124833",
    ("std48", "auto", 3, 1): "31a06209350fd0267dfc189d5d19d07e75ee5a4b3c7b297038a1b466f0907049",
    ("med48", "lazy", 1, 1): "0fd7f96979deda441dfa30c2377f8bb595cf67f1f8d0d183bd3238f86c8e734c",
    ("med48", "lazy", 2, 1): "cb77a5a918cf54ea98ec33e2be24ce9665c4bd1e054e6d337ce8bc020af198b8",
    ("med48", "lazy", 3, 1): "6c0f26f12eb51ad190d1e0f65c956def18307ba29381c895a09ddd2762d96515",
    ("med48", "auto", 1, 1): "50a3777947103fd31af40384e98b0ea80da40d1bea6affa9d8fe3a5604969ca1",
    ("med48", "auto", 2, 1): "fe0ff1532e6c0971b455cde7c1210678acaa0def22ffdb02339280d5983c9621",
    ("med48", "auto", 3, 1): "cb9e2718f31d71f97eb71733401b11a3254e6293aa3b2f35d9f5ac751af85233",
    ("std12", "lazy", 1, 1): "e79b7998e40fef4abdabf5bb565543cba1add9a363be4f631a1a3a0a7da76dea",
    ("std12", "lazy", 2, 1): "bf695fe6a6a200827bdcc24a7651d3b3970373da0e22547206d4658057b11796",
    ("std12", "lazy", 3, 1): "f3f8a84e17f71de310a4be0cfd604ac223d654e2975419bb05b6205369b6aaaf",
    ("std12", "auto", 1, 1): "d5ab1d2b06dc19ee822d372ccba86a663ede8d4fd0b1b421cc78ef8596632586",
    ("std12", "auto", 2, 1): "bf2c36a846c1b75e90b36839bd0eb53ba14f75bfab45fd3acdc1f785b5a35108",
    ("std12", "auto", 3, 1): "55d7bc9909abc4b1731abcf9c58fa8ddb4b2c8cbd754d6f23975c843502249f7",
    ("clr12", "lazy", 1, 1): "7a73cee9ee7dc9991a49ba175e426e45467fa35127075abe80da3948ae5e61c5",
    ("clr12", "lazy", 2, 1): "14d58a998c0a51fa7a1e1d174f47e1a3f3671e5226239ae580bfb691678ae272",
    ("clr12", "lazy", 3, 1): "af7e7a6650b7f1c7cb5a2bcbd342965f3b7988a31e7886373a405b2ec514bf00",
    ("clr12", "auto", 1, 1): "bb309f4ff1f46d00185f81ba17b8be00072ee35a786e290632aa7bcb3b6a72e7",
    ("clr12", "auto", 2, 1): "61e0de3314664fa986a7840b444ef1b1134b47470fab32a0a8f26f5f71a37b79",
    ("clr12", "auto", 3, 1): "6add8b6cc01fa270aa7e3dfb214571aa98396b9f07f86523d8296bd9e19e9268",
    ("custom12", "lazy", 1, 1): "c92941cdfbf9ae526955ffc4f2605c527743a7b35d8b754e5e87ca87aa9c3a08",
    ("custom12", "lazy", 2, 1): "72404b69a0cf314834a623a5d009044b1f2451a745512d47723c7939c1ba2935",
    ("custom12", "lazy", 3, 1): "b4b49d838bd8b871f7bcf70f3e924ad6514040e4ee881dc7e6170a09afe20809",
    ("custom12", "auto", 1, 1): "22f7d472a19eac7e8bc05ee8c8f8351c4df5ed7f3c0503445a51a8adf4cde2e0",
    ("custom12", "auto", 2, 1): "7f1214e8de384dc553f607c1314fdbd36e2a1aff932095e27be549c0f04b5729",
    ("custom12", "auto", 3, 1): "7f54bf87fedbc02899b01c53972a02bef30feebf0ec746da7277287aeec135b2",
    ("std80", "lazy", 1, 1): "6fac3739f21ee8cb3042fe2f658abd93078516948206f36f4b4ceb51ac3e2add",
    ("std80", "lazy", 2, 1): "3e06621520f90e42250498c2f84e336cce7e0ffe0dfe83245ec8ceb5bd1757dc",
    ("std80", "lazy", 3, 1): "f40f03372042af2e257fff3487998b2b59d2d1cd9fb2aa4b0a90e8f0e6df5d2f",
    ("std80", "auto", 1, 1): "f8e553a73eb237063893cf637604015de970033f7ad797d35b858f96a288f2a3",
    ("std80", "auto", 2, 1): "62b58734f611bc4fd8c2b7332411772074dc41ccbd8689badd260e7f52f2d54c",
    ("std80", "auto", 3, 1): "4cd4987e5df6cc9dccbd6b8ae05b168bf7e65fb9c65a38052fcc4734884c8099",
    ("std48", "lazy", 1, 8): "4d1e67c0d9331b5a4a4912559b4d5390962e2d2261b39f818d5870037f82bd10",
    ("std48", "lazy", 2, 8): "beed7556ae63a06765ea284c442c0d62de054547fda9523ea3371f165f3b01d7",
    ("std48", "lazy", 3, 8): "c1883f718f9169ad2d7706c4e13922b75c455ec1144f6f6bd4e73e1a4735cfe7",
    ("std48", "auto", 1, 8): "32c839b5e80197420026b9904a34bca4051b10d6f04c05e3e935242b4bd8eb19",
    ("std48", "auto", 2, 8): "1893bd421666801dce7043b8edeb269f597a0b1d6ab5fea5b17b92317d2dfaea",
    ("std48", "auto", 3, 8): "dd7cdd3d76d61bf97b853501c6fbc881b5ac074b5c2cc2c89e0452598d5c61b6",
    ("med48", "lazy", 1, 8): "877b53ddfa12fe2d194abb72ba7ef8284930f0454117d7a1e9afaaccb221b743",
    ("med48", "lazy", 2, 8): "94d8507d697f6f6256863695e1fa3fff7d454d4a72df4132c2871b4020211074",
    ("med48", "lazy", 3, 8): "664d3048c088e6327eae565d8811418a48882d11506221d5628d5c6143662275",
    ("med48", "auto", 1, 8): "2fb5f35ec9253348c278fb403538910eda92629ad4635a4543bc61a99e1a0512",
    ("med48", "auto", 2, 8): "04a344ecf3106df6b28fd4a3088fea3fd8e474e708866a0c30a5b44ac5534c8f",
    ("med48", "auto", 3, 8): "a9a3f96926c0c36aa47251b94ba58a9726ddbcff204a17d2b052c273d0228953",
    ("std12", "lazy", 1, 8): "f0c293f1324528b3b3859bbb6297d4c8f040204a5aae416e9123eefd0714c863",
    ("std12", "lazy", 2, 8): "d1b8ba5b4a8bb5b867889ad597824d3cd32ca8a76469ee3b5f46f65d5d68f16d",
    ("std12", "lazy", 3, 8): "f46001258a5711f51bf5c47b885f43dba0127a44f64496fa597cc531de3cdadf",
    ("std12", "auto", 1, 8): "20d5f2075fe390cac02722d18ecfaabda15f475fdc9de7b6a4f2109636b56b46",
    ("std12", "auto", 2, 8): "066b9bf144407ca2aec606b3ac5e905beeb5014ca2ef1a6a8c69ffd49e807dbd",
    ("std12", "auto", 3, 8): "9fe814b87dca5fab6e80aec50cdf22b9bff17360922bced04cc6ec1d058d6a81",
    ("clr12", "lazy", 1, 8): "ddae8768dc02e25ac5234548a091b8e5439596913cecb570f5ab87091ffe3227",
    ("clr12", "lazy", 2, 8): "102af3e7560bb5f565baacf293f2208a4d7c6417ab0e49130897de4ca8551e69",
    ("clr12", "lazy", 3, 8): "08da026274d34e4d74103b7e8ace0ead83c6d9e54d490a874784c345a77ab351",
    ("clr12", "auto", 1, 8): "d8bbb9d02aff7f9c1324e96db733558281f3baa263907781e39dbbb3872334de",
    ("clr12", "auto", 2, 8): "9825488746e0fca08e4e2a6ac32dc3f55489428ebb71de1e9deb47c739ace3ba",
    ("clr12", "auto", 3, 8): "486ba7cfdfd16b78fca9b4ea984fbf641bff17710c72a699483b5b93de887f61",
    ("custom12", "lazy", 1, 8): "b3ab6acc4389b989354440cb79eb3c6f7b537a91a60477af6323a24105cd5c24",
    ("custom12", "lazy", 2, 8): "0660e92a63bd85bfc8ee25140b2bb3e23d2fac8da1626c618f059712f4f18408",
    ("custom12", "lazy", 3, 8): "e285fb11f71c5489611f967fe9a50008e1a05388edecb1293c2595a5e0ad379d",
    ("custom12", "auto", 1, 8): "7ead2a3e3a1078e3c50f4fbe238ae4704bce2f28b3dddfdb52dd3ddc13840e2b",
    ("custom12", "auto", 2, 8): "c18235d562556e06f63b27c011c9b09ec088898acff7ada87e457a2034c78216",
    ("custom12", "auto", 3, 8): "98a224fdc6b772f882e301086feb74dfbd6ab1d763114ba6abe669f0c9f0d6c6",
    ("std80", "lazy", 1, 8): "395c930a1b25129cc2a54269c6e447a334c0cf6e9ff181f7737772b216f5f6eb",
    ("std80", "lazy", 2, 8): "cdada319d51a04ed3f648d516ffcf83eb7a5d0949914a18c37b07e4e64f3b589",
    ("std80", "lazy", 3, 8): "bf15a30cf2a1902e93ef70c09b912dfcbd3fbbd93010109bfdea15cc8d740440",
    ("std80", "auto", 1, 8): "de13e40c160d2a878e772728f55a41175c1e8d8d80f2a839c127547c3f4c4928",
    ("std80", "auto", 2, 8): "cdb7d458d2db53a806cbc1fe99b2b21ac3ec1da7b9c6f2a51ca83fe39a30cc43",
    ("std80", "auto", 3, 8): "05a51c6c39ed06afd99c719280721d8c30df8a5c1e6318368efed2f96ed2b736",
}


@pytest.mark.parametrize("key", list(SIGMA_DIGESTS), ids=lambda k: "-".join(str(v) for v in k))
def test_sigma_walks_are_unchanged(key):
    cfg, mode, seed, scale = key
    ops = cs.generate(cfg, seed, scale=scale, profile="sigma", mode=mode)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == SIGMA_DIGESTS[key]


# ---- the accum profile -------------------------------------------------------------------------------------------------
ACCUM_NEW_OPS = set(cs.ACCUM_OPS) | set(cs.MASKED_SCORES) | {"update_mode", "run", "run_end"}
ACCEPTING = ("std48", "med48", "std12", "std80")       # vsom_batch_accum_begin opens an epoch (callseq.accepts_accum)


def test_accum_ops_stay_out_of_the_other_walks():
    assert ACCEPTING == tuple(c for c in cs.CONFIGS if cs.accepts_accum(cs.CONFIGS[c]))
    for cfg in cs.CONFIGS:
        for seed in SEEDS:
            for scale in (1, SCALE):
                walks = [cs.generate(cfg, seed, scale=scale)]
                walks += [cs.generate(cfg, seed, scale=scale, profile="sigma", mode=mode) for mode in MODES]
                for ops in walks:
                    assert not ACCUM_NEW_OPS & {op[0] for op in ops}
                    assert not any("poisoned" in op[1] for op in ops)
                    assert all(op[1]["chunk"] < len(cs.CONFIGS[cfg]["chunks"]) for op in ops if "chunk" in op[1])


def _accum_walks():
    return [(c, m, s) for c in cs.CONFIGS for m in MODES for s in GPU_SEEDS]


def _accum_ops(cfg, mode, seed, scale=SCALE):
    return cs.generate(cfg, seed, n_ops=cs.ACCUM_DRAWS, scale=scale, profile="accum", mode=mode)


def _run_accum(cfg, mode, seed, mutant=None, scale=SCALE):
    return cs.run_walk(_accum_ops(cfg, mode, seed, scale), lambda name, model: FakeBackend(name, model, mutant))


@functools.lru_cache(maxsize=None)
def _faithful_accum(cfg, mode, seed, scale=SCALE):
    return _run_accum(cfg, mode, seed, scale=scale)


def _gpu_conditions(cfg, stats):
    """what tests/test_gpu_call_sequences.py, test_accum_walk_matches_oracle, asserts of a walk's counts"""
    a = stats["accum"]
    assert stats["ops"] >= 50
    if cfg in ACCEPTING:
        assert a["chunks"] >= 8 and a["masked"] >= 3 and a["ends"] >= 2 and a["aborts"] >= 1, a
        assert a["staged"] == (1 if cs.stages_ahead(cs.CONFIGS[cfg]) else 0), a
    else:
        assert not any(a.values()), a               # every begin refused, so every other call too


@pytest.mark.parametrize("cfg,mode,seed", _accum_walks())
def test_faithful_fake_passes_accum_walks(cfg, mode, seed):
    stats = _faithful_accum(cfg, mode, seed)
    _gpu_conditions(cfg, stats)
    if cfg not in DEFERRING:
        assert stats["sigma"] == (0, 0, 0, 0)
    # run 5: refused where a prefetch behind an asynchronous epoch stages ahead (run_walk requires it there), nowhere else
    assert stats["accum"]["staged"] == (1 if cs.stages_ahead(cs.CONFIGS[cfg]) else 0), stats


def _accum_trace(cfg, ops):
    """[(run, op, refusal, a sigmaMap record is pending at the call)] along an accum walk, from the contract alone (no
    oracle): callseq.Model.accum_refusal on a stand-in that knows the open epoch's rows and the chunk's size, and
    callseq.SigmaRecord.  A call that only a chunk staged ahead could refuse counts as accepted."""
    import types
    conf = cs.CONFIGS[cfg]
    rec = cs.SigmaRecord(conf)
    g = cs._Gen(cfg, 0, ops[0][1]["scale"], "accum", ops[0][1]["mode"])
    m = types.SimpleNamespace(cfg=conf, acc=None, update_mode=cs.UPDATE_STRICT, X=None, B=0)
    out, run = [], None
    for op in ops[1:]:
        name, p = op
        if name in ("run", "run_end"):
            run = p["id"] if name == "run" else None
            continue
        why = cs.Model.accum_refusal(m, op) if name in cs.ACCUM_OPS else None
        if why is None and ((conf["custom"] and name in cs.CUSTOM_REFUSED) or (conf["tr"] == po.CLR and name in cs.CLR_REFUSED)):
            why = "custom / CLR"
        out.append((run, op, why, rec.pending))
        g.emit(name, **p)
        if name in ("upload", "upload_empty", "commit"):
            m.X = True
        m.B = g.B
        if why is not None:
            rec.read()
            continue
        rec.accepted(op, g.B, g.N)
        if name == "accum_begin":
            m.acc = {"rows": 0, "total": p["total"]}
        elif name in ("accum_chunk", "accum_chunk_masked"):
            m.acc["rows"] += g.B
        elif name in ("accum_end", "accum_abort"):
            m.acc = None
        elif name == "update_mode":
            m.update_mode = p["mode"]
    return out


def _trace_counts(trace):
    """the counts of callseq.run_walk's stats["accum"], run 5's calls left out (its first chunk call may be refused)"""
    n = {"chunks": 0, "masked": 0, "ends": 0, "aborts": 0}
    for run, (name, p), why, _ in trace:
        if why is None and run != 5 and name in cs.ACCUM_OPS[1:]:
            if name in ("accum_chunk", "accum_chunk_masked"):
                n["chunks"] += 1                    # (an empty chunk is counted here and not there: see the caller)
                n["masked"] += name == "accum_chunk_masked"
            else:
                n[name[6:] + "s"] += 1
    return n


@pytest.mark.parametrize("cfg", list(cs.CONFIGS))
def test_gpu_accum_walks_meet_their_conditions(cfg):
    """What test_accum_walk_matches_oracle asserts of its walks' counts is a condition on the inputs: here it is checked at
    that test's own scale -- against the faithful fake where the model can afford it (the 12 x 12 maps), from the contract
    alone for the others (_accum_trace: no refusal but the ones the header names, so the GPU test cannot pass by having
    everything refused)."""
    for mode in MODES:
        for seed in GPU_SEEDS:
            ops = _accum_ops(cfg, mode, seed, scale=1)
            trace = _accum_trace(cfg, ops)
            n = _trace_counts(trace)
            empty = sum(1 for run, op, why, _ in trace if run == 6 and why is None and op[0] == "accum_chunk") - 2
            if cfg in ACCEPTING:
                assert empty == 1                   # run 6: two chunks and the empty one
                assert n["chunks"] - empty >= 8 and n["masked"] >= 3 and n["ends"] >= 2 and n["aborts"] >= 1, (mode, seed, n)
            else:
                assert not any(n.values())
            assert len(trace) >= 50
            if cfg in ("std12", "clr12", "custom12"):
                stats = _faithful_accum(cfg, mode, seed, 1)
                _gpu_conditions(cfg, stats)
                if cfg in ACCEPTING:                # the trace is the walk: run 5 adds its two chunks and its abort
                    a = stats["accum"]
                    assert (a["chunks"], a["masked"], a["ends"], a["aborts"], a["staged"]) == \
                        (n["chunks"] - empty + 2, n["masked"], n["ends"], n["aborts"] + 1, 0)


RUN6_REFUSALS = ["no chunk loaded"] + ["no accumulated epoch is open"] * 3 + \
    ["valid_host is null", "strict update mode", "already open", "valid_host is null", "exceed total_rows", "rows accumulated"]


def test_accum_walks_hold_the_required_runs():
    """from the op lists alone: every accum walk holds runs 1-9 of callseq's module docstring, no call of a no-wait run
    waits for the stream, and by the contract no call of runs 1-4 and 6-9 is refused but the refusals run 6 is made of"""
    loads = ("upload", "prefetch", "stage", "commit")
    for scale in (SCALE, 1):
        for cfg, mode, seed in _accum_walks():
            where = (cfg, mode, seed, scale)
            conf = cs.CONFIGS[cfg]
            ops = _accum_ops(cfg, mode, seed, scale)
            assert ops[1] == ("sigma_mode", {"mode": mode})
            trace = _accum_trace(cfg, ops)
            runs = {r: [t for t in trace if t[0] == r] for r in cs.RUNS}
            names = {r: [t[1][0] for t in runs[r]] for r in cs.RUNS}
            chunks = {r: [t[1] for t in runs[r] if t[1][0] in ("accum_chunk", "accum_chunk_masked")] for r in cs.RUNS}
            sizes = cs._Gen(cfg, 0, scale, "accum", mode).sizes
            assert all(names[r] for r in cs.RUNS), where

            def between_chunks(r, wanted):
                """the names of `wanted` that stand between the first and the last chunk call of run r, in order"""
                at = [i for i, n in enumerate(names[r]) if n in ("accum_chunk", "accum_chunk_masked")]
                return [n for n in names[r][at[0]:at[-1]] if n in wanted]

            # no refusal by the contract, but run 6's (and everything behind a refused begin)
            for r in cs.RUNS:
                why = [t[2] for t in runs[r] if t[2] is not None]
                if cfg not in ACCEPTING:
                    assert all(t[2] is not None for t in runs[r] if t[1][0] in cs.ACCUM_OPS), where
                elif r == 6:
                    assert why == RUN6_REFUSALS, (where, why)
                else:
                    assert not why, (where, r, why)
            # the no-wait runs
            for r in cs.NO_WAIT_RUNS:
                assert names[r][0] == "accum_begin" and names[r][-1] == "accum_end", where
                assert runs[r][0][1][1]["first"] is True, where
                for _, (name, p), _, _ in runs[r][1:-1]:
                    if r == 2 and name == "topk":
                        continue
                    assert name in cs.NO_WAIT_OPS, (where, r, name)
                    assert name != "upload" or p["asynchronous"], (where, r)
                    assert name != "prefetch" or p["src"] == "pinned", (where, r)
            # 1: three masked chunks or more and nothing else; a row without a valid column
            assert len(chunks[1]) >= 3 and all(c[0] == "accum_chunk_masked" for c in chunks[1]), where
            assert [c[1]["k"] for c in chunks[1]] == list(range(len(chunks[1]))), where
            assert len({c[1]["seed"] for c in chunks[1]}) == 1, where
            assert any(c[1].get("full") and c[1]["form"] == "rows" for c in chunks[1]), where
            rows1 = [t[1][1]["chunk"] for t in runs[1] if t[1][0] in ("upload", "prefetch", "stage")]
            if len(cs.maskable(conf, True)) > 1:       # different rows behind each other: a late reader would see them
                assert all(x != y for x, y in zip(rows1, rows1[1:])), (where, rows1)
            # 2: growing chunks, the largest last, one top-8 query on a 64-row window between two chunk calls
            up = [sizes[t[1][1]["chunk"]] for t in runs[2] if t[1][0] in ("upload", "prefetch", "stage")]
            assert len(up) >= 3 and up == sorted(up) and up[-1] == max(sizes) and up[0] < up[-1], (where, up)
            assert all(c[0] == "accum_chunk" for c in chunks[2]) and len(chunks[2]) == len(up), where
            assert between_chunks(2, ("topk",)) == ["topk"] and names[2].count("topk") == 1, where
            q = [t[1][1] for t in runs[2] if t[1][0] == "topk"][0]
            assert q["k"] == 8 and q["r1"] - q["r0"] == min(64, up[-2]), (where, q)
            # 3: plain, masked, plain in a non-first epoch, set_last_bmu between each load and its chunk call
            assert [c[0] for c in chunks[3]] == ["accum_chunk", "accum_chunk_masked", "accum_chunk"], where
            assert runs[3][0][1][0] == "accum_begin" and runs[3][0][1][1]["first"] is False, where
            for i, n in enumerate(names[3]):
                if n in ("accum_chunk", "accum_chunk_masked"):
                    assert names[3][i - 1] == "set_last_bmu" and names[3][i - 2] in loads, where
            assert names[3][-1] == "accum_end", where
            # 4: an abort behind two chunks or more, one masked; get_state; a plain epoch
            a = names[4].index("accum_abort")
            first = [n for n in names[4][:a] if n in ("accum_chunk", "accum_chunk_masked")]
            assert len(first) >= 2 and "accum_chunk_masked" in first, where
            assert names[4][a + 1] == "get_state" and names[4][a + 2] == "accum_begin", where
            rest = names[4][a + 2:]
            assert "accum_chunk" in rest and "accum_chunk_masked" not in rest and rest[-1] == "accum_end", where
            # 5: the stage-ahead refusal
            assert names[5] == ["epoch_async", "prefetch", "accum_begin", "accum_chunk", "commit", "accum_chunk",
                                "accum_abort"], where
            # 6: the empty epoch, the empty chunk (the refusals: above)
            assert any(names[6][i:i + 2] == ["accum_begin", "accum_end"] and runs[6][i][1][1]["total"] == 0
                       for i in range(len(names[6]))), where
            assert any(names[6][i:i + 2] == ["upload_empty", "accum_chunk"] and (runs[6][i + 1][2] is None or
                                                                                 cfg not in ACCEPTING)
                       for i in range(len(names[6]))), where
            # 7: a pending record meets begin
            b = names[7].index("accum_begin")
            assert names[7][b - 1] == "epoch_async" and names[7][-1] == "accum_end", where
            if cfg in DEFERRING:
                assert runs[7][b][3] and not any(t[3] for t in runs[7][b + 1:]), where
            # 8: a map write and a single step at another sigma between two chunks; ended with end
            assert between_chunks(8, ("set_state", "single")) == ["set_state", "single"], where
            st = [t[1][1] for t in runs[8] if t[1][0] in ("set_state", "single")]
            assert st[0]["parts"] == "map" and st[1]["sigma"] != runs[8][0][1][1]["sigma"], where
            assert names[8][-1] == "accum_end" and "accum_abort" not in names[8], where
            # 9: the queries between two chunks
            got = between_chunks(9, cs.MASKED_SCORES + cs.ARENA + cs.READERS)
            assert got[:4] == ["similarity_masked", "evaluate_masked", "bmu_masked", "bmd"] and got[4] in cs.READERS, where
            assert len(got) == 5 and names[9][-1] == "accum_end", where


def test_accum_masks_are_engineered():
    """the dirty columns of an epoch's masked chunks: the border columns, a column invalid throughout, columns that turn
    dirty in the second and in the third masked chunk, MAX_DIRTY at the most; the rows a masked chunk call is given hold
    NaN / inf under every invalid entry of its mask and nowhere else, and every walk loads exactly those rows for it"""
    for cfg in ACCEPTING:
        conf = cs.CONFIGS[cfg]
        J = conf["J"]
        chunks = cs.chunk_data(cfg, 1, 1, "accum")
        assert len(cs.maskable(conf, True)) >= 2 or conf["W"] * conf["H"] * 300 <= cs.MASK_DISTANCES
        for i in cs.maskable(conf):
            X = chunks[i]
            assert np.isfinite(X).all()
            dirty = []
            for form in ("rows", "one_mask"):
                for k in range(3):
                    v = np.broadcast_to(cs.accum_mask(77, k, form, False, X) != 0, X.shape)
                    P = cs.poisoned_rows(X, 77, k, form, False)
                    assert (np.isfinite(P) == v).all() and (P[v] == X[v]).all()
                    assert (np.broadcast_to(cs.accum_mask(77, k, form, False, P) != 0, X.shape) == v).all()
                    dirty.append(set(np.flatnonzero(~v.all(axis=0))))
                    if form == "rows":
                        assert v.any(axis=1).all()
            assert len(set.union(*dirty[:3])) <= cs.MAX_DIRTY and len(set.union(*dirty[3:])) <= cs.MAX_DIRTY
            assert set(cs.border_columns(J)) <= dirty[0]
            assert dirty[0] < dirty[1] < dirty[2]           # the dirty set grows: the fold kernel's fresh path
            dead = [d for d in range(J) if all(not np.broadcast_to(cs.accum_mask(77, k, f, False, X), X.shape)[:, d].any()
                                               for k in range(3) for f in ("rows", "one_mask"))]
            assert len(dead) == 1 and dead[0] not in cs.border_columns(J)
            full = cs.accum_mask(77, 0, "rows", True, X) != 0
            assert (~full.any(axis=1)).sum() == 1
            P = cs.poisoned_rows(X, 77, 0, "rows", True)
            assert (np.isfinite(P) == full).all() and (~np.isfinite(P)).all(axis=1).sum() == 1
    # every masked chunk call of a walk stands behind the load of its own poisoned rows
    for cfg, mode, seed in _accum_walks():
        ops = [op for op in _accum_ops(cfg, mode, seed) if op[0] not in ("set_last_bmu", "commit", "run", "run_end")]
        masked = [i for i, op in enumerate(ops) if op[0] == "accum_chunk_masked" and not op[1].get("null")]
        assert masked
        for i in masked:
            load = ops[i - 1]
            assert load[0] in ("upload", "prefetch", "stage"), (cfg, mode, seed, load)
            if cfg in ACCEPTING:
                assert load[1]["poisoned"] == ops[i][1], (cfg, mode, seed, load)
            else:
                assert "poisoned" not in load[1]
        assert sum("poisoned" in op[1] for op in ops) == (len(masked) if cfg in ACCEPTING else 0)


@pytest.mark.parametrize("mutant", ["l", "m", "n", "o", "p", "q", "r", "s"])
def test_accum_mutants_are_caught(mutant):
    caught = []
    for cfg, mode, seed in _accum_walks():
        if cfg not in ("std12", "std48"):
            continue
        try:
            _run_accum(cfg, mode, seed, mutant)
        except cs.WalkFailure as e:
            caught.append((cfg, mode, seed, str(e).splitlines()[0]))
            break
    assert caught, f"mutant {mutant} was not caught by any walk"


# ---- the ensemble profile ----------------------------------------------------------------------------------------------
class FakeEnsemble:
    """The members and the ensembles as the header describes them, on a second set of oracles (callseq.EnsModel).  A
    prefetch right behind an asynchronous epoch is staged ahead where callseq.stages_ahead holds, and every row-reading
    ensemble call is then refused naming the member; vsom_sigma_stats follows callseq.SigmaRecord until the member joins,
    which materialises a pending record and ends the deferring.  `mutant` breaks it:
      mse       an ensemble online call with first_chunk = 0 restarts member 1's running MSE
      trained   a refused call has already trained the members before the refusing one
      idle_lb   a member with epochs[k] = 0 gets its lastBMU reset
      lb        a non-first ensemble epoch or a schedule ignores a lastBMU written by vsom_set_last_bmu
      share     members with equal offsets get the first one's B
      null_mask a NULL-validity member is treated as masked, so a masked call refuses C
      begin     a former member accepts vsom_batch_accum_begin
      um        vsom_ensemble_umatrix leaves the per-member buffer unwritten: vsom_get_umatrix is stale
    and, in the four query calls of the ensemble_query profile (_query):
      q_lb          a query overwrites the covered members' lastBMU / sqres with its own search
      q_skip        a skipped member's output arrays are written
      q_skip_refuse a skipped member that has no chunk, or a chunk staged ahead, makes the call refuse
      q_ahead       a covered member with a chunk staged ahead is accepted
      q_hits        min_hits is applied to the bmuHits as they were at vsom_ensemble_create
      q_sigma       the similarity words come from the sigmaMap before the last training call
      q_k           every member gets k[0]
      q_order       in an ensemble created over another order, per-member arguments are matched by the member's index
                    in the first ensemble
      q_one_mask    one_mask[k] is read as one_mask[0]
      q_pad         a row with fewer than k candidates repeats its last candidate instead of the padding
      q_stale       a call behind a larger one returns, for its last covered member, what the larger call left
      q_b0          a member with B = 0 gets its arrays zeroed"""

    def __init__(self, cfg_name, em, mutant=None):
        self.f = cs.EnsModel(cfg_name, 0)
        for n in em.names:
            self.f.m[n].chunks = em.m[n].chunks
        self.mutant = mutant
        self.ahead = {n: False for n in em.names}
        self.last = {n: None for n in em.names}
        self.stale = {}
        self.rec = {n: cs.SigmaRecord(cs.config(n)) for n in em.names}
        self.first_order, self.hits_at_create, self.prev_sigma, self.prev_out = None, {}, {}, None

    def close(self):
        self.f.close()

    def observe(self, n):
        mod = self.f.m[n]
        st = mod.state()
        st.update(lb=mod.lb.copy(), mse=mod.mse)
        return st

    def _member(self, n, inner, a):
        f, mod = self.f, self.f.m[n]
        why = f.member_refusal(n, inner)
        if why is not None and not (self.mutant == "begin" and why[2] == "member_accum_begin"):
            return why[0], f"{inner[0]}: {why[1]}", {}
        name = inner[0]
        if name == "prefetch" and self.last[n] == "epoch_async" and cs.stages_ahead(mod.cfg):
            self.ahead[n] = True
        elif name in ("commit", "upload"):
            self.ahead[n] = False
        if name in ("commit", "upload"):
            self.stale.pop(n, None)
        if name == "set_last_bmu" and self.mutant == "lb":
            self.stale[n] = mod.lb.copy()
        self.rec[n].accepted(inner, mod.B, mod.N)
        self.last[n] = name
        out = cs.plain(f.apply_member(n, inner, a))
        return 0, "", {k: v for k, v in out.items() if v is not None}

    def call(self, op, a):
        name, p = op
        f = self.f
        if name == "m":
            return self._member(p["k"], p["op"], a)
        if name == "sigma_stats":
            return 0, "", {"stats": self.rec[p["k"]].stats()}
        if name == "ens_create":
            for n in p["order"]:
                self.rec[n].read()           # create materialises a pending record; a member never defers again
                self.rec[n].can_defer = False
        if name == "ens_create":
            self.first_order = self.first_order or list(p["order"])
            self.hits_at_create.update({n: f.m[n].som.hits.copy() for n in p["order"]})
        if name in ("ens_create", "ens_destroy"):
            f.apply(op, a)
            return 0, "", {}
        order = f.ens[p["e"]]
        if name in cs.ENSQ_CALLS:
            return self._query(op, a)
        why = f.ens_refusal(op, a)
        if why is None and self.mutant == "null_mask" and p.get("masks"):
            for k, n in enumerate(order):
                if f.m[n].cfg["custom"] or f.m[n].cfg["tr"] == po.CLR:
                    why = (k, "CLR contexts are not supported", None)
                    break
        if why is None and name not in ("ens_upload", "ens_umatrix"):
            for k, n in enumerate(order):
                if self.ahead[n] and ("sigmas" not in p or p["sigmas"][k]):
                    why = (k, "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first", None)
                    break
        if why is not None:
            if self.mutant == "trained" and why[0]:
                for n in order[:why[0]]:
                    if f.m[n].X is not None:
                        f.m[n].som.train_single(f.m[n].X[0], 0.1, 1.0, 0, 0)
            who = "" if why[0] is None else f"member {why[0]}: "
            return cs.VSOM_ERR_INVALID, f"vsom_ensemble: {who}{why[1]}", {}
        if name == "ens_upload":
            for n in order:
                self.ahead[n] = False
                self.stale.pop(n, None)
            if self.mutant == "share":
                X = dict(a["X"])
                for n in order:
                    if "share" in p["rows"][n]:
                        X[n] = X[p["rows"][n]["share"]]
                a = dict(a, X=X)
        if name in ("ens_online", "ens_online_masked") and not p["first"] and self.mutant == "mse":
            f.m[order[1]].run = np.float32(0)
        if name in ("ens_epoch", "ens_schedule", "ens_schedule_masked", "ens_epoch_masked"):
            for n in order:
                if n in self.stale:
                    f.m[n].lb[:] = self.stale.pop(n)
        before = {n: f.m[n].um for n in order}
        if name in cs.ENS_TRAIN and self.mutant == "q_sigma":
            self.prev_sigma = {n: f.m[n].som.sigma.copy() for n in order}
        out = f.apply(op, a)
        if name == "ens_umatrix" and self.mutant == "um":
            for n in order:
                f.m[n].um = np.zeros(f.m[n].N) if before[n] is None else before[n]
        if "sigmas" in p and self.mutant == "idle_lb":
            for k, n in enumerate(order):
                if not p["sigmas"][k]:
                    f.m[n].lb[:] = 0
        for n in order:
            self.last[n] = name
            self.rec[n].read()
        return 0, "", {k: v for k, v in out.items() if v is not None}

    # ---- the four query calls ----
    @staticmethod
    def _asked(name, p, key, k):
        """whether the call's struct holds a pointer for this output of member k"""
        if key in ("fill", "delta") or (key in ("dist", "count", "nvalid") and name in ("ens_topk", "ens_topk_masked")):
            return p[key][k]
        return True

    def _query(self, op, a):
        name, p = op
        f, mu = self.f, self.mutant
        order = f.ens[p["e"]]
        K = len(order)
        cov = cs.covered(op, order)
        asks = {}
        if "k" in p and p.get("bad") != "null_k":     # vsom_ensemble_topk_applies, asked before every top-k call
            asks = {"applies": {n: int(cs.topk_fast(f.m[n].cfg, f.m[n].B, p["k"][order.index(n)], name == "ens_topk_masked"))
                                for n in cov}}
        why = f.ensq_refusal(op)
        if why is None:
            ahead = "the next chunk is staged ahead over the current chunk's rows: vsom_commit_chunk first"
            for k, n in enumerate(order):
                if self.ahead[n] and ((n in cov and mu != "q_ahead") or (n not in cov and mu == "q_skip_refuse")):
                    why = (k, ahead, None)
                elif n not in cov and mu == "q_skip_refuse" and f.m[n].X is None:
                    why = (k, "no chunk loaded", None)
                if why:
                    break
        if why is not None:
            who = "" if why[0] is None else f"member {why[0]}: "
            return cs.VSOM_ERR_INVALID, f"vsom_ensemble: {who}{why[1]}", asks
        q, valid = dict(p), dict(a.get("valid", {}))
        per_member = [key for key in ("k", "min_hits", "num_sigmas") if key in p]
        if mu == "q_k" and "k" in p:
            q["k"] = [p["k"][0]] * K
        if mu == "q_order" and order != self.first_order[:K]:
            at = [self.first_order.index(n) % K for n in order]
            for key in per_member:
                q[key] = [p[key][i] for i in at]
        if mu == "q_one_mask" and name != "ens_topk":
            one0 = valid.get(order[0]) is not None and valid[order[0]].ndim == 1
            for n in cov:
                v = valid[n]
                if f.m[n].B and (v.ndim == 1) != one0:
                    if one0:
                        valid[n] = np.ascontiguousarray(v[0])
                    else:                    # (B x J bytes read from a mask of J: what lies behind it is not valid)
                        valid[n] = np.zeros((f.m[n].B, v.size), np.uint8)
                        valid[n][0] = v
        hits = self.hits_at_create if mu == "q_hits" else None
        sigma = self.prev_sigma if mu == "q_sigma" else None
        out, size, last = dict(asks), 0, None
        for n, (rows, exp) in f.query((name, q), dict(a, valid=valid), hits=hits, sigma=sigma).items():
            k, B = order.index(n), f.m[n].B
            if mu == "q_pad" and "count" in exp:
                for r, c in enumerate(exp["count"]):
                    exp["idx"][r, c:] = exp["idx"][r, c - 1]
                    exp["dist"][r, c:] = exp["dist"][r, c - 1]
            if mu == "q_lb" and "bmu" in exp:
                f.m[n].lb[rows] = exp["bmu"]
                f.m[n].sqres = np.zeros(B, np.float32) if f.m[n].sqres is None else f.m[n].sqres
                f.m[n].sqres[rows] = exp["dist"]
            for key, v in exp.items():
                if self._asked(name, p, key, k):
                    full = np.zeros((B,) + v.shape[1:], v.dtype)
                    full[rows] = v
                    out[f"{n}.{key}"] = full
                    size += full.size
            last = f"{n}.{'bmu' if 'bmu' in exp else 'idx'}"
        if mu == "q_skip":
            for n in order:
                if n not in cov and f.m[n].B:
                    out[f"{n}.idx"] = np.zeros(f.m[n].B, np.uint64)
                    break
        if mu == "q_b0":
            for n in cov:
                if f.m[n].X is not None and f.m[n].B == 0:
                    out[f"{n}.idx"] = np.zeros(1, np.uint64)
        if last is not None:
            kept = out[last].copy()
            if mu == "q_stale" and self.prev_out is not None and size < self.prev_out[0]:
                out[last] = np.resize(self.prev_out[1], out[last].shape).astype(out[last].dtype)
            self.prev_out = (size, kept)
        for n in cov:
            self.last[n] = name
            self.rec[n].read()
        return 0, "", out


ENS_SEEDS = (1, 2)   # tests/test_gpu_call_sequences.py, test_ensemble_walk_matches_oracle


def _ens_walks():
    return [(c, s) for c in cs.ENS_CONFIGS for s in ENS_SEEDS]


def _run_ens(cfg, seed, mutant=None):
    return cs.run_ensemble_walk(cs.generate_ensemble(cfg, seed), lambda name, em: FakeEnsemble(name, em, mutant))


@functools.lru_cache(maxsize=None)
def _faithful_ens(cfg, seed):
    return _run_ens(cfg, seed)


def test_ensemble_ops_stay_out_of_the_other_walks():
    assert not set(cs.ENS_MEMBERS) & set(cs.CONFIGS)
    for cfg in cs.CONFIGS:
        for seed in SEEDS:
            walks = [cs.generate(cfg, seed, scale=SCALE)]
            walks += [cs.generate(cfg, seed, scale=SCALE, profile="sigma", mode=mode) for mode in MODES]
            walks += [_accum_ops(cfg, mode, seed) for mode in MODES]
            for ops in walks:
                assert not cs.ENS_NEW_OPS & {op[0] for op in ops}


def test_ensemble_predicates_stand_at_their_borders():
    """every row count of callseq.ENS_MEMBERS is at a border of a restated path predicate"""
    M = cs.ENS_MEMBERS
    assert [cs.batch_tiny(M["A"], b) for b in (20, 160, 163, 164, 170, 257)] == [True, True, True, False, False, False]
    assert [cs.batch_tiny(M["B"], b) for b in (37, 121, 122, 151, 152)] == [True, True, False, False, False]
    assert 151 * 108 <= 16384 < 152 * 108 and 121 * 108 * 20 <= 262144 < 122 * 108 * 20
    assert [cs.batch_tiny(M["C"], b) for b in (77, 128)] == [True, False] and not cs.masked_batch_tiny(M["C"], 77)
    assert cs.batch_tiny(M["D"], 64) and not cs.batch_tiny(M["D"], 65)         # N D B = 262144 exactly
    assert cs.online_tiny(M["D"], 64, 2.5) and M["D"]["W"] * M["D"]["H"] * 512 == 4096
    assert all(cs.online_tiny(M["A"], b, 0.7) for b in (20, 160, 170, 257))
    assert not cs.online_tiny(M["A"], 20, 2.5, cs.BMU_EXACT) and not cs.online_tiny(M["A"], 20, float("nan"))
    assert not cs.online_tiny(M["C"], 77, 2.5) and not cs.online_tiny(M["F"], 64, 2.5)
    for n in ("E", "F", "G"):
        assert not any(cs.batch_tiny(M[n], b) or cs.online_tiny(M[n], b, 2.5) for b, _ in M[n]["chunks"])
    assert cs.stages_ahead(M["G"]) and cs.defers(M["G"]) and not cs.stages_ahead(M["E"])
    assert cs.masked_batch_tiny(M["A"], 20) and not cs.masked_batch_tiny(M["A"], 20, strict=False)


def test_ensemble_masks_are_engineered():
    """NaN / inf under every invalid entry and nowhere else, a column valid in no row, the row without a valid column"""
    for n in cs.ENS_MASKABLE:
        for X in cs.chunk_data(n, 1, 1, "ensemble"):
            for form in ("rows", "one_mask"):
                spec = {"seed": 77, "form": form, "full": form == "rows"}
                v = np.broadcast_to(cs.ens_mask(spec, X) != 0, X.shape)
                P = cs.ens_poisoned(spec, X)
                assert (np.isfinite(P) == v).all() and (P[v] == X[v]).all()
                assert (np.broadcast_to(cs.ens_mask(spec, P) != 0, X.shape) == v).all()
                assert (~v.any(axis=0)).sum() >= 1
                if form == "rows":
                    assert (~v.any(axis=1)).sum() == 1
    X = cs.chunk_data("E", 1, 1, "ensemble")[2]
    assert X.shape[0] == 1100 and not X[:, 5].any() and X[:, 4].any()
    a, a2 = cs.chunk_data("A", 1, 1, "ensemble"), cs.chunk_data("A2", 1, 1, "ensemble")
    assert all((x == y).all() for x, y in zip(a, a2))


def _ens_runs(ops):
    """the ops between each run's markers (runs 8 and 9, which open the walk, overlap)"""
    runs, inside = {}, []
    for op in ops[1:]:
        if op[0] == "run":
            inside.append(op[1]["id"])
        elif op[0] == "run_end":
            inside.remove(op[1]["id"])
        for run in inside:
            if op[0] != "run":
                runs.setdefault(run, []).append(op)
    return runs


def test_ensemble_walks_hold_the_required_runs():
    for cfg, seed in _ens_walks():
        own = cfg == "ens_own"
        ops = cs.generate_ensemble(cfg, seed)
        assert ast.literal_eval(repr(ops)) == ops        # a printed walk can be replayed
        runs = _ens_runs(ops)
        assert set(runs) == set(cs.ENS_RUNS) - (set() if own else {8}), (cfg, seed, sorted(runs))
        names = {r: [o[1]["op"][0] if o[0] == "m" else o[0] for o in runs[r]] for r in runs}
        # 1: nothing but ensemble calls; two wait = 0 uploads, the second larger, each followed by a train call
        assert names[1] == ["ens_upload", "ens_epoch_masked", "ens_bmu"] + ([] if own else ["ens_umatrix"]) + \
            ["ens_schedule_masked", "ens_online_masked", "ens_upload", "ens_epoch"], names[1]
        ups = [o[1] for o in runs[1] if o[0] == "ens_upload"]
        assert all(u["wait"] == 0 for u in ups) and ups[0]["poison"] and "poison" not in ups[1]
        assert any(s.get("full") for s in ups[0]["poison"].values())
        size = lambda u: sum(cs.ENS_MEMBERS[n]["chunks"][s["chunk"]][0] * cs.ENS_MEMBERS[n]["J"] for n, s in u["rows"].items())
        assert size(ups[1]) > size(ups[0])
        assert any(v is None for v in [runs[1][1][1]["masks"].get(n) for n in ups[0]["rows"]])       # NULL-validity members
        # 2: first_chunk = 1, own uploads, a single online chunk with first = 0, the masked call with first_chunk = 0
        assert names[2][:5] == ["ens_online", "upload", "upload", "online", "ens_online_masked"], names[2]
        assert runs[2][0][1]["first"] and not runs[2][3][1]["op"][1]["first"] and not runs[2][4][1]["first"]
        # 3: A at 160, 170, 160 rows and B at 121, 122, 121 / 151, 152, 121 in front of each kind of call; EXACT and AUTO; a
        # NaN; epochs 0
        sizes = [(cs.ENS_MEMBERS["A"]["chunks"][o[1]["rows"]["A"]["chunk"]][0],
                  cs.ENS_MEMBERS["B"]["chunks"][o[1]["rows"]["B"]["chunk"]][0]) for o in runs[3] if o[0] == "ens_upload"]
        assert sizes == [(160, 121), (170, 122), (160, 121), (160, 151), (170, 152), (160, 121)], sizes
        for kind in cs.ENS_TRAIN:
            assert names[3].count(kind) >= 2, (kind, names[3])
        modes = [o[1]["op"][1]["mode"] for o in runs[3] if o[0] == "m" and o[1]["op"][0] == "bmu_mode"]
        assert modes == [cs.BMU_EXACT, cs.BMU_AUTO]
        sched = [o[1]["sigmas"] for o in runs[3] if o[0] in ("ens_schedule", "ens_schedule_masked")]
        assert any(None in s for sg in sched for s in sg) and any(s == [] for sg in sched for s in sg)
        # 4: the stage-ahead
        k = "G" if own else "E"
        assert names[4][:3] == ["upload", "epoch_async", "prefetch"] and runs[4][1][1]["k"] == k
        refused = [o for o in runs[4] if "must_refuse" in o[1]]
        assert [o[0] for o in refused] == (list(cs.ENS_TRAIN) + ["ens_bmu"] if own else [])
        rest = names[4][names[4].index("ens_upload"):]
        assert rest == ["ens_upload", "commit", "ens_epoch", "ens_bmu"], rest
        # 6: state rewritten between ensemble calls
        assert names[6] == ["set_state", "set_state", "set_last_bmu", "set_last_bmu", "ens_epoch", "set_last_bmu",
                            "ens_schedule_masked", "get_last_bmu"], names[6]
        assert not runs[6][4][1]["first"] and not runs[6][6][1]["reset"]
        # 7: lifetime
        assert names[7][0] == "ens_destroy" and names[7].count("ens_create") == 2 and "ens_umatrix" in names[7]
        created = [o[1]["order"] for o in runs[7] if o[0] == "ens_create"]
        assert "F" not in created[0] and set(created[1]) & set(created[0])
        es = [o[1]["e"] for o in runs[7] if o[0] in cs.ENS_CALLS]
        assert any(x != y for x, y in zip(es, es[1:]))
        # 8, 9: before the first create
        first = [o[0] for o in ops].index("ens_create")
        if own:
            assert ops[first - 1] != ops[first] and ("sigma_stats", {"k": "G", "expect": [1, 0, 0, 1]}) in ops[:first]
            assert ops[first + 1] == ("sigma_stats", {"k": "G", "expect": [1, 0, 1, 0]})
        # (the first ensemble epoch is the one refused for C, which has no chunk yet)
        assert [n for n in names[9] if n in ("accum_begin", "accum_chunk", "ens_create", "ens_epoch", "accum_end")] == \
            ["accum_begin", "accum_chunk", "ens_create", "ens_epoch", "ens_epoch", "accum_chunk", "accum_end"], names[9]


@pytest.mark.parametrize("cfg,seed", _ens_walks())
def test_faithful_fake_passes_ensemble_walks(cfg, seed):
    """... and the walks the GPU test runs meet the conditions it asserts (callseq.ens_conditions)"""
    cs.ens_conditions(cfg, _faithful_ens(cfg, seed))


# sha256(repr(generate_ensemble(cfg, seed)))
ENS_DIGESTS = {
    ("ens_shared", 1): "e7e68cd3eb80eb062226cdfa914adac94f070ec2c05f7126dff782a4ad386aef",
    ("ens_shared", 2): "0e4207a8364dea50c2ff26f2fe5e50ff826ec982a2819a158f471bf21c40c9e4",
    ("ens_own", 1): "2f4dacc5fbdd06a73f159177002cedc9635d4bdec383617c585338133cc3aba8",
    ("ens_own", 2): "06ea491e869f80c28c0331a1f68f3d9a1fb386533084403a3f32067c856d702b",
}


@pytest.mark.parametrize("key", [(c, s) for c in cs.ENS_CONFIGS for s in ENS_SEEDS], ids=lambda k: "-".join(str(v) for v in k))
def test_ensemble_walks_are_unchanged(key):
    ops = cs.generate_ensemble(*key)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == ENS_DIGESTS[key]


@pytest.mark.parametrize("mutant", ["mse", "trained", "idle_lb", "lb", "share", "null_mask", "begin", "um"])
def test_ensemble_mutants_are_caught(mutant):
    caught = []
    for cfg, seed in _ens_walks():
        try:
            _run_ens(cfg, seed, mutant)
        except cs.WalkFailure as e:
            text = str(e)
            assert f"seed {seed}" in text and "replay(ops) with ops = [('config'" in text
            # the first differing element, or the return code where it is the call's acceptance that differs
            assert "element" in text or "returned" in text or "failed: -1" in text, text.splitlines()[0]
            caught.append((cfg, seed, text.splitlines()[0]))
            break
    assert caught, f"mutant {mutant} was not caught by any walk"


# ---- the ensemble_query profile ------------------------------------------------------------------------------------------
def _ensq_walks():
    return [(c, s) for c in cs.ENSQ_CONFIGS for s in ENS_SEEDS]     # tests/test_gpu_call_sequences.py runs these four


def _run_ensq(cfg, seed, mutant=None):
    return cs.run_ensemble_walk(cs.generate_ensemble_query(cfg, seed), lambda name, em: FakeEnsemble(name, em, mutant))


@functools.lru_cache(maxsize=None)
def _faithful_ensq(cfg, seed):
    return _run_ensq(cfg, seed)


@pytest.mark.parametrize("cfg,seed", _ensq_walks())
def test_faithful_fake_passes_ensemble_query_walks(cfg, seed):
    """... and the walks the GPU test runs meet the conditions it asserts (callseq.ensq_conditions)"""
    cs.ensq_conditions(cfg, _faithful_ensq(cfg, seed))


# sha256(repr(generate_ensemble_query(cfg, seed)))
ENSQ_DIGESTS = {
    ("ensq_shared", 1): "8d9fad2f87c2c7438270b8703d4d5154e5d6b66151b72a644601f82bbf86bf20",
    ("ensq_shared", 2): "f438b6bf52400ecb69bc6a952b9d70110b4aab61dd648448226c5994abfe3fdc",
    ("ensq_own", 1): "4fee7816e3a8733451844a919754cbb0b1af925390cf54169aa1acfc36cb7dde",
    ("ensq_own", 2): "79e70bf208deea422cf5a3c27456ce547ce38737924afd73087c76a8b2073975",
}


@pytest.mark.parametrize("key", _ensq_walks(), ids=lambda k: "-".join(str(v) for v in k))
def test_ensemble_query_walks_are_unchanged(key):
    ops = cs.generate_ensemble_query(*key)
    assert hashlib.sha256(repr(ops).encode()).hexdigest() == ENSQ_DIGESTS[key]


def test_ensemble_query_ops_stay_out_of_the_other_walks():
    assert not (set(cs.ENSQ_MEMBERS) & (set(cs.CONFIGS) | set(cs.ENS_MEMBERS))) and not set(cs.ENSQ_CONFIGS) & set(cs.ENS_CONFIGS)
    assert not set(cs.ENSQ_CALLS) & set(cs.ENS_CALLS) and not cs.ENSQ_NEW_OPS & cs.ENS_NEW_OPS
    walks = [cs.generate_ensemble(cfg, seed) for cfg, seed in _ens_walks()]
    for cfg in cs.CONFIGS:
        for seed in SEEDS:
            walks.append(cs.generate(cfg, seed, scale=SCALE))
            walks += [cs.generate(cfg, seed, scale=SCALE, profile="sigma", mode=mode) for mode in MODES]
            walks += [_accum_ops(cfg, mode, seed) for mode in MODES]
    for ops in walks:
        names = {op[0] for op in ops} | {op[1]["op"][0] for op in ops if op[0] == "m"}
        assert not (cs.ENSQ_NEW_OPS - set(cs.MASKED_SCORES)) & names
        assert not {op[1]["k"] for op in ops if op[0] == "m"} & set(cs.ENSQ_MEMBERS)
    # (similarity_masked is the accum profile's too: there it is a row-window query of one context)
    for cfg, seed in _ens_walks():
        assert "similarity_masked" not in {op[1]["op"][0] for op in cs.generate_ensemble(cfg, seed) if op[0] == "m"}


def test_ensemble_query_predicates_stand_at_their_borders():
    """callseq.masked_query_fast / topk_fast at N * D = 4096 and beyond, at k = 0, 1, min(64, N) and above, for CLR, custom
    and empty chunks; the LDS terms the header names never bind for a member of these walks"""
    M = dict(cs.ENS_MEMBERS, **cs.ENSQ_MEMBERS)
    N = lambda n: M[n]["W"] * M[n]["H"]
    assert N("D") * 512 == 4096 and N("D2") * 513 == 4104
    assert cs.masked_query_fast(M["D"], 3) and not cs.masked_query_fast(M["D2"], 3)
    assert not cs.masked_query_fast(M["D"], 0) and cs.masked_query_fast(M["Q"], 1) and cs.masked_query_fast(M["B"], 152)
    assert not cs.masked_query_fast(M["C"], 77) and not cs.masked_query_fast(M["F"], 64)
    assert not any(cs.masked_query_fast(M[n], 77) for n in ("E", "G"))
    for masked in (False, True):
        assert [cs.topk_fast(M["D"], 3, k, masked) for k in (0, 1, 8, 9)] == [False, True, True, False]
        assert not any(cs.topk_fast(M["D2"], 3, k, masked) for k in (1, 8))
        assert [cs.topk_fast(M["Q"], 1, k, masked) for k in (0, 1, 64, 65)] == [False, True, True, False]
        assert not cs.topk_fast(M["Q"], 0, 2, masked) and not cs.topk_fast(M["F"], 64, 2, masked)
        assert not any(cs.topk_fast(M[n], 77, 2, masked) for n in ("E", "G"))
    assert cs.topk_fast(M["C"], 77, 64, False) and not cs.topk_fast(M["C"], 77, 64, True)
    assert N("C") * (cs.po.length(cs.po.CLR, 6) // 2) <= 4096
    # the LDS terms: within 64 KiB wherever N * part_len <= 4096 lets a member of these walks onto the fast path
    for n, cfg in M.items():
        D = cs.po.length(cfg["tr"], cfg["J"])
        part = D // 2 if cfg["tr"] == cs.po.CLR else D
        if N(n) * part <= 4096:
            assert 512 + 512 * (min(64, N(n)) | 1) + 4 * N(n) * D <= 65536, n
            assert cfg["tr"] == cs.po.CLR or 768 + 4 * N(n) * D <= 65536, n
    # every row count of Q is at a border of the 64-row tile
    assert [b for b, _ in M["Q"]["chunks"]] == [1, 63, 64, 65, 128, 129]
    assert [x.shape[0] for x in cs.chunk_data("Q", 1, 1, "ensemble")] == [1, 63, 64, 65, 128, 129]
    assert [x.shape for x in cs.chunk_data("D2", 1, 1, "ensemble")] == [(3, 513), (64, 513)]


def test_ensemble_query_walks_hold_the_required_runs():
    for cfg, seed in _ensq_walks():
        own = cfg == "ensq_own"
        S = "G" if own else "E"
        ops = cs.generate_ensemble_query(cfg, seed)
        assert ast.literal_eval(repr(ops)) == ops        # a printed walk can be replayed
        runs = _ens_runs(ops)
        assert set(runs) == set(cs.ENSQ_RUNS) - (set() if own else {8}), (cfg, seed, sorted(runs))
        names = {r: [o[1]["op"][0] if o[0] == "m" else o[0] for o in runs[r]] for r in runs}
        members = cs.ENSQ_CONFIGS[cfg]["members"]
        cov = lambda o: cs.covered(o, members)
        # 1: two wait = 0 uploads, training tables and query images in turn, every query covers the slow member and skips one
        assert names[1] == ["ens_upload", "ens_epoch_masked", "ens_bmu_masked", "ens_schedule_masked", "ens_topk_masked",
                            "ens_online_masked", "ens_similarity_masked", "ens_upload", "ens_topk", "ens_epoch"], names[1]
        ups = [o[1] for o in runs[1] if o[0] == "ens_upload"]
        assert all(u["wait"] == 0 for u in ups) and ups[0]["poison"] and "poison" not in ups[1]
        size = lambda u: sum(cs.config(n)["chunks"][s["chunk"]][0] * cs.config(n)["J"] for n, s in u["rows"].items())
        assert size(ups[1]) > size(ups[0])
        for o in runs[1]:
            if o[0] in cs.ENSQ_CALLS:
                assert S in cov(o) and len(cov(o)) < len(members), o
        assert all(runs[1][2][1]["fill"]) and all(runs[1][6][1]["delta"])
        # 2: the layouts in the issue's order
        assert names[2] == ["ens_upload", "ens_similarity_masked", "ens_topk", "ens_bmu_masked", "ens_topk", "ens_topk_masked",
                            "ens_bmu_masked"], names[2]
        r2 = [o[1] for o in runs[2]]
        assert all(r2[1]["delta"]) and set(cs.ENSQ_MASKABLE) & set(members) <= set(r2[1]["masks"])
        assert max(r2[2]["k"]) == 64 and set(r2[4]["k"]) == {1} and len(r2[3]["masks"]) == 2 and not any(r2[3]["fill"])
        c5 = cov(runs[2][5])
        for key in ("dist", "count", "nvalid"):
            flags = [v for n, v in zip(members, r2[5][key]) if n in c5]
            assert not all(flags) and any(flags), (key, flags)
        assert len({k for n, k in zip(members, r2[5]["k"]) if n in c5}) >= 3
        assert sum(v for n, v in zip(members, r2[6]["fill"]) if n in cov(runs[2][6])) == 1
        # 3: lastBMU written, the four queries, the observers, a non-first epoch; hits rewritten; queries, training, queries
        assert names[3][:7] == ["ens_upload", "set_last_bmu", "set_last_bmu"] + list(cs.ENSQ_CALLS), names[3]
        at = names[3].index("ens_epoch")
        assert set(names[3][7:at]) == {"get_last_bmu", "get_sqres", "get_mse"} and not runs[3][at][1]["first"]
        assert names[3][at + 1:] == ["set_state", "set_state", "ens_bmu_masked", "ens_similarity_masked", "ens_topk_masked",
                                     "ens_online", "ens_bmu_masked", "ens_similarity_masked", "ens_topk_masked"]
        assert runs[3][at + 1][1]["op"][1]["parts"] == "hits0" and runs[3][at + 1][1]["k"] == "B"
        assert max(runs[3][at + 3][1]["min_hits"]) == 1 and max(runs[3][at + 4][1]["min_hits"]) == 2
        # 4: Q's row counts, D and D2 in the same calls
        rows = [cs.config("Q")["chunks"][o[1]["rows"]["Q"]["chunk"]][0] for o in runs[4] if o[0] == "ens_upload"]
        assert rows == [63, 64, 65, 129, 1], rows
        assert all({"D", "D2", "Q"} <= set(cov(o)) for o in runs[4] if o[0] in cs.ENSQ_CALLS and "labels" not in o[1])
        modes = [o[1]["op"][1]["mode"] for o in runs[4] if o[0] == "m" and o[1]["op"][0] in ("bmu_mode", "update_mode")]
        assert modes == [cs.BMU_EXACT, cs.UPDATE_FMA, cs.UPDATE_STRICT, cs.BMU_AUTO]
        if not own:
            assert any(None in s for o in runs[4] if o[0] == "ens_schedule" for s in o[1]["sigmas"])
        # 5: covered (refused where staged ahead), skipped, committed
        assert names[5] == ["upload", "epoch_async", "prefetch"] + list(cs.ENSQ_CALLS) * 2 + ["commit"] + list(cs.ENSQ_CALLS)
        five = [o for o in runs[5] if o[0] in cs.ENSQ_CALLS]
        assert [("must_refuse" in o[1], S in cov(o)) for o in five] == [(own, True)] * 4 + [(False, False)] * 4 + [(False, True)] * 4
        # 6: the refusals, in the generator's order
        bad = [(o[0], o[1].get("bad")) for o in runs[6] if o[0] in cs.ENSQ_CALLS and o[1].get("bad")]
        assert bad == [(c, "null_valid") for c in cs.ENSQ_MASKED] + [(c, "null_out") for c in cs.ENSQ_CALLS] + \
            [("ens_topk", "null_k"), ("ens_topk_masked", "null_k"), ("ens_similarity_masked", "null_num_sigmas"),
             ("ens_similarity_masked", "bad_rule"), ("ens_topk_masked", "null_idx")], bad
        ks = [o[1]["k"][0] for o in runs[6] if "k" in o[1] and o[1]["k"][0] in (0, 65)]
        assert ks == [0, 65, 0, 65] and sum(9 in o[1].get("k", ()) for o in runs[6]) == 4
        assert sum("C" in cov(o) for o in runs[6] if o[0] in cs.ENSQ_CALLS) == 5
        assert sum("F" in cov(o) for o in runs[6] if o[0] in cs.ENSQ_CALLS) == (4 if own else 0)
        # 7: lifetime
        assert names[7][0] == "ens_destroy" and names[7].count("ens_create") == 2 and names[7].count("ens_destroy") == 3 and names[7][-1] == "ens_destroy"
        created = [o[1]["order"] for o in runs[7] if o[0] == "ens_create"]
        assert set(created[1]) <= set(created[0]) and created[1] != [n for n in created[0] if n in created[1]]
        es = [o[1]["e"] for o in runs[7] if o[0] in cs.ENSQ_CALLS]
        assert sum(x != y for x, y in zip(es, es[1:])) >= 7
        assert any("head" in s for o in runs[7] if o[0] == "ens_upload" for s in o[1]["rows"].values())
        singles = {o[1]["op"][0] for o in runs[7] if o[0] == "m"}
        assert singles & (cs.ENSQ_NEW_OPS | {"topk"})
        if own:
            first = [o[0] for o in ops].index("ens_create")
            assert ("sigma_stats", {"k": "G", "expect": [1, 0, 0, 1]}) in ops[:first]
            assert [n for n in names[8] if n.startswith("ens_")][-2:] == ["ens_epoch", "ens_similarity_masked"]
            assert "G" in cov(runs[8][-2])


QUERY_MUTANTS = ["q_lb", "q_skip", "q_skip_refuse", "q_ahead", "q_hits", "q_sigma", "q_k", "q_order", "q_one_mask", "q_pad",
                 "q_stale", "q_b0"]


@pytest.mark.parametrize("mutant", QUERY_MUTANTS)
def test_ensemble_query_mutants_are_caught(mutant):
    caught = []
    for cfg, seed in [("ensq_own", 1), ("ensq_own", 2), ("ensq_shared", 1), ("ensq_shared", 2)]:
        try:
            _run_ensq(cfg, seed, mutant)
        except cs.WalkFailure as e:
            text = str(e)
            assert f"seed {seed}" in text and "replay(ops) with ops = [('config'" in text
            # the first differing element, or the return code where it is the call's acceptance that differs
            assert "element" in text or "returned" in text or "failed: -1" in text, text.splitlines()[0]
            caught.append((cfg, seed, text.splitlines()[0]))
            break
    assert caught, f"mutant {mutant} was not caught by any walk"
