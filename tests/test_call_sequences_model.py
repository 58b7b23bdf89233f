"""CPU self-test of the call-sequence walk (tests/callseq.py): the same walks as tests/test_gpu_call_sequences.py, run
against fake contexts backed by a second oracle.  The faithful fake must pass; each mutant -- a fake with one of the
ingest bugs the walk exists to find -- must be caught by at least one seed.  This shows, without a GPU, that the walk
can see that class of bug."""
import numpy as np
import pytest

import callseq as cs

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
      d  a refused call has already changed the model"""

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

    def close(self):
        self.m.close()

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

    def call(self, op, a):
        name, p = op
        late = self._flush(name)
        m = self.m
        if self.cfg["custom"] and name in cs.CUSTOM_REFUSED:
            return cs.VSOM_ERR_INVALID, "not for a custom context", {}
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
            out = m.apply(op, a)
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
        st = self.m.state()
        st.update(lb=self.m.lb.copy(), mse=self.m.mse)
        return st


def _walks():
    return [(c, s) for c in cs.CONFIGS for s in SEEDS]


def _run(cfg, seed, mutant=None):
    ops = cs.generate(cfg, seed, scale=SCALE)
    return cs.run_walk(ops, lambda name, model: FakeBackend(name, model, mutant))


@pytest.mark.parametrize("cfg,seed", _walks())
def test_faithful_fake_passes(cfg, seed):
    stats = _run(cfg, seed)
    assert stats["ops"] >= 30


def test_walks_hold_the_required_runs():
    """each walk contains the three runs without a synchronising call inside (callseq.generate)"""
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
