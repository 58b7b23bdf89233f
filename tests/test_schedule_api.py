"""CPU tier of the resident batch schedule (vsom_batch_schedule, vsom_ensemble_batch_schedule):
the contract restated on the oracle (tests/schedule_ref.py) is trainBatchSom on a one-chunk data set, the sigma helper
stops where trainBatchSom returns, the two symbols are declared and listed, and the Python mirrors refuse bad shapes and
multi-chunk data sets before any device call (stub contexts: no GPU here)."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen  # noqa: E402
import schedule_ref as sref  # noqa: E402
from schedule_ref import beq  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsom_batch_schedule", "vsom_ensemble_batch_schedule")


def fixture_rows():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    return np.array(fx["rows"], np.float32)


def median_case():
    z = np.load(os.path.join(ROOT, "tests", "golden", "q10_nonsquare_5x11_median_batch.npz"))
    return z["X"].astype(np.float32), z["init_map"].astype(np.float32)


CASES = {
    # the reference's perf scenario: 33 of 40 epochs run before sigma < 1
    "fixture": lambda: (10, 10, 9, po.STANDARD, fixture_rows(), gen.random_map(100, 9, 42), 40, 5.0, 0.05, 33),
    # SomIndex divides by HEIGHT (Q10): W != H, Median
    "median_5x11": lambda: (5, 11, 10, po.MEDIAN, *median_case(), 12, 3.0, 0.15, 8),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_loop_is_train_batch_on_one_chunk(name):
    W, H, J, tr, X, init, epochs, sigma0, decay, ran = CASES[name]()
    sigmas = vs.batch_sigma_schedule(epochs, sigma0, decay)
    assert len(sigmas) == ran
    a, b = po.OracleSom(W, H, J, tr), po.OracleSom(W, H, J, tr)
    a.set_state(map=init)
    b.set_state(map=init)
    mse, lb = sref.oracle_loop(a, X, sigmas, reset_bmu=True)
    done, mse_ref = b.train_batch(X, [0, X.shape[0]], epochs, sigma0, decay)
    assert done == ran
    assert beq(mse, mse_ref[:ran]) and np.isnan(mse_ref[ran:]).all()
    for k in ("map", "sigma", "S", "weight", "hits"):
        assert beq(getattr(a, k), getattr(b, k)), k
    assert (lb < W * H).all() and a.hits.sum() == ran * X.shape[0]


def test_carried_bmus_differ_from_the_reset_walk_somewhere():
    """reset_bmu is not a no-op of the restated contract: on the fixture the walk from the previous BMU and the walk from
    unit 0 end in different units for some row of some epoch (else the GPU tests of reset_bmu = 0 would show nothing)"""
    W, H, J, tr, X, init, epochs, sigma0, decay, ran = CASES["fixture"]()
    sigmas = vs.batch_sigma_schedule(epochs, sigma0, decay)
    a, b = po.OracleSom(W, H, J, tr), po.OracleSom(W, H, J, tr)
    a.set_state(map=init)
    b.set_state(map=init)
    mse_a, lb_a = sref.oracle_loop(a, X, sigmas, reset_bmu=True)
    mse_b, lb_b = sref.oracle_loop(b, X, sigmas, reset_bmu=False)
    assert not (beq(mse_a, mse_b) and beq(lb_a, lb_b) and beq(a.map, b.map))


@pytest.mark.parametrize("epochs,sigma0,decay", [(40, 5.0, 0.05), (200, 5.0, 0.005), (5, 1.0, 0.0), (5, 1.0, 0.1),
                                                 (7, 3.0, 0.0), (4, 0.99, 0.0), (0, 5.0, 0.1), (6, 2.0, 0.5)])
def test_sigma_schedule_stops_where_train_batch_returns(epochs, sigma0, decay):
    sig = vs.batch_sigma_schedule(epochs, sigma0, decay)
    o = po.OracleSom(3, 3, 2)
    o.set_state(map=gen.random_map(9, 2, 1))
    X = gen.blobs(4, 2, 2, 1, 2)
    done, _ = o.train_batch(X, [0, 4], epochs, sigma0, decay)
    assert len(sig) == done
    assert all(s >= 1.0 for s in sig)
    assert sig == [sigma0 * math.exp(-decay * float(i)) for i in range(len(sig))]     # _trainBatchSom's formula


def test_sigma_schedule_edges():
    assert vs.batch_sigma_schedule(5, 1.0, 0.0) == [1.0] * 5          # decay 0 runs every epoch; sigma = 1.0 trains
    assert vs.batch_sigma_schedule(5, 1.0, 0.1) == [1.0]              # ... and the first sigma < 1 ends the schedule
    assert vs.batch_sigma_schedule(3, 0.5, 0.0) == []
    assert len(vs.batch_sigma_schedule(40, 5.0, 0.05)) == 33
    assert len(vs.batch_sigma_schedule(200, 5.0, 0.005)) == 200


def test_new_symbols_declared_and_listed():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vsom_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
    m = re.search(r"#define\s+VSOM_SCHEDULE_MAX_EPOCHS\s+(\d+)", txt)
    assert m and int(m.group(1)) == capi.SCHEDULE_MAX_EPOCHS


# ---- the mirrors refuse before any device call ------------------------------------------------------------------
class StubCtx:
    """records the calls a mirror makes; batch_schedule answers one MSE per sigma"""

    def __init__(self, B=0):
        self.calls = []
        self.B = B

    def upload_chunk(self, X):
        self.calls.append("upload_chunk")
        self.B = X.shape[0]

    def batch_schedule(self, sigmas, reset_bmu=True):
        self.calls.append(("batch_schedule", list(sigmas), reset_bmu))
        return np.arange(1, len(sigmas) + 1, dtype=np.float32) / np.float32(8)

    def get_last_bmu(self):
        self.calls.append("get_last_bmu")
        return np.arange(self.B, dtype=np.uint64)


def stub_som(ctx):
    s = vs.Som.__new__(vs.Som)
    s.ctx = ctx
    s._verbose = False
    return s


def test_context_schedule_shape_errors_raise_before_the_call():
    ctx = capi.Context.__new__(capi.Context)
    ctx._h = None                                   # (a call into the library would fail on it)
    with pytest.raises(ValueError, match="1-D"):
        ctx.batch_schedule([[3.0, 2.0], [2.0, 1.5]])
    with pytest.raises(ValueError, match="1-D"):
        ctx.batch_schedule(3.0)
    ens = capi.Ensemble.__new__(capi.Ensemble)
    ens.members, ens._h, ens._pinned = [ctx, ctx], None, None
    with pytest.raises(ValueError, match="3 schedules for 2 members"):
        ens.batch_schedule([[3.0], [2.0], [1.5]])
    with pytest.raises(ValueError, match="1-D"):
        ens.batch_schedule([[[3.0]], [[2.0]]])


def test_resident_training_refuses_a_multi_chunk_data_set():
    X = gen.blobs(20, 4, 3, 1, 2)
    ctx = StubCtx()
    som = stub_som(ctx)
    data = vs.ArrayDataSet(X, maxLoadCount=12)
    with pytest.raises(ValueError, match="one chunk"):
        som.trainBatchSomResident(data, 5, 3.0, 0.1)
    assert ctx.calls == []                          # nothing was uploaded or trained
    assert som.metrics.MeanSquaredError == [0.0] * 5


def test_resident_training_writes_metrics_bmus_and_resets_the_stream():
    X = gen.blobs(20, 4, 3, 1, 2)
    ctx = StubCtx()
    som = stub_som(ctx)
    data = vs.ArrayDataSet(X)
    som.trainBatchSomResident(data, 6, 2.0, 0.3)
    sig = vs.batch_sigma_schedule(6, 2.0, 0.3)
    assert len(sig) == 3
    assert ctx.calls == ["upload_chunk", ("batch_schedule", sig, True), "get_last_bmu"]
    assert som.metrics.MeanSquaredError[:3] == [np.float32(k / 8) for k in (1, 2, 3)]
    assert som.metrics.MeanSquaredError[3:] == [0.0] * 3
    assert (data.lastBMU == np.arange(20, dtype=np.uint64)).all()
    assert not data.hasReadWholeDataStream() and data.isAtStartOfDataStream()
    # an empty schedule loads nothing (trainBatchSom returns at its first sigma)
    ctx2 = StubCtx()
    som2 = stub_som(ctx2)
    data2 = vs.ArrayDataSet(X)
    som2.trainBatchSomResident(data2, 4, 0.9, 0.1)
    assert ctx2.calls == [] and data2.size() == 0 and som2.metrics.MeanSquaredError == [0.0] * 4
