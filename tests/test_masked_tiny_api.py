"""CPU tier of the masked one-launch schedules and ensembles (vsom_batch_schedule_masked, vsom_ensemble_batch_epoch_masked,
vsom_ensemble_batch_schedule_masked, vsom_masked_tiny_applies): the symbols are declared, listed and
exported, the Python wrappers refuse wrong shapes of `valid` before any call into the library, and
trainBatchSomResidentMasked refuses a multi-chunk data set before it trains (stub contexts: no GPU here)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from vsom_amd import capi
from vsom_amd import som as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsom_batch_schedule_masked", "vsom_ensemble_batch_epoch_masked", "vsom_ensemble_batch_schedule_masked",
       "vsom_masked_tiny_applies")


def test_new_symbols_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(vsom_[a-z0-9_]+)\s*\(", txt))
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(L, name), name
    for name in ("batch_schedule_masked", "masked_tiny_applies"):
        assert hasattr(capi.Context, name), name
    for name in ("batch_epoch_masked", "batch_schedule_masked"):
        assert hasattr(capi.Ensemble, name), name
    assert hasattr(vs.Som, "trainBatchSomResidentMasked")


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len

    def close(self):
        pass


BAD = (np.ones(4), np.ones((7, 4)), np.ones((6, 5)), np.ones((7, 5, 1)), np.ones(()))


def test_context_shape_checks_raise_before_the_call():
    ctx = NoDevice(5)
    for bad in BAD:
        with pytest.raises(ValueError, match="valid has shape"):
            ctx.batch_schedule_masked([3.0, 2.0], bad)
    with pytest.raises(ValueError, match="1-D"):
        ctx.batch_schedule_masked([[3.0, 2.0]], np.ones((7, 5)))
    with pytest.raises(ValueError, match="1-D"):
        ctx.batch_schedule_masked(3.0, np.ones(5))


def test_ensemble_shape_checks_raise_before_the_call():
    a, b = NoDevice(5), NoDevice(3)
    ens = capi.Ensemble.__new__(capi.Ensemble)
    ens.members, ens._h, ens._pinned = [a, b], None, None
    good = [np.ones((7, 5)), None]
    for call in (lambda v: ens.batch_epoch_masked(2.0, True, v), lambda v: ens.batch_schedule_masked([3.0, 2.0], v)):
        for bad in BAD:
            with pytest.raises(ValueError, match="valid has shape"):
                call([bad, None])
        with pytest.raises(ValueError, match="valid has shape"):
            call([np.ones((7, 5)), np.ones(5)])          # member 1 has 3 columns
        for wrong in ([np.ones((7, 5))], [None, None, None], np.ones((2, 7, 5)), None):
            with pytest.raises(ValueError, match="one entry per member"):
                call(wrong)
    with pytest.raises(ValueError, match="3 schedules for 2 members"):
        ens.batch_schedule_masked([[3.0], [2.0], [1.5]], good)
    with pytest.raises(ValueError, match="1-D"):
        ens.batch_schedule_masked([[[3.0]], [[2.0]]], good)
    with pytest.raises(ValueError, match="2 values for 2 members|3 values for 2 members"):
        ens.batch_epoch_masked([1.0, 2.0, 3.0], True, good)


# ---- the Som mirror ------------------------------------------------------------------------------------------------------
class StubCtx:
    """records the calls a mirror makes; batch_schedule_masked answers one MSE per sigma"""

    def __init__(self, in_len):
        self.calls = []
        self.in_len = in_len
        self.B = 0

    def upload_chunk(self, X):
        self.calls.append("upload_chunk")
        self.B = X.shape[0]

    def batch_schedule_masked(self, sigmas, valid, reset_bmu=True):
        self.calls.append(("batch_schedule_masked", list(sigmas), np.array(valid), reset_bmu))
        return np.arange(1, len(sigmas) + 1, dtype=np.float32) / np.float32(8)

    def get_last_bmu(self):
        self.calls.append("get_last_bmu")
        return np.arange(self.B, dtype=np.uint64)


class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet whose loaded rows carry validity flags"""

    def __init__(self, X, validity, maxLoadCount=None):
        super().__init__(X, maxLoadCount)
        self._validity = validity
        self.validity = validity[0:0]

    def loadNextDataFromStream(self):
        start = self._pos
        super().loadNextDataFromStream()
        self.validity = self._validity[start:start + self.data.shape[0]]


def stub_som(ctx):
    s = vs.Som.__new__(vs.Som)
    s.ctx = ctx
    s._verbose = False
    return s


def test_resident_masked_training_refuses_a_multi_chunk_data_set():
    X = gen.blobs(20, 4, 3, 1, 2)
    ctx = StubCtx(4)
    som = stub_som(ctx)
    data = ValidDataSet(X, np.ones((20, 4), np.uint8), 12)
    with pytest.raises(ValueError, match="one chunk"):
        som.trainBatchSomResidentMasked(data, 5, 3.0, 0.1)
    assert ctx.calls == []                          # nothing was uploaded or trained
    assert som.metrics.MeanSquaredError == [0.0] * 5


def test_resident_masked_training_passes_the_validity_and_writes_metrics():
    X = gen.blobs(20, 4, 3, 1, 2)
    valid = np.random.default_rng(1).random((20, 4)) < 0.7
    ctx = StubCtx(4)
    som = stub_som(ctx)
    data = ValidDataSet(X, valid)
    som.trainBatchSomResidentMasked(data, 6, 2.0, 0.3)
    sig = vs.batch_sigma_schedule(6, 2.0, 0.3)
    assert len(sig) == 3
    assert ctx.calls[0] == "upload_chunk" and ctx.calls[2] == "get_last_bmu" and len(ctx.calls) == 3
    name, sg, v, reset = ctx.calls[1]
    assert name == "batch_schedule_masked" and sg == sig and reset is True and (v == valid).all()
    assert som.metrics.MeanSquaredError[:3] == [np.float32(k / 8) for k in (1, 2, 3)]
    assert som.metrics.MeanSquaredError[3:] == [0.0] * 3
    assert (data.lastBMU == np.arange(20, dtype=np.uint64)).all()
    assert not data.hasReadWholeDataStream() and data.isAtStartOfDataStream()
    # a data set without validity flags: every column is valid (one row of J ones)
    ctx2 = StubCtx(4)
    som2 = stub_som(ctx2)
    som2.trainBatchSomResidentMasked(vs.ArrayDataSet(X), 2, 2.0, 0.0)
    assert ctx2.calls[1][2].shape == (4,) and ctx2.calls[1][2].all()
