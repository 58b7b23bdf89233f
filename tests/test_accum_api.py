"""CPU: the accumulated batch epoch (vsom_batch_accum_begin / _chunk / _end / _abort) is declared, exported and bound;
the Python argument checks raise before any call into the library; Som.trainBatchSomWhole has its signature."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from vsom_amd import capi
from vsom_amd import som as vs

NAMES = ("vsom_batch_accum_begin", "vsom_batch_accum_chunk", "vsom_batch_accum_end", "vsom_batch_accum_abort")


def test_symbols_listed_and_exported():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert n in capi.SYMBOLS, n
        assert hasattr(L, n), n


class _NoLibrary:
    """stands where the library would: any call through it is the failure"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


@pytest.mark.parametrize("sigma, rows", [(2.0, -1), (2.0, -70), (float("nan"), 10), (float("inf"), 10), (-float("inf"), 10),
                                         (2.0, 1.5)])
def test_argument_errors_raise_before_the_c_call(monkeypatch, sigma, rows):
    ctx = capi.Context.__new__(capi.Context)        # no device: the checks come before the handle is used
    ctx._h, ctx._owned = None, False
    monkeypatch.setattr(capi, "lib", lambda: _NoLibrary())
    with pytest.raises(ValueError):
        ctx.batch_accum_begin(sigma, True, rows)


def test_valid_arguments_reach_the_library(monkeypatch):
    seen = []

    class Lib:
        def vsom_batch_accum_begin(self, h, sigma, first, rows):
            seen.append((sigma, first, rows))
            return 0

    ctx = capi.Context.__new__(capi.Context)
    ctx._h, ctx._owned = None, False
    monkeypatch.setattr(capi, "lib", lambda: Lib())
    ctx.batch_accum_begin(np.float32(2.5), 1, np.int64(70))
    ctx.batch_accum_begin(1.0, False, 0)
    assert seen == [(2.5, 1, 70), (1.0, 0, 0)]


def test_context_methods():
    for n in ("batch_accum_begin", "batch_accum_chunk", "batch_accum_end", "batch_accum_abort"):
        assert callable(getattr(capi.Context, n)), n
    assert list(inspect.signature(capi.Context.batch_accum_begin).parameters) == ["self", "sigma", "is_first", "total_rows"]


def test_train_batch_som_whole_signature():
    p = inspect.signature(vs.Som.trainBatchSomWhole).parameters
    assert list(p) == ["self", "data", "numberOfEpochs", "sigma0", "sigmaDecay", "updateUMatrixAfterEpoch", "reset_bmu"]
    assert p["updateUMatrixAfterEpoch"].default is False and p["reset_bmu"].default is True


def test_stream_rows_counts_a_data_set_that_cannot_tell():
    class Stream(vs.ArrayDataSet):
        totalRows = None

        def __getattribute__(self, name):
            if name == "totalRows":
                raise AttributeError(name)
            return super().__getattribute__(name)

    X = np.zeros((110, 3), np.float32)
    assert vs.Som._streamRows(vs.ArrayDataSet(X, 70)) == 110
    ds = Stream(X, 70)
    assert not hasattr(ds, "totalRows")
    assert vs.Som._streamRows(ds) == 110
    assert ds.isAtStartOfDataStream() and not ds.hasReadWholeDataStream()     # the counting pass leaves a clean stream
