"""CPU: the masked chunk call of the accumulated epoch (vsom_batch_accum_chunk_masked) is declared, exported and bound;
Context.batch_accum_chunk_masked checks the shape of its mask before any call into the library; Som.trainBatchSomWholeMasked
has trainBatchSomWhole's signature and hands every chunk's validity to the masked call."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from vsom_amd import capi
from vsom_amd import som as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vsom_batch_accum_chunk_masked"


def test_symbol_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert "int vsom_batch_accum_chunk_masked(vsom_ctx *ctx, const uint8_t *valid_host, int one_mask);" in txt
    assert NAME in capi.SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), NAME)


def test_the_header_no_longer_lists_it_as_out_of_scope():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert "a masked accumulating epoch" not in txt


def test_signatures():
    assert list(inspect.signature(capi.Context.batch_accum_chunk_masked).parameters) == ["self", "valid"]
    p = inspect.signature(vs.Som.trainBatchSomWholeMasked).parameters
    assert list(p) == ["self", "data", "numberOfEpochs", "sigma0", "sigmaDecay", "updateUMatrixAfterEpoch", "reset_bmu"]
    assert p["updateUMatrixAfterEpoch"].default is False and p["reset_bmu"].default is True
    assert inspect.signature(vs.Som.trainBatchSomWholeMasked) == inspect.signature(vs.Som.trainBatchSomWhole)


class _NoLibrary:
    """stands where the library would: any call through it is the failure"""

    def __getattr__(self, name):
        raise AssertionError(f"{name} was reached")


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len

    def close(self):
        pass


@pytest.mark.parametrize("bad", [np.ones(4), np.ones(6), np.ones((7, 4)), np.ones((6, 5)), np.ones((8, 5)), np.ones((7, 5, 1)),
                                 np.ones(()), np.ones((5, 7))], ids=lambda a: "x".join(map(str, a.shape)) or "scalar")
def test_shape_errors_raise_before_the_c_call(monkeypatch, bad):
    monkeypatch.setattr(capi, "lib", lambda: _NoLibrary())
    with pytest.raises(ValueError, match="valid has shape"):
        NoDevice(5).batch_accum_chunk_masked(bad)


def test_valid_masks_reach_the_library(monkeypatch):
    seen = []

    class Lib:
        def vsom_batch_accum_chunk_masked(self, h, ptr, one):
            n = 5 if one else 35
            seen.append((one, bytes(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint8))[:n])))
            return 0

    monkeypatch.setattr(capi, "lib", lambda: Lib())
    ctx = NoDevice(5)
    ctx.batch_accum_chunk_masked(np.array([1, 0, 2.5, 0, -1]))                 # nonzero = valid
    full = np.arange(35).reshape(7, 5) % 3
    ctx.batch_accum_chunk_masked(full)
    ctx.batch_accum_chunk_masked(np.asfortranarray(full))                       # any memory order: B x J row-major bytes
    assert seen[0] == (1, bytes([1, 0, 1, 0, 1]))
    assert seen[1] == (0, bytes((full != 0).astype(np.uint8).ravel())) and seen[2] == seen[1]


class _RecordingContext:
    """the calls of Som's whole-data-set driver, without a device"""

    in_len = 3

    def __init__(self):
        self.calls = []
        self.rows = None

    def batch_accum_begin(self, sigma, first, total):
        self.calls.append(("begin", bool(first), total))

    def prefetch_chunk(self, rows):
        self.next = rows

    def commit_chunk(self):
        self.rows = self.next

    def set_last_bmu(self, lb):
        pass

    def batch_accum_chunk(self):
        self.calls.append(("chunk", self.rows.shape[0]))

    def batch_accum_chunk_masked(self, valid):
        self.calls.append(("masked", self.rows.shape[0], np.array(valid)))

    def get_last_bmu(self):
        return np.zeros(self.rows.shape[0], np.uint64)

    def batch_accum_end(self):
        self.calls.append(("end",))
        return np.float32(0.25)

    def batch_accum_abort(self):
        self.calls.append(("abort",))


class _FlaggedDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with a `validity` attribute that belongs to the rows currently loaded"""

    def __init__(self, X, V, chunk):
        super().__init__(X, chunk)
        self.V = V

    def loadNextDataFromStream(self):
        pos = self._pos
        super().loadNextDataFromStream()
        self.validity = self.V[pos:pos + self.data.shape[0]]


def _driver(data, masked=True):
    s = vs.Som.__new__(vs.Som)
    s.ctx, s._verbose = _RecordingContext(), False
    (s.trainBatchSomWholeMasked if masked else s.trainBatchSomWhole)(data, 3, 2.0, 0.5)    # sigma 2, 1.21, then 0.74 < 1
    return s


def test_the_driver_hands_every_chunk_its_own_validity():
    X = np.arange(30, dtype=np.float32).reshape(10, 3)
    V = (np.arange(30).reshape(10, 3) % 4 != 0).astype(np.uint8)
    s = _driver(_FlaggedDataSet(X, V, 4))
    calls = s.ctx.calls
    assert [c[0] for c in calls] == ["begin", "masked", "masked", "masked", "end"] * 2
    assert calls[0] == ("begin", True, 10) and calls[5] == ("begin", False, 10)
    for base in (0, 5):
        off = 0
        for _, rows, valid in calls[base + 1:base + 4]:
            # the mask of the chunk being accumulated, not of the chunk already loaded behind it
            assert valid.shape == (rows, 3) and (valid == V[off:off + rows]).all()
            off += rows
        assert off == 10
    assert list(s.metrics.MeanSquaredError) == [np.float32(0.25), np.float32(0.25), 0.0]


def test_the_driver_without_a_validity_attribute_is_all_valid():
    X = np.zeros((10, 3), np.float32)
    s = _driver(vs.ArrayDataSet(X, 6))
    masks = [c[2] for c in s.ctx.calls if c[0] == "masked"]
    assert len(masks) == 4 and all(m.shape == (3,) and m.all() for m in masks)
    # and the plain driver still makes the plain call
    assert [c[0] for c in _driver(vs.ArrayDataSet(X, 6), masked=False).ctx.calls] == ["begin", "chunk", "chunk", "end"] * 2
