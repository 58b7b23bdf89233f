"""CPU: vsom_train_online_chunk_masked is declared, listed and exported; its Python layers exist and check the shape of
`valid` before any call into the library (no device needed)."""
import ctypes
import os

import numpy as np
import pytest

from vsom_amd import capi
from vsom_amd import som as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "vsom_train_online_chunk_masked"


def test_declared_listed_and_exported():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert ("int vsom_train_online_chunk_masked(vsom_ctx *ctx, double eta, double sigma, int decay_fn, int first_chunk,"
            in txt)
    assert NAME in capi.SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), NAME)
    assert capi.TIMER_NAMES and len(capi.TIMER_NAMES) == 7        # VSOM_T_COUNT stays 7: no new timing group


def test_python_layers_exist():
    assert callable(getattr(capi.Context, "train_online_chunk_masked"))
    assert callable(getattr(vs.Som, "trainBasicSomMasked"))


class _NoDevice(capi.Context):
    """a Context that never reaches the library: the shape check comes first"""

    def __init__(self, in_len, rows):
        self.in_len, self._rows, self._h = in_len, rows, None

    @property
    def chunk_size(self):
        return self._rows

    def close(self):
        pass

    def __del__(self):
        pass


@pytest.mark.parametrize("bad", [np.ones((4, 6), np.uint8), np.ones((5, 5), np.uint8), np.ones(6, np.uint8),
                                 np.ones((5, 6, 1), np.uint8), np.ones((), np.uint8)])
def test_a_wrongly_shaped_valid_is_a_value_error_without_a_device(bad, monkeypatch):
    def no_library():
        raise AssertionError("the library was called before the shape check")

    monkeypatch.setattr(capi, "lib", no_library)
    ctx = _NoDevice(5, 4)            # J = 5, B = 4
    with pytest.raises(ValueError, match="valid has shape"):
        ctx.train_online_chunk_masked(0.3, 2.0, capi.EXPONENTIAL, bad)
