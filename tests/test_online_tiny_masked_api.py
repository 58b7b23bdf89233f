"""CPU tier of the one-launch masked online chunk (vsom_online_masked_tiny_applies, vsom_ensemble_train_online_chunk_masked;
DESIGN.md section 4u): the symbols are declared, listed and exported, and Ensemble.train_online_chunk_masked refuses a
wrong `valid` list before any call into the library (stub contexts: no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsom_online_masked_tiny_applies", "vsom_ensemble_train_online_chunk_masked")


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
    assert callable(getattr(capi.Context, "online_masked_tiny_applies"))
    assert callable(getattr(capi.Ensemble, "train_online_chunk_masked"))


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len

    def close(self):
        pass


BAD = (np.ones(4), np.ones((7, 4)), np.ones((6, 5)), np.ones((7, 5, 1)), np.ones(()))


def test_ensemble_shape_checks_raise_before_the_call():
    a, b = NoDevice(5), NoDevice(3)
    ens = capi.Ensemble.__new__(capi.Ensemble)
    ens.members, ens._h, ens._pinned = [a, b], None, None

    def call(v):
        return ens.train_online_chunk_masked(0.3, 2.0, capi.EXPONENTIAL, v)

    for bad in BAD:
        with pytest.raises(ValueError, match="valid has shape"):
            call([bad, None])
    with pytest.raises(ValueError, match="valid has shape"):
        call([np.ones((7, 5)), np.ones(5)])          # member 1 has 3 columns
    for wrong in ([np.ones((7, 5))], [None, None, None], np.ones((2, 7, 5)), None):
        with pytest.raises(ValueError, match="one entry per member"):
            call(wrong)
