"""CPU tier of the ensemble's masked queries (vsom_ensemble_bmu_masked_batch, vsom_ensemble_similarity_masked_batch;
DESIGN.md section 4v): the symbols are declared, listed and exported, and Ensemble.bmu_masked / similarity_masked / impute
refuse wrong arguments before any call into the library (stub contexts: no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsom_ensemble_bmu_masked_batch", "vsom_ensemble_similarity_masked_batch")


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
    for name in ("bmu_masked", "similarity_masked", "impute"):
        assert callable(getattr(capi.Ensemble, name)), name


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len

    def close(self):
        pass


BAD = (np.ones(4), np.ones((7, 4)), np.ones((6, 5)), np.ones((7, 5, 1)), np.ones(()))


def stub():
    ens = capi.Ensemble.__new__(capi.Ensemble)
    ens.members, ens._h, ens._pinned = [NoDevice(5), NoDevice(3)], None, None
    return ens


CALLS = (lambda e, v: e.bmu_masked(v), lambda e, v: e.bmu_masked(v, min_hits=2, fill=True), lambda e, v: e.impute(v),
         lambda e, v: e.similarity_masked(v, 0, 3), lambda e, v: e.similarity_masked(v, [0, 1], [3, 2], delta=True))


@pytest.mark.parametrize("call", CALLS)
def test_validity_checks_raise_before_the_call(call):
    ens = stub()
    for bad in BAD:
        with pytest.raises(ValueError, match="valid has shape"):
            call(ens, [bad, None])
    with pytest.raises(ValueError, match="valid has shape"):
        call(ens, [np.ones((7, 5)), np.ones(5)])          # member 1 has 3 columns
    for wrong in ([np.ones((7, 5))], [None, None, None], np.ones((2, 7, 5)), None):
        with pytest.raises(ValueError, match=r"one entry per member \(2\), None for a skipped member"):
            call(ens, wrong)


def test_parameter_checks_raise_before_the_call():
    ens = stub()
    ok = [np.ones((7, 5)), np.ones(3)]
    with pytest.raises(ValueError, match="min_hits must be >= 0"):
        ens.bmu_masked(ok, min_hits=-1)
    with pytest.raises(ValueError, match="min_hits must be >= 0"):
        ens.similarity_masked(ok, [0, -2], 3)
    with pytest.raises(ValueError, match="values of min_hits for 2 members"):
        ens.bmu_masked(ok, min_hits=[1, 2, 3])
    with pytest.raises(ValueError, match="values of min_hits for 2 members"):
        ens.impute(ok, min_hits=[1])
    with pytest.raises(ValueError, match="values of num_sigmas for 2 members"):
        ens.similarity_masked(ok, 0, [3])
    with pytest.raises(ValueError, match="num_sigmas must fit an int"):
        ens.similarity_masked(ok, 0, [3, 2 ** 31])
    for rule in (2, -1):
        with pytest.raises(ValueError, match="sigma_rule"):
            ens.similarity_masked(ok, 0, 3, sigma_rule=rule)
