"""CPU tier of the ensemble's top-k calls (vsom_ensemble_bmu_topk_batch, vsom_ensemble_bmu_topk_masked_batch,
vsom_ensemble_topk_applies): the symbols are declared, listed and exported, the ctypes structure has
the header's layout, and Ensemble.bmu_topk / bmu_topk_masked / topographic_error_masked refuse wrong arguments before any
call into the library (stub contexts: no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsom_ensemble_bmu_topk_batch", "vsom_ensemble_bmu_topk_masked_batch", "vsom_ensemble_topk_applies")


def header():
    return open(os.path.join(ROOT, "include", "vsom_hip.h")).read()


def test_new_symbols_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(vsom_[a-z0-9_]+)\s*\(", txt))
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(L, name), name
    for name in ("bmu_topk", "bmu_topk_masked", "topk_applies", "topographic_error", "topographic_error_masked"):
        assert callable(getattr(capi.Ensemble, name)), name


def test_structure_layout_matches_the_header():
    """vsom_ensemble_topk_out: four pointers -- idx, dist, count, nvalid -- of the header's types, in its order, and no
    blend field"""
    body = re.search(r"typedef\s+struct\s+vsom_ensemble_topk_out\s*\{(.*?)\}\s*vsom_ensemble_topk_out\s*;", header(), re.S)
    assert body
    fields = re.findall(r"(\w+)\s*\*\s*(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S))
    assert fields == [("uint64_t", "idx"), ("float", "dist"), ("uint32_t", "count"), ("uint32_t", "nvalid")]
    ctype = {"uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    assert [(n, t) for n, t in capi.EnsembleTopkOut._fields_] == [(n, ctypes.POINTER(ctype[t])) for t, n in fields]
    assert ctypes.sizeof(capi.EnsembleTopkOut) == 4 * ctypes.sizeof(ctypes.c_void_p)
    for i, (_, name) in enumerate(fields):
        assert getattr(capi.EnsembleTopkOut, name).offset == i * ctypes.sizeof(ctypes.c_void_p), name
    assert "blend" not in body.group(1)


def test_null_ensemble_is_refused_without_a_device():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = capi.lib()
    ks = (ctypes.c_uint32 * 1)(2)
    outs = (capi.EnsembleTopkOut * 1)()
    vp = (ctypes.POINTER(ctypes.c_uint8) * 1)()
    assert L.vsom_ensemble_bmu_topk_batch(None, ks, outs) == -1
    assert b"null ensemble" in L.vsom_last_error()
    assert L.vsom_ensemble_bmu_topk_masked_batch(None, ks, None, vp, None, outs) == -1
    assert b"null ensemble" in L.vsom_last_error()
    assert L.vsom_ensemble_topk_applies(None, 0, 2, 0) == -1
    assert b"null ensemble" in L.vsom_last_error()


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len
        self.width, self.height, self.n_nodes = 5, 3, 15

    def close(self):
        pass


def stub():
    ens = capi.Ensemble.__new__(capi.Ensemble)
    ens.members, ens._h, ens._pinned = [NoDevice(5), NoDevice(3)], None, None
    return ens


OK = [np.ones((7, 5)), np.ones(3)]


def test_k_checks_raise_before_the_call():
    ens = stub()
    for bad in ([2], [2, 2, 2], []):
        with pytest.raises(ValueError, match="values of k for 2 members"):
            ens.bmu_topk(bad)
        with pytest.raises(ValueError, match="values of k for 2 members"):
            ens.bmu_topk_masked(bad, OK)
    for bad in (0, 65, [2, 0], [65, 2], -1):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            ens.bmu_topk(bad)
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            ens.bmu_topk_masked(bad, OK)
    for bad in ([2], [0, 5], [-1]):
        with pytest.raises(ValueError, match="members must be indices"):
            ens.bmu_topk(2, members=bad)


BAD = (np.ones(4), np.ones((7, 4)), np.ones((6, 5)), np.ones((7, 5, 1)), np.ones(()))
CALLS = (lambda e, v: e.bmu_topk_masked(2, v), lambda e, v: e.bmu_topk_masked([1, 3], v, min_hits=2, dist=False),
         lambda e, v: e.topographic_error_masked(v), lambda e, v: e.topographic_error_masked(v, min_hits=[0, 1]))


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


def test_min_hits_checks_raise_before_the_call():
    ens = stub()
    with pytest.raises(ValueError, match="min_hits must be >= 0"):
        ens.bmu_topk_masked(2, OK, min_hits=-1)
    with pytest.raises(ValueError, match="values of min_hits for 2 members"):
        ens.bmu_topk_masked(2, OK, min_hits=[1, 2, 3])
    with pytest.raises(ValueError, match="min_hits must be >= 0"):
        ens.topographic_error_masked(OK, min_hits=[0, -2])
