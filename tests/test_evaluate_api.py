"""vsom_evaluate_batch without a GPU: the symbol is declared, exported and bound; the Python and C++ wrappers exist; the
Python wrapper checks its arguments before reaching the library; the C call refuses a null context; the fp32 restatement
the GPU tests use agrees with the float64 one within the stated tolerance on ordinary operands."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert re.search(r"int\s+vsom_evaluate_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*size_t\s+r0\s*,\s*size_t\s+r1\s*,"
                     r"\s*const\s+float\s*\*\s*binary_host\s*,\s*const\s+float\s*\*\s*continuous_host\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*valid_host\s*,\s*vsom_evaluate_out\s*\*\s*out\s*\)", txt)
    assert re.search(r"typedef\s+struct\s+vsom_evaluate_out\s*\{\s*uint64_t\s*\*\s*bmu\s*;\s*float\s*\*\s*dist\s*;"
                     r"\s*float\s*\*\s*bsum\s*;\s*uint32_t\s*\*\s*nrepl\s*;\s*double\s*\*\s*error\s*;\s*\}\s*vsom_evaluate_out\s*;", txt)
    assert "vsom_evaluate_batch" in capi.SYMBOLS
    L = _lib()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "vsom_evaluate_batch")
    assert len(L.vsom_evaluate_batch.argtypes) == 7
    assert [f[0] for f in capi.EvaluateOut._fields_] == ["bmu", "dist", "bsum", "nrepl", "error"]
    assert ctypes.sizeof(capi.EvaluateOut) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_wrappers_exist():
    assert callable(getattr(capi.Context, "evaluate", None))
    assert callable(getattr(vs.Som, "evaluate", None))
    assert callable(getattr(vs.Som, "evaluateRows", None))
    hpp = open(os.path.join(HOST, "include", "vsom_api.hpp")).read()
    assert re.search(r"EvaluateRows\s+evaluateRows\s*\(\s*const\s+DataSet\s*&\s*\w+\s*\)\s*const\s*;", hpp)
    assert re.search(r"double\s+evaluate\s*\(\s*const\s+DataSet\s*&\s*\w+\s*\)\s*const\s*;", hpp)
    assert "host_evaluate_test" in open(os.path.join(HOST, "build.sh")).read()


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, rows of 7 values, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100
        self.in_len = 7
        self.depth = 7


@pytest.mark.parametrize("kw", [dict(binary=np.zeros(6)), dict(binary=np.zeros(8)), dict(binary=np.zeros((1, 7))),
                                dict(continuous=np.ones(6)), dict(continuous=np.ones(8)), dict(continuous=np.ones((7, 1))),
                                dict(valid=np.ones((10, 6))), dict(valid=np.ones((9, 7))), dict(valid=np.ones(70)),
                                dict(r0=2, r1=5, valid=np.ones((10, 7))), dict(r0=5, r1=4), dict(r1=11),
                                dict(r0=-1, r1=3)])
def test_wrapper_refuses_before_the_library(monkeypatch, kw):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    args = dict(binary=np.zeros(7), continuous=np.ones(7))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().evaluate(**args)


def test_null_context_refused():
    L = _lib()
    out = capi.EvaluateOut()
    cols = np.zeros(7, np.float32)
    p = cols.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = L.vsom_evaluate_batch(None, 0, 1, p, p, None, ctypes.byref(out))
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


# ---- the restatements the GPU tests hold the device to -------------------------------------------------------------------
def test_restatements_agree_with_each_other():
    """numpy's fp32 log is within an ulp too: on ordinary operands the fp32 restatement lies within the stated bound of the
    float64 one, the counts agree, and a zero factor or a replaced term is the same in both"""
    rng = np.random.default_rng(7)
    for C in (3, 7, 9, 12, 15, 37, 100):
        n = 40
        M = rng.uniform(0.02, 0.98, (n, C)).astype(np.float32)
        X = rng.random((n, C)).astype(np.float32)
        X[:, ::3] = np.float32(0)
        X[:, 1::5] = np.float32(1)
        binary = (rng.random(C) < 0.5).astype(np.float32)
        continuous = (rng.random(C) < 0.8).astype(np.float32)
        valid = rng.random((n, C)) < 0.6
        for v in (None, valid):
            b64, n64 = ref.restate64(X, M, binary, continuous, v)
            b32, n32, _, _ = ref.restate32(X, M, binary, continuous, v)
            assert (n64 == 0).all() and (n32 == 0).all()
            assert ((b64 == 0) == (b32 == 0)).all()
            nz = b64 != 0
            assert (np.abs(b32[nz].astype(np.float64) - b64[nz]) <= ref.bound(C) * b64[nz]).all()
    # replaced terms: exact in both
    M = np.array([[0.0, 1.0, -0.5, 2.0, np.nan, np.inf, 0.5]], np.float32)
    X = np.array([[0.5, 0.0, 1.0, 0.5, 0.0, 1.0, 0.25]], np.float32)
    binary = np.array([1, 1, 1, 1, 1, 1, 0], np.float32)
    b64, n64 = ref.restate64(X, M, binary, np.ones(7, np.float32))
    b32, n32, exact, _ = ref.restate32(X, M, binary, np.ones(7, np.float32))
    assert n64[0] == 6 and n32[0] == 6 and exact[0]
    assert abs(float(b32[0]) - b64[0]) <= 7 * 2.0 ** -24 * b64[0]


def test_running_mean():
    assert ref.running_mean([], []) == 0.0
    assert ref.running_mean(np.float32([3.0]), np.float32([16.0])) == 7.0
    assert ref.running_mean(np.float32([1.0, 3.0]), np.float32([0.0, 0.0])) == 2.0
    assert np.isnan(ref.running_mean(np.float32([1.0, np.nan, 2.0]), np.float32([0.0, 0.0, 0.0])))
