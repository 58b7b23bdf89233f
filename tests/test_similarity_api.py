"""vsom_similarity_batch without a GPU: the symbol is declared, exported and bound; the Python wrappers exist and check
their arguments before reaching the library; the C call refuses a null context; measure_similarity_from_rows equals the
reference's literal double loop (Som.cpp:641-711) on seeded random delta matrices."""
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
import similarity_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert re.search(r"int\s+vsom_similarity_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+min_hits\s*,\s*int\s+num_sigmas"
                     r"\s*,\s*int\s+sigma_rule\s*,\s*size_t\s+r0\s*,\s*size_t\s+r1\s*,\s*const\s+uint8_t\s*\*\s*valid_host"
                     r"\s*,\s*vsom_similarity_out\s*\*\s*out\s*\)", txt)
    assert "VSOM_SIGMA_AS_WRITTEN = 0" in txt and "VSOM_SIGMA_FLOOR = 1" in txt
    assert "vsom_similarity_batch" in capi.SYMBOLS
    L = _lib()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "vsom_similarity_batch")
    assert len(L.vsom_similarity_batch.argtypes) == 8
    assert (capi.SIGMA_AS_WRITTEN, capi.SIGMA_FLOOR) == (0, 1)
    assert [f[0] for f in capi.SimilarityOut._fields_] == ["bmu", "dist", "dmax", "dmax_col", "first", "amax", "amax_col",
                                                          "outside", "delta"]
    assert ctypes.sizeof(capi.SimilarityOut) == 9 * ctypes.sizeof(ctypes.c_void_p)


def test_wrappers_exist():
    assert callable(getattr(capi.Context, "similarity", None))
    assert callable(getattr(vs.Som, "measureSimilarity", None))
    assert callable(getattr(vs.Som, "similarityRows", None))
    assert callable(getattr(vs, "measure_similarity_from_rows", None))


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, rows of 7 values, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100
        self.in_len = 7
        self.depth = 7


@pytest.mark.parametrize("kw", [dict(r0=5, r1=4), dict(r1=11), dict(r0=-1, r1=3), dict(sigma_rule=2), dict(sigma_rule=-1),
                                dict(min_hits=-1), dict(num_sigmas=2 ** 31), dict(valid=np.ones((10, 6))),
                                dict(valid=np.ones((9, 7))), dict(r0=2, r1=5, valid=np.ones((10, 7)))])
def test_wrapper_refuses_before_the_library(monkeypatch, kw):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    args = dict(min_hits=1, num_sigmas=3)
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().similarity(**args)


def test_null_context_and_null_out_refused():
    L = _lib()
    out = capi.SimilarityOut()
    rc = L.vsom_similarity_batch(None, 1, 3, 0, 0, 1, None, ctypes.byref(out))
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


# ---- the finish: measure_similarity_from_rows against the literal loop ------------------------------------------------
def _check(delta):
    delta = np.ascontiguousarray(delta, np.float32)
    first, dmax, _ = ref.rows_from_delta(delta)
    outside = np.arange(delta.shape[0]) % 2            # the reported row decides the verdict: odd rows "fail"
    row, ok = vs.measure_similarity_from_rows(first, dmax, outside)
    want, _ = ref.literal_loop(delta)
    assert row == want, (row, want, delta)
    assert ok == (outside[want] == 0)


def _random_delta(rng, n, C):
    kind = rng.integers(0, 6)
    d = rng.standard_normal((n, C)).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 9))
    if kind == 1:
        d = -np.abs(d)                                 # all negative: only the first trigger ever fires
    elif kind == 2:
        d[...] = d.flat[0]                             # all equal
    elif kind == 3:
        d = np.round(d)                                # many ties
    specials = np.array([np.nan, np.inf, -np.inf, -99999999.0, -1.0e9, -3.0e38, 0.0, -0.0], np.float32)
    mask = rng.random((n, C)) < rng.choice([0.0, 0.1, 0.5, 0.9])
    d[mask] = rng.choice(specials, size=int(mask.sum()))
    if kind == 4 and n > 1:
        d[rng.integers(0, n)] = np.nan                 # an all-NaN row
    return d


def test_finish_equals_the_literal_loop_on_random_matrices():
    rng = np.random.default_rng(20261016)
    for _ in range(3000):
        n, C = int(rng.integers(1, 9)), int(rng.integers(1, 8))
        _check(_random_delta(rng, n, C))


def test_finish_on_engineered_matrices():
    nan, inf = np.nan, np.inf
    # a negative first trigger larger in magnitude than every positive delta: the first row stays the reported one
    _check([[-1000.0, 3.0, 5.0], [7.0, 900.0, 999.0], [1.0, 2.0, 3.0]])
    # ... until a positive delta exceeds that magnitude
    _check([[-1000.0, 3.0, 5.0], [7.0, 900.0, 1001.0], [2000.0, 2.0, 3.0]])
    # values at or below the start value never trigger; the first one above does
    _check([[-99999999.0, -1.0e9, nan], [nan, -inf, -2.0e8], [-5.0, nan, nan], [4.0, nan, 6.0]])
    _check([[nan, nan], [nan, nan]])                   # nothing triggers: row 0
    _check([[-inf, -inf], [-1.0e9, -99999999.0]])
    _check([[nan, nan, nan], [nan, 2.0, nan], [nan, nan, 2.0], [nan, 2.5, nan]])
    _check([[inf, 1.0], [inf, inf], [3.0, 4.0]])       # +inf: stays with the first row that has it
    _check([[1.0, -inf], [2.0, inf]])
    _check([[5.0]])                                    # one row, one column
    _check([[nan]])
    _check([[-3.0], [2.0], [3.0], [3.5], [3.5]])       # one column
    _check([[1.0, 2.0, 3.0, 2.0, 9.0, -9.0, nan]])     # one row
    _check([[-2.0, 1.0, 2.0, 2.5]])                    # the trigger row's later columns: 2.5 > |-2|
    _check([[0.0, -0.0], [-0.0, 0.0]])


def test_finish_refuses_mismatched_lengths_and_accepts_no_rows():
    with pytest.raises(ValueError):
        vs.measure_similarity_from_rows(np.zeros(3, np.float32), np.zeros(2, np.float32), np.zeros(3, np.uint32))
    assert vs.measure_similarity_from_rows(np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32)) == (0, True)
