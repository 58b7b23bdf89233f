"""vsom_bmu_topk_batch without a GPU: the symbol is declared, exported and bound; the Python wrappers exist and check
their arguments before reaching the library; the C call refuses a null context; topographic_error on hand-worked grids."""
import ctypes
import os
import re

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert re.search(r"int\s+vsom_bmu_topk_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+k\s*,\s*size_t\s+r0\s*,"
                     r"\s*size_t\s+r1\s*,\s*uint64_t\s*\*\s*idx_out\s*,\s*float\s*\*\s*dist_out\s*\)", txt)
    assert "vsom_bmu_topk_batch" in capi.SYMBOLS
    L = _lib()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "vsom_bmu_topk_batch")
    assert L.vsom_bmu_topk_batch.argtypes is not None and len(L.vsom_bmu_topk_batch.argtypes) == 6


def test_wrappers_exist():
    assert callable(getattr(capi.Context, "bmu_topk", None))
    assert callable(getattr(vs.Som, "findBestMatchingUnits", None))
    assert callable(getattr(vs.Som, "topographicError", None))
    assert callable(getattr(vs, "topographic_error", None))


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100


@pytest.mark.parametrize("k, r0, r1", [(0, 0, None), (65, 0, None), (2, 5, 4), (2, 0, 11), (2, -1, 3)])
def test_wrapper_refuses_before_the_library(monkeypatch, k, r0, r1):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    with pytest.raises(ValueError):
        _Stub().bmu_topk(k, r0, r1)


def test_wrapper_refuses_k_above_n(monkeypatch):
    monkeypatch.setattr(capi, "lib", lambda: (_ for _ in ()).throw(AssertionError("reached the library")))
    s = _Stub()
    s.n_nodes = 3
    with pytest.raises(ValueError):
        s.bmu_topk(4)


def test_null_context_refused():
    L = _lib()
    idx = np.zeros(4, np.uint64)
    rc = L.vsom_bmu_topk_batch(None, 2, 0, 2, capi._u(idx), None)
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


def _te(pairs, W):
    return vs.topographic_error(np.array(pairs, np.uint64).reshape(-1, 2), W)


def test_topographic_error_neighbours_in_all_directions():
    W = 5
    c = 2 * W + 2                                      # (row 2, column 2)
    nbrs = [c - W - 1, c - W, c - W + 1, c - 1, c + 1, c + W - 1, c + W, c + W + 1]
    assert _te([(c, n) for n in nbrs], W) == 0.0
    assert _te([(n, c) for n in nbrs], W) == 0.0


def test_topographic_error_far_and_wrapped_pairs():
    W, H = 5, 4
    assert _te([(0, 2)], W) == 1.0                     # two apart in a row
    assert _te([(0, 2 * W)], W) == 1.0                 # two apart in a column
    assert _te([(W - 1, W)], W) == 1.0                 # end of row 0 / start of row 1: no wrap
    assert _te([(0, W - 1)], W) == 1.0                 # the two ends of a row
    assert _te([(0, (H - 1) * W)], W) == 1.0           # top / bottom: no wrap
    assert _te([(0, 1), (0, 2), (0, W + 1), (3, 10)], W) == 0.5


def test_topographic_error_non_square_map():
    # W = 7, H = 3: node n at (n // 7, n % 7); SomIndex::fromLinear's divide-by-height would place 7 at row 2
    W = 7
    assert _te([(0, 7)], W) == 0.0                     # (0,0) - (1,0)
    assert _te([(6, 7)], W) == 1.0                     # (0,6) - (1,0)
    assert _te([(6, 13)], W) == 0.0                    # (0,6) - (1,6)
    assert _te([(0, 14)], W) == 1.0                    # (0,0) - (2,0)
    assert _te([(8, 16), (8, 1), (8, 15), (8, 3)], W) == 0.25
    # W = 3, H = 7
    assert _te([(2, 3)], 3) == 1.0 and _te([(2, 5)], 3) == 0.0 and _te([(0, 4)], 3) == 0.0


def test_topographic_error_empty_and_extra_columns():
    assert vs.topographic_error(np.zeros((0, 2), np.uint64), 4) == 0.0
    assert vs.topographic_error(np.array([[0, 1, 9], [0, 5, 1]], np.uint64), 4) == 0.0   # columns 0 and 1 only
    r = vs.topographic_error(np.array([[0, 2]] * 3 + [[0, 1]] * 4, np.uint64), 4)
    assert r == 3.0 / 7.0 and isinstance(r, float)
