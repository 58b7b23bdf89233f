"""vsom_bmu_topk_masked_batch without a GPU: the entry point and its struct are declared, exported and bound; the Python
wrappers and the C++ mirror's methods exist; the wrapper checks its arguments before reaching the library; the C call refuses
a null context; the custom kernel text still compiles.  And the reference of the GPU tests (tests/topk_masked_ref.py) is
consistent with itself: with an all-valid mask and min_hits = 0 its lists are the key sort of the oracle's distances (the
`expected` of tests/test_gpu_topk.py, restated here), its candidate counts are the ones the GPU cases rely on, and its blend
stays within the contract's bound of a numpy.longdouble evaluation."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
import topk_masked_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert re.search(r"int\s+vsom_bmu_topk_masked_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+k\s*,\s*uint64_t\s+min_hits\s*,"
                     r"\s*size_t\s+r0\s*,\s*size_t\s+r1\s*,\s*const\s+uint8_t\s*\*\s*valid_host\s*,\s*int\s+one_mask\s*,"
                     r"\s*vsom_topk_masked_out\s*\*\s*out\s*\)", txt)
    assert re.search(r"typedef\s+struct\s+vsom_topk_masked_out\s*\{\s*uint64_t\s*\*\s*idx\s*;\s*float\s*\*\s*dist\s*;"
                     r"\s*uint32_t\s*\*\s*count\s*;\s*uint32_t\s*\*\s*nvalid\s*;\s*double\s*\*\s*blend\s*;\s*\}"
                     r"\s*vsom_topk_masked_out\s*;", txt)
    assert "vsom_bmu_topk_masked_batch" in capi.SYMBOLS
    L = _lib()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "vsom_bmu_topk_masked_batch")
    assert len(L.vsom_bmu_topk_masked_batch.argtypes) == 8
    assert [f[0] for f in capi.TopkMaskedOut._fields_] == ["idx", "dist", "count", "nvalid", "blend"]
    assert ctypes.sizeof(capi.TopkMaskedOut) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_wrappers_exist():
    assert callable(getattr(capi.Context, "bmu_topk_masked", None))
    for name in ("findBestMatchingUnitsMasked", "topographicErrorMasked", "imputeBlend"):
        assert callable(getattr(vs.Som, name, None)), name


def test_cpp_mirror_declares_the_calls():
    txt = open(os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "include", "vsom_api.hpp")).read()
    assert re.search(r"std::vector<uint64_t>\s+findBestMatchingUnitsMasked\s*\(\s*const\s+DataSet\s*\*\s*\w+\s*,\s*size_t\s+k\s*,"
                     r"\s*size_t\s+minBmuHits\s*,\s*std::vector<float>\s*\*\s*dist\s*=\s*nullptr\s*,"
                     r"\s*std::vector<uint32_t>\s*\*\s*count\s*=\s*nullptr\s*\)\s*const", txt)
    assert re.search(r"double\s+topographicErrorMasked\s*\(\s*const\s+DataSet\s*\*\s*\w+\s*,\s*size_t\s+minBmuHits\s*,"
                     r"\s*size_t\s*\*\s*rowsCounted\s*=\s*nullptr\s*\)\s*const", txt)
    assert re.search(r"std::vector<double>\s+imputeBlend\s*\(\s*const\s+DataSet\s*\*\s*\w+\s*,\s*size_t\s+k\s*,"
                     r"\s*size_t\s+minBmuHits\s*\)\s*const", txt)


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, rows of 7 values, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100
        self.in_len = 7
        self.depth = 7


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=-1), dict(k=65), dict(r0=5, r1=4), dict(r1=11), dict(r0=-1, r1=3),
                                dict(min_hits=-1), dict(valid=np.ones((10, 6))), dict(valid=np.ones((9, 7))),
                                dict(valid=np.ones(6)), dict(valid=np.ones(8)), dict(r0=2, r1=5, valid=np.ones((10, 7))),
                                dict(valid=np.ones((10, 7, 1)))])
def test_wrapper_refuses_before_the_library(monkeypatch, kw):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    args = dict(k=2, valid=np.ones((10, 7)))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().bmu_topk_masked(**args)


def test_wrapper_refuses_k_above_n(monkeypatch):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    s = _Stub()
    s.n_nodes = 12
    with pytest.raises(ValueError):
        s.bmu_topk_masked(13, np.ones(7))


def test_null_context_refused():
    L = _lib()
    idx = np.zeros(2, np.uint64)
    out = capi.TopkMaskedOut()
    out.idx = idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    v = (ctypes.c_uint8 * 4)(1, 1, 1, 1)
    rc = L.vsom_bmu_topk_masked_batch(None, 2, 0, 0, 1, v, 1, ctypes.byref(out))
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


@pytest.mark.parametrize("kind", ["standard", "median", "clr"])
def test_custom_kernel_text_still_compiles(kind):
    depth, rlen = hooks.shape(kind, 9)
    L = _lib()
    assert L.vsom_custom_compile_check(hooks.SOURCES[kind].encode(), depth, rlen) == 0, L.vsom_last_error().decode()


# ---- the reference is consistent with itself ----------------------------------------------------------------------------------
def _keys(d):
    bits = d.view(np.uint32).astype(np.uint64)
    bits[np.isnan(d)] = 0xFFFFFFFF
    return (bits << np.uint64(32)) | np.arange(d.size, dtype=np.uint64)


def _expected_row(d, k):
    """tests/test_gpu_topk.py's contract on one row of distances, restated"""
    order = np.argsort(_keys(d), kind="stable")
    if np.isnan(d[0]):
        order = np.concatenate([[0], order[order != 0]])
    idx = order[:k].astype(np.uint64)
    dist = d[idx.astype(np.int64)].copy()
    dist[np.isnan(dist)] = np.uint32(0x7FC00000).view(f32)
    return idx, dist


@pytest.mark.parametrize("tr", ref.bmr.KINDS)
def test_all_valid_lists_are_the_key_sort_of_the_oracle(tr):
    W, H, J = 9, 15, 37
    M, S, hits = ref.bmr.unit_state(W, H, J, 4)
    X = ref.bmr.unit_rows(6, J, 5)
    X[2, 3] = np.nan                                   # a row whose every distance is NaN: the node-0 rule
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=M, hits=hits)
    D = np.array([[o.dist(i, x) for i in range(W * H)] for x in X], f32)
    d = ref.masked_d(tr, X, M, np.ones(J, bool))
    assert ref.beq(d, D)
    for k in (1, 2, 7, 64):
        idx, dist, count = ref.lists(d, hits, 0, k)
        assert (count == k).all()
        for r in range(X.shape[0]):
            ei, ed = _expected_row(D[r], k)
            assert (idx[r] == ei).all() and ref.beq(dist[r], ed), (k, r)
    assert np.isnan(D[2]).all()


def test_candidate_counts_of_the_gpu_cases():
    for tr, W, H, J in ref.SHAPES:
        c = ref.case(tr, W, H, J)
        N = W * H
        assert c["hits"][0] == 0 and c["hits"].max() == 5
        n0, n3, n6 = (ref.candidates(c["hits"], m).size for m in ref.MIN_HITS)
        assert n0 == N and n6 == 1                                       # min_hits = 6: node 0 alone
        # min_hits = 3 (about half the nodes): k = min(64, N) pads on the 7 x 5 map and on no other
        assert (2 <= n3 < 35) if N == 35 else (64 <= n3 < N), (W, H, J, n3)
    assert ref.candidates(ref.case(po.STANDARD, 7, 5, 9)["hits"], 3).size == 18
    # k = min(64, N) pads on the 7 x 5 map under min_hits = 3, and under min_hits = 6 everywhere
    c = ref.case(po.STANDARD, 7, 5, 9)
    idx, dist, count = ref.lists(c["d"], c["hits"], 3, 35)
    assert (count == 18).all() and (idx[:, 18:] == ref.NO_UNIT).all() and (idx[:, :18] < 35).all()
    assert (dist[:, 18:].view(np.uint32) == ref.QNAN32).all()
    idx, dist, count = ref.lists(c["d"], c["hits"], 6, 2)
    assert (count == 1).all() and (idx[:, 0] == 0).all() and (idx[:, 1] == ref.NO_UNIT).all()
    # the row without a valid column: every distance +0, the first candidates in index order
    idx, dist, count = ref.lists(c["d"], c["hits"], 3, 7)
    r = ref.NO_VALID_ROW
    assert (idx[r] == ref.candidates(c["hits"], 3)[:7]).all() and (dist[r].view(np.uint32) == 0).all()


def test_column_zero_is_the_masked_search():
    import masked_score_ref as msr
    for tr, W, H, J in ((po.STANDARD, 9, 15, 9), (po.MEDIAN, 7, 5, 37)):
        c = ref.case(tr, W, H, J)
        for min_hits in ref.MIN_HITS:
            idx, dist, count = ref.lists(c["d"], c["hits"], min_hits, 3)
            bmu, bd = msr.checker(tr, c["X"], c["M"], c["valid"], c["hits"], min_hits)
            assert (idx[:, 0] == bmu).all() and ref.beq(dist[:, 0], bd), (tr, min_hits)


@pytest.mark.parametrize("tr,W,H,J", [(po.STANDARD, 7, 5, 9), (po.MEDIAN, 9, 15, 37), (po.STANDARD, 17, 16, 70)])
def test_blend_against_longdouble(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    worst = 0.0
    for min_hits, k in ((0, 7), (3, min(64, W * H)), (6, 2)):
        idx, dist, count = ref.lists(c["d"], c["hits"], min_hits, k)
        b64, mass = ref.blend(c["X"], c["valid"], c["M"], idx, dist, count)
        bld, massl = ref.blend(c["X"], c["valid"], c["M"], idx, dist, count, np.longdouble)
        assert mass.all() and (mass == massl).all()
        v = c["valid"]
        assert ref.beq(b64[v], c["X"][v].astype(np.float64))                         # valid columns: (double)x on the bits
        bound = ref.blend_bound(c["M"], idx, count, k)
        err = np.abs(b64.astype(np.longdouble) - bld)[~v].astype(np.float64)
        assert (err <= bound[~v]).all()
        worst = max(worst, float((err / bound[~v]).max()))
        # the row without a valid column: the plain mean of its first `count` candidates
        r = ref.NO_VALID_ROW
        n = int(count[r])
        mean = c["M"][idx[r, :n].astype(np.int64)].astype(np.float64).mean(axis=0)
        assert (np.abs(b64[r] - mean) <= bound[r]).all()
    print(f"[topk_masked_ref] {tr}/{W}x{H}x{J}: worst |float64 - longdouble| / bound = {worst:.3f}")
    assert worst < 1.0


def test_blend_without_mass_and_skipped_terms():
    M = np.array([[1.0, 2.0], [3.0, np.inf], [5.0, 6.0]], f32)
    x = np.array([0.5, np.nan], f32)
    valid = np.array([True, False])
    # entry 1 has an infinite distance: skipped, not multiplied -- its inf model entry does not reach the blend
    idx = np.array([[0, 1, ref.NO_UNIT]], np.uint64)
    dist = np.array([[0.0, np.inf, np.nan]], f32)
    b, mass = ref.blend(x[None], valid, M, idx, dist, np.array([2], np.uint32))
    assert mass[0] and b[0].tolist() == [0.5, 2.0]
    # the node-0 rule: a NaN in front, the weights are relative to the first entry that is not NaN
    dist = np.array([[np.nan, 3.0, 3.0]], f32)
    idx = np.array([[1, 0, 2]], np.uint64)
    b, mass = ref.blend(x[None], valid, M, idx, dist, np.array([3], np.uint32))
    assert mass[0] and b[0].tolist() == [0.5, 4.0]
    # no finite distance: no mass, the quiet NaN at the invalid column, x at the valid one
    for dd in ([np.nan, np.nan, np.nan], [np.inf, np.inf, np.nan], [np.nan, np.inf, np.inf]):
        b, mass = ref.blend(x[None], valid, M, idx, np.array([dd], f32), np.array([3], np.uint32))
        assert not mass[0] and b[0, 0] == 0.5 and b.view(np.uint64)[0, 1] == ref.QNAN64
