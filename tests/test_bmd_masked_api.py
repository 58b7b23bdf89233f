"""vsom_bmd_masked_batch / vsom_generate_masked_batch without a GPU: both symbols are declared, exported and bound, the
existing out struct and timer names are as they were, the Python wrappers and the Som / C++ mirror methods exist, the wrappers
check their arguments before reaching the library, the C calls refuse a null context; and the reference helper of the GPU
tests (tests/bmd_masked_ref.py) is checked against the oracle's findRestrictedBmd, against poison at invalid positions, on the
row without a valid column and on the keep-observed select.  The draws the GPU tests compare are counted here, on the reference
alone: at most one per case may lie within relative 1e-12 of a cumulative boundary (the rule of tests/test_gpu_bmd_batch.py)."""
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
import bmd_masked_ref as ref  # noqa: E402
import generate_ref as gr  # noqa: E402
import masked_score_ref as msr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def _header():
    return open(os.path.join(ROOT, "include", "vsom_hip.h")).read()


def test_declared_exported_bound():
    txt = re.sub(r"\s+", " ", _header())
    for decl in ("int vsom_bmd_masked_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, const uint8_t *valid_host, "
                 "int one_mask, const double *u_host, uint64_t *draw_out, double *norm_out, double *prob_out);",
                 "int vsom_generate_masked_batch(vsom_ctx *ctx, uint64_t min_hits, size_t r0, size_t r1, "
                 "const uint8_t *valid_host, int one_mask, uint32_t draws, int keep_observed, const double *u_host, "
                 "const double *l_host, vsom_generate_out *out);"):
        squeezed = re.sub(r"\s*([(),*;])\s*", r"\1", decl)
        assert squeezed in re.sub(r"\s*([(),*;])\s*", r"\1", txt), decl
    L = _lib()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name, nargs in (("vsom_bmd_masked_batch", 10), ("vsom_generate_masked_batch", 11)):
        assert name in capi.SYMBOLS
        assert hasattr(raw, name)
        assert len(getattr(L, name).argtypes) == nargs


def test_existing_struct_and_timers_unchanged():
    txt = _header()
    assert re.search(r"typedef\s+struct\s+vsom_generate_out\s*\{\s*uint64_t\s*\*\s*unit\s*;\s*double\s*\*\s*record\s*;\s*\}", txt)
    assert [f[0] for f in capi.GenerateOut._fields_] == ["unit", "record"]
    assert ctypes.sizeof(capi.GenerateOut) == 2 * ctypes.sizeof(ctypes.c_void_p)
    assert capi.TIMER_NAMES == ["stage", "bmu", "finish", "cw", "update", "online", "sigma"]
    assert re.search(r"VSOM_T_COUNT\s*=\s*7\b", txt)


def test_wrappers_and_mirrors_exist():
    for name in ("restricted_bmd_masked", "generate_masked"):
        assert callable(getattr(capi.Context, name, None)), name
    for name in ("findRestrictedBmdMasked", "drawModelVectorsMasked", "generateRowsMasked", "imputeSampled"):
        assert callable(getattr(vs.Som, name, None)), name
    api = open(os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "include", "vsom_api.hpp")).read()
    for name in ("findRestrictedBmdMasked", "drawModelVectorsMasked", "generateRowsMasked"):
        assert re.search(r"\b" + name + r"\s*\(", api), name
    assert re.search(r"GeneratedRows\s+generateRowsMasked\s*\(", api)


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, rows of 7 values, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100
        self.in_len = 7
        self.depth = 7


def _no_lib():
    raise AssertionError("the wrapper reached the library")


@pytest.mark.parametrize("kw", [dict(r0=5, r1=4), dict(r1=11), dict(r0=-1, r1=3), dict(min_hits=-1),
                                dict(valid=np.ones((10, 6))), dict(valid=np.ones((9, 7))), dict(valid=np.ones(6)),
                                dict(r0=2, r1=5, valid=np.ones((10, 7))), dict(valid=np.ones((1, 10, 7))),
                                dict(u=np.full(9, 0.5)), dict(u=np.full((10, 2), 0.5)), dict(u=np.full(10, 1.0)),
                                dict(u=np.full(10, -0.25)), dict(u=np.full(10, np.nan))])
def test_bmd_wrapper_refuses_before_the_library(monkeypatch, kw):
    monkeypatch.setattr(capi, "lib", _no_lib)
    args = dict(valid=np.ones((10, 7)), min_hits=1, u=np.full(10, 0.5))
    args.update(kw)
    if "valid" not in kw and ("r0" in kw or "r1" in kw):
        args["valid"] = np.ones(7)
    with pytest.raises(ValueError):
        _Stub().restricted_bmd_masked(**args)


@pytest.mark.parametrize("kw", [dict(r0=5, r1=4), dict(r1=11), dict(min_hits=-1), dict(valid=np.ones((10, 6))),
                                dict(valid=np.ones(8)), dict(draws=0), dict(draws=65536), dict(draws=-1),
                                dict(draws=2), dict(draws=2, u=np.full((10, 2), 0.5)),
                                dict(draws=2, l=np.full((10, 2, 7), 0.5)), dict(u=np.full(10, 1.0)),
                                dict(u=np.full((10, 1), np.nan)), dict(l=np.full((10, 6), 0.5)), dict(l=np.full((9, 1, 7), 0.5)),
                                dict(r0=2, r1=5)])
def test_generate_wrapper_refuses_before_the_library(monkeypatch, kw):
    monkeypatch.setattr(capi, "lib", _no_lib)
    args = dict(valid=np.ones(7), min_hits=0, u=np.full(10, 0.5), l=np.full((10, 7), 0.5))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().generate_masked(**args)


def test_null_context_refused():
    L = _lib()
    v = np.ones(3, np.uint8)
    vp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    norm, u, l = np.zeros(1), np.full(1, 0.5), np.full(3, 0.5)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = L.vsom_bmd_masked_batch(None, 0, 0, 1, vp, 1, None, None, norm.ctypes.data_as(dp), None)
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)
    rc = L.vsom_generate_masked_batch(None, 0, 0, 1, vp, 1, 1, 1, u.ctypes.data_as(dp), l.ctypes.data_as(dp),
                                      ctypes.byref(capi.GenerateOut()))
    assert rc == -1
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


# ---- the reference helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", ref.KINDS)
def test_helper_on_an_all_valid_mask_is_the_oracle(tr):
    W, H, J = 9, 15, 37
    M, S, hits = ref.unit_state(W, H, J, 4)
    X = ref.unit_rows(6, J, 5)
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=M, hits=hits)
    d = ref.masked_d(tr, X, M, np.ones(J, bool))
    assert msr.beq(d, np.array([[o.dist(i, x) for i in range(W * H)] for x in X], f32))      # the distances: bit for bit
    for min_hits in ref.MIN_HITS:
        P, norm, prob = ref.distribution(d, hits, min_hits)
        for r in range(X.shape[0]):
            # (numpy's exp against the oracle's libm exp: the figure of tests/test_gpu_bmd_batch.py for the same quantity)
            want = o.find_restricted_bmd(X[r], min_hits)
            assert np.allclose(prob[r], want, rtol=1e-15, atol=0), (min_hits, r, np.abs(prob[r] - want).max())
            assert ((prob[r] == 0) == (want == 0)).all() and ((prob[r] == 0) == (hits < np.uint64(min_hits))).all()
        assert (norm > 0).all()


def test_poison_at_invalid_positions_changes_nothing():
    tr, W, H, J = po.STANDARD, 7, 5, 9
    M, S, hits = ref.unit_state(W, H, J, 6)
    X = ref.unit_rows(12, J, 7)
    valid = np.random.default_rng(8).random((12, J)) < 0.6
    colmask = np.random.default_rng(9).random(J) < 0.6
    base = ref.masked_d(tr, X, M, valid)
    base1 = ref.masked_d(tr, X, M, colmask)
    for junk in (f32(np.nan), f32(np.inf), f32(-np.inf), f32(1e30)):
        Xp = np.where(valid, X, junk).astype(f32)
        assert msr.beq(ref.masked_d(tr, Xp, M, valid), base), junk
        Xq = np.where(colmask, X, junk).astype(f32)
        Mq = np.where(colmask, M, junk).astype(f32)            # model rows too, where every row is invalid
        assert msr.beq(ref.masked_d(tr, Xq, Mq, colmask), base1), junk
    assert np.isfinite(base).all() and np.isfinite(base1).all()


def test_row_without_a_valid_column_is_uniform():
    tr, W, H, J = po.STANDARD, 7, 5, 9
    M, S, hits = ref.unit_state(W, H, J, 10)
    X = np.full((1, J), np.nan, f32)
    d = ref.masked_d(tr, X, M, np.zeros(J, bool))
    assert (d == 0).all() and not np.signbit(d).any()
    for min_hits in (0, 1, 3, 6):
        P, norm, prob = ref.distribution(d, hits, min_hits)
        ok = np.flatnonzero(hits >= np.uint64(min_hits))
        if ok.size == 0:
            assert norm[0] == 0 and gr.draw(P[0], 0.5) == ref.NO_UNIT
            continue
        assert norm[0] == ok.size
        assert (prob[0][ok] == 1.0 / ok.size).all() and (np.delete(prob[0], ok) == 0).all()
        for u in (0.0, 0.25, 0.5, 0.999, np.nextafter(1.0, 0.0)):
            k = int(np.floor(u * ok.size))      # (u * count may round up to count: the last node then)
            assert gr.draw(P[0], u) == ok[min(k, ok.size - 1)]


def test_keep_observed_select():
    M = np.array([[0.25, 0.5, 0.75], [0.1, 0.2, 0.3]], f32)
    S = np.array([[0.5, 0.0, 0.25], [1.0, 1.0, 1.0]], f32)
    X = np.array([[9.0, np.nan, 7.0], [np.nan, 5.0, np.nan]], f32)
    valid = np.array([[1, 0, 1], [0, 1, 0]], bool)
    unit = np.array([[0, 1], [1, ref.NO_UNIT]], np.uint64)
    L = np.full((2, 2, 3), 0.5)
    L[0, 0, 0] = np.nan                       # at a kept column: no effect
    L[0, 1, 1] = 0.75
    rec, zs, kept = ref.records(M, S, unit, L, X, valid, True)
    assert kept.tolist() == [[[True, False, True]] * 2, [[False, True, False], [False, False, False]]]
    assert rec[0, 0].tolist() == [9.0, 0.5, 7.0]                         # L = 0.5: the unit's mean, exactly
    assert rec[0, 1, 0] == 9.0 and rec[0, 1, 2] == 7.0
    assert rec[0, 1, 1] == np.log(0.75 / 0.25) / 1.6 * 1.0 + np.float64(f32(0.2))
    assert rec[1, 0].tolist() == [np.float64(f32(0.1)), 5.0, np.float64(f32(0.3))]
    assert (rec[1, 1].view(np.uint64) == ref.QNAN_BITS).all()            # no mass: NaN throughout, the observed column too
    assert (zs[kept] == 0).all()
    # nothing kept: the plain decode, NaN where L is NaN
    plain, _, none = ref.records(M, S, unit, L, X, valid, False)
    assert not none.any() and np.isnan(plain[0, 0, 0]) and plain[0, 0, 1] == 0.5
    assert gr.beq(plain.reshape(4, 3), gr.decode(M, S, unit.reshape(-1), L.reshape(4, 3))[0])


# ---- the draws the GPU tests compare ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_gpu_draws_keep_clear_of_the_boundaries(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    assert not c["valid"][ref.NO_VALID_ROW].any() and np.isnan(c["X"][~c["valid"]]).all()
    assert 0.6 < c["valid"].mean() < 0.8
    for min_hits in ref.MIN_HITS:
        P, norm, prob, unit, nr = ref.case_draws(c, min_hits)
        assert (norm > 0).all() and np.isfinite(norm).all()              # every row has mass
        assert (unit != ref.NO_UNIT).all()
        assert int((nr <= ref.NEAR).sum()) <= ref.NEAR_CAP, (min_hits, int((nr <= ref.NEAR).sum()))
        count = int((c["hits"] >= np.uint64(min_hits)).sum())
        assert norm[ref.NO_VALID_ROW] == count                           # the row without a valid column: p = 1 each
