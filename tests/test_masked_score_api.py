"""vsom_similarity_masked_batch / vsom_evaluate_masked_batch without a GPU: both symbols are declared, exported and bound,
the out structs have the layout of the header, the Python wrappers exist and check their arguments before reaching the
library, the C calls refuse a null context; and the reference helper of the GPU tests (tests/masked_score_ref.py) is
checked against the reference's literal double loop (similarity_ref.literal_loop) on engineered delta matrices with invalid
columns, and against plain sums for the evaluate select."""
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
import masked_score_ref as ref  # noqa: E402
import similarity_ref as sr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SIM_FIELDS = ["bmu", "dist", "dmax", "dmax_col", "first", "amax", "amax_col", "outside", "delta", "nvalid"]
EV_FIELDS = ["bmu", "dist", "bsum", "nrepl", "error", "nvalid"]


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def _header():
    return open(os.path.join(ROOT, "include", "vsom_hip.h")).read()


def _struct_fields(txt, name):
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", txt, flags=re.S).group(1)
    return [(re.sub(r"\s+", " ", t.strip()), n) for t, n in re.findall(r"([a-z0-9_ ]+?)\s*\*\s*([a-z_]+)\s*;", body)]


def test_declared_exported_bound():
    txt = _header()
    assert re.search(r"int\s+vsom_similarity_masked_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+min_hits\s*,\s*int\s+num_sigmas"
                     r"\s*,\s*int\s+sigma_rule\s*,\s*size_t\s+r0\s*,\s*size_t\s+r1\s*,\s*const\s+uint8_t\s*\*\s*valid_host"
                     r"\s*,\s*int\s+one_mask\s*,\s*vsom_similarity_masked_out\s*\*\s*out\s*\)", txt)
    assert re.search(r"int\s+vsom_evaluate_masked_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+min_hits\s*,\s*size_t\s+r0\s*,"
                     r"\s*size_t\s+r1\s*,\s*const\s+float\s*\*\s*binary_host\s*,\s*const\s+float\s*\*\s*continuous_host\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*valid_host\s*,\s*int\s+one_mask\s*,\s*vsom_evaluate_masked_out\s*\*\s*out\s*\)", txt)
    L = _lib()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name, nargs in (("vsom_similarity_masked_batch", 9), ("vsom_evaluate_masked_batch", 9)):
        assert name in capi.SYMBOLS
        assert hasattr(raw, name)
        assert len(getattr(L, name).argtypes) == nargs


def test_struct_layouts():
    txt = _header()
    sim = _struct_fields(txt, "vsom_similarity_masked_out")
    assert [n for _, n in sim] == SIM_FIELDS == [f[0] for f in capi.SimilarityMaskedOut._fields_]
    assert sim[:9] == _struct_fields(txt, "vsom_similarity_out")       # the unmasked struct's fields, then nvalid
    assert sim[9] == ("uint32_t", "nvalid")
    ev = _struct_fields(txt, "vsom_evaluate_masked_out")
    assert [n for _, n in ev] == EV_FIELDS == [f[0] for f in capi.EvaluateMaskedOut._fields_]
    assert ev[:5] == _struct_fields(txt, "vsom_evaluate_out")
    assert ev[4] == ("double", "error") and ev[5] == ("uint32_t", "nvalid")
    ptr = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(capi.SimilarityMaskedOut) == 10 * ptr and ctypes.sizeof(capi.EvaluateMaskedOut) == 6 * ptr
    ctype_of = {"uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    for fields, cls in ((sim, capi.SimilarityMaskedOut), (ev, capi.EvaluateMaskedOut)):
        for (ctype, name), (pyname, pytype) in zip(fields, cls._fields_):
            assert pytype._type_ is ctype_of[ctype], name
            assert getattr(cls, name).offset == fields.index((ctype, name)) * ptr
    # the existing structs are as they were: existing callers size them
    assert ctypes.sizeof(capi.SimilarityOut) == 9 * ptr and ctypes.sizeof(capi.EvaluateOut) == 5 * ptr


def test_wrappers_exist_and_no_new_timing_group():
    for name in ("similarity_masked", "evaluate_masked"):
        assert callable(getattr(capi.Context, name, None)), name
    for name in ("similarityRowsMasked", "measureSimilarityMasked", "evaluateRowsMasked", "evaluateMasked"):
        assert callable(getattr(vs.Som, name, None)), name
    assert len(capi.TIMER_NAMES) == 7                  # VSOM_T_COUNT stays 7: search under "bmu", scoring under "finish"
    assert re.search(r"VSOM_T_COUNT\s*=\s*7\b", _header())
    api = open(os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "include", "vsom_api.hpp")).read()
    for name in ("similarityRowsMasked", "measureSimilarityMasked", "evaluateRowsMasked", "evaluateMasked"):
        assert re.search(r"\b" + name + r"\s*\(", api), name


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


@pytest.mark.parametrize("kw", [dict(r0=5, r1=4), dict(r1=11), dict(r0=-1, r1=3), dict(sigma_rule=2), dict(min_hits=-1),
                                dict(num_sigmas=2 ** 31), dict(valid=np.ones((10, 6))), dict(valid=np.ones((9, 7))),
                                dict(valid=np.ones(6)), dict(r0=2, r1=5, valid=np.ones((10, 7))), dict(valid=np.ones((1, 10, 7)))])
def test_similarity_wrapper_refuses_before_the_library(monkeypatch, kw):
    monkeypatch.setattr(capi, "lib", _no_lib)
    args = dict(valid=np.ones((10, 7)), min_hits=1, num_sigmas=3)
    args.update(kw)
    if "valid" not in kw and ("r0" in kw or "r1" in kw):
        args["valid"] = np.ones(7)
    with pytest.raises(ValueError):
        _Stub().similarity_masked(**args)


@pytest.mark.parametrize("kw", [dict(r0=5, r1=4), dict(r1=11), dict(min_hits=-1), dict(valid=np.ones((10, 6))),
                                dict(valid=np.ones(8)), dict(binary=np.zeros(6)), dict(continuous=np.ones((7, 1))),
                                dict(r0=2, r1=5, valid=np.ones((10, 7)))])
def test_evaluate_wrapper_refuses_before_the_library(monkeypatch, kw):
    monkeypatch.setattr(capi, "lib", _no_lib)
    args = dict(valid=np.ones(7), binary=np.zeros(7), continuous=np.ones(7))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().evaluate_masked(**args)


def test_null_context_refused():
    L = _lib()
    v = np.ones(3, np.uint8)
    vp = v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    rc = L.vsom_similarity_masked_batch(None, 1, 3, 0, 0, 1, vp, 1, ctypes.byref(capi.SimilarityMaskedOut()))
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)
    b = np.zeros(3, np.float32)
    rc = L.vsom_evaluate_masked_batch(None, 0, 0, 1, capi._f(b), capi._f(b), vp, 1, ctypes.byref(capi.EvaluateMaskedOut()))
    assert rc == -1
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


# ---- the reference helper: similarity ---------------------------------------------------------------------------------------
def _check_similarity(X, m, s, valid, num_sigmas=3, floor=True):
    """the helper's rows, finished by measure_similarity_from_rows, against the literal loop over the masked delta"""
    X, m, s = (np.ascontiguousarray(a, f32) for a in (X, m, s))
    valid = np.asarray(valid, bool)
    delta, lo, hi = sr.columns(X, m, s, num_sigmas, floor)
    rep = ref.similarity(X, m, s, num_sigmas, floor, valid)
    md = ref.masked_delta(delta, valid)
    row, ok = vs.measure_similarity_from_rows(rep["first"], rep["dmax"], rep["outside"])
    want_row, want_ok = sr.literal_loop(md, X, lo, hi, valid)
    assert row == want_row, (row, want_row)
    assert ok == want_ok
    # nothing of an invalid column is reported
    for r in range(X.shape[0]):
        for k in ("dmax_col", "amax_col"):
            c = rep[k][r]
            assert c == sr.NONE or valid[r, c], (k, r)
        assert (rep["delta"][r][~valid[r]] == 0).all()
        if not valid[r].any():
            assert rep["dmax"][r] == -np.inf and rep["dmax_col"][r] == sr.NONE and np.isnan(rep["first"][r])
            assert rep["amax"][r] == 0 and rep["amax_col"][r] == sr.NONE and rep["outside"][r] == 0
    return rep


def test_similarity_helper_on_engineered_matrices():
    m = np.zeros((4, 4), f32)
    s = np.full((4, 4), 1.0 / 3.0, f32)                # sM k = 1 (to a rounding): delta ~ x
    X = np.array([[-1000.0, 3.0, 5.0, 1.0], [7.0, 900.0, 1001.0, 2.0], [2000.0, 2.0, 3.0, 0.5], [0.1, 0.2, 0.3, 0.4]], f32)
    allv = np.ones((4, 4), bool)
    base = _check_similarity(X, m, s, allv)
    # the largest delta of the matrix invalid: the reported row moves, and that row's dmax is its next valid column
    v = allv.copy()
    v[2, 0] = False
    rep = _check_similarity(X, m, s, v)
    assert base["dmax_col"][2] == 0 and rep["dmax_col"][2] == 2 and rep["dmax"][2] == rep["delta"][2, 2]
    # an invalid lowest column: first skips it
    v = allv.copy()
    v[0, 0] = False
    rep = _check_similarity(X, m, s, v)
    assert rep["first"][0] == rep["delta"][0, 1] and base["first"][0] == base["delta"][0, 0]
    # a row without a valid column, the first row among them; and a matrix without any
    v = allv.copy()
    v[0] = False
    v[3] = False
    _check_similarity(X, m, s, v)
    _check_similarity(X, m, s, np.zeros((4, 4), bool))
    # poison at invalid positions of the row and of the model / sigma rows
    Xp, mp, sp = X.copy(), m.copy(), s.copy()
    v = allv.copy()
    for r, c, px in ((0, 1, np.nan), (1, 2, np.inf), (2, 0, 1e30), (3, 3, -np.inf)):
        v[r, c] = False
        Xp[r, c] = px
        mp[r, c] = np.nan
        sp[r, c] = np.nan
    rep = _check_similarity(Xp, mp, sp, v)
    clean = _check_similarity(np.where(v, Xp, 0), np.where(v, mp, 0), np.where(v, sp, 1), v)
    for k in rep:
        assert sr.beq(rep[k], clean[k]), k
    # a tie for amax between a valid and an invalid column resolves to the valid one; as written (a cap) as well
    Xt = np.array([[2.0, -2.0, 2.0, 1.0]], f32)
    vt = np.array([[False, True, True, True]])
    for floor in (True, False):
        rep = _check_similarity(Xt, m[:1], s[:1], vt, floor=floor)
        assert rep["amax_col"][0] == 1 and rep["dmax_col"][0] == 2
        assert _check_similarity(Xt, m[:1], s[:1], np.ones((1, 4), bool), floor=floor)["amax_col"][0] == 0


def test_similarity_helper_on_random_matrices():
    rng = np.random.default_rng(20261020)
    specials = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 0.0, -0.0], f32)
    for _ in range(400):
        n, C = int(rng.integers(1, 7)), int(rng.integers(1, 8))
        X = (rng.standard_normal((n, C)) * 10.0 ** rng.integers(-2, 4)).astype(f32)
        m = rng.standard_normal((n, C)).astype(f32)
        s = np.abs(rng.standard_normal((n, C))).astype(f32) * f32(10.0 ** rng.integers(-7, 1))
        for a in (X, m, s):
            mask = rng.random((n, C)) < rng.choice([0.0, 0.1, 0.4])
            a[mask] = rng.choice(specials, size=int(mask.sum()))
        valid = rng.random((n, C)) < rng.choice([0.0, 0.3, 0.7, 1.0])
        _check_similarity(X, m, s, valid, num_sigmas=int(rng.choice([1, 3, 1000000])), floor=bool(rng.integers(0, 2)))


# ---- the reference helper: search and evaluate ------------------------------------------------------------------------------
def test_search_helper_is_the_oracle_on_all_valid_rows_and_ignores_invalid_positions():
    rng = np.random.default_rng(5)
    W, H, J = 5, 4, 9
    M = rng.standard_normal((W * H, J)).astype(f32)
    X = rng.standard_normal((12, J)).astype(f32)
    hits = rng.integers(0, 5, W * H).astype(np.uint64)
    o = po.OracleSom(W, H, J)
    o.set_state(map=M, hits=hits)
    for min_hits in (0, 3):
        bmu, dist = ref.checker(po.STANDARD, X, M, np.ones(J, bool), hits, min_hits)
        assert (bmu == np.array([o.find_restricted_bmu(x, min_hits) for x in X], np.uint64)).all()
        assert sr.beq(dist, np.array([o.dist(int(b), x) for b, x in zip(bmu, X)], f32))
    valid = rng.random((12, J)) < 0.6
    valid[4] = False
    Xp = np.where(valid, X, f32(np.nan))
    a = ref.checker(po.STANDARD, X, M, valid, hits, 0)
    b = ref.checker(po.STANDARD, Xp, M, valid, hits, 0)
    assert (a[0] == b[0]).all() and sr.beq(a[1], b[1])
    assert a[0][4] == 0 and a[1][4].view(np.uint32) == 0       # no valid column: node 0, distance +0


def test_evaluate_helper_select():
    rng = np.random.default_rng(6)
    n, C = 9, 13
    X = rng.random((n, C)).astype(f32)
    M = rng.uniform(0.05, 0.95, (n, C)).astype(f32)
    binary = (rng.random(C) < 0.6).astype(f32)
    binary[0] = 1
    continuous = np.ones(C, f32)
    valid = rng.random((n, C)) < 0.7
    valid[2] = False
    b32, n32, exact, t = ref.evaluate32(X, M, binary, continuous, valid)
    b64, n64 = ref.evaluate64(X, M, binary, continuous, valid)
    assert (t[~valid] == 0).all() and not np.signbit(t[~valid]).any()
    assert b32[2] == 0 and b64[2] == 0 and (n32 == n64).all()
    nz = b64 != 0
    assert nz.any() and (np.abs(b32[nz] - b64[nz]) / b64[nz] <= ref.bound(C)).all()
    # the literal sum over the valid columns only, in float64
    for r in range(n):
        want = 0.0
        for d in np.flatnonzero(valid[r]):
            x, m = float(X[r, d]), float(M[r, d])
            be = np.log(m) * x + np.log(float(f32(1) - M[r, d])) * float(f32(1) - X[r, d])
            want += (be * float(binary[d]) * float(continuous[d])) ** 2
        assert abs(b64[r] - want) <= 1e-12 * max(1.0, want)
    # what the invalid positions hold does not matter, nor does a factor whose fp32 product overflows there
    Xp = np.where(valid, X, f32(np.nan))
    Mp = np.where(valid, M, f32(7.0))
    p32 = ref.evaluate32(Xp, Mp, binary, continuous, valid)
    assert sr.beq(p32[0], b32) and (p32[1] == n32).all()
    big = binary.copy()
    big[3] = f32(1e35)                                 # -99999 * 1e35 overflows in fp32: (inf * 0) would be NaN
    v3 = valid.copy()
    v3[:, 3] = False
    g32, gn, _, _ = ref.evaluate32(Xp, Mp, big, continuous, v3)
    h32, hn, _, _ = ref.evaluate32(X, M, binary, continuous, v3)
    assert np.isfinite(g32).all() and sr.beq(g32, h32) and (gn == hn).all()
    # replaced terms count only at valid columns
    M0 = M.copy()
    M0[:, 0] = 0
    X0 = X.copy()
    X0[:, 0] = 0                                       # log(0) * 0 = NaN -> -99999
    r32, rn, _, _ = ref.evaluate32(X0, M0, binary, continuous, valid)
    assert (rn == valid[:, 0].astype(np.uint32) + n32).all()
