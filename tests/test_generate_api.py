"""vsom_generate_batch / vsom_decode_nodes without a GPU: the symbols are declared, exported and bound; the Python and C++
wrappers and the host driver exist; the Python wrappers check their arguments before reaching the library; the C calls
refuse a null context; the float64 restatement the GPU tests use holds the reference's exact cases."""
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
import generate_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert re.search(r"int\s+vsom_generate_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+min_hits\s*,\s*int\s+rule\s*,"
                     r"\s*size_t\s+r0\s*,\s*size_t\s+r1\s*,\s*const\s+double\s*\*\s*u_host\s*,"
                     r"\s*const\s+double\s*\*\s*l_host\s*,\s*vsom_generate_out\s*\*\s*out\s*\)", txt)
    assert re.search(r"int\s+vsom_decode_nodes\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*const\s+uint64_t\s*\*\s*nodes_host\s*,"
                     r"\s*size_t\s+count\s*,\s*const\s+double\s*\*\s*l_host\s*,\s*double\s*\*\s*record_out\s*\)", txt)
    assert re.search(r"typedef\s+struct\s+vsom_generate_out\s*\{\s*uint64_t\s*\*\s*unit\s*;\s*double\s*\*\s*record\s*;\s*\}"
                     r"\s*vsom_generate_out\s*;", txt)
    assert re.search(r"VSOM_GENERATE_AS_WRITTEN\s*=\s*0\s*,", txt) and re.search(r"VSOM_GENERATE_PER_ROW\s*=\s*1\b", txt)
    assert "vsom_generate_batch" in capi.SYMBOLS and "vsom_decode_nodes" in capi.SYMBOLS
    assert (capi.GENERATE_AS_WRITTEN, capi.GENERATE_PER_ROW) == (0, 1)
    L = _lib()
    raw = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(raw, "vsom_generate_batch") and hasattr(raw, "vsom_decode_nodes")
    assert len(L.vsom_generate_batch.argtypes) == 8
    assert len(L.vsom_decode_nodes.argtypes) == 5
    assert [f[0] for f in capi.GenerateOut._fields_] == ["unit", "record"]
    assert ctypes.sizeof(capi.GenerateOut) == 2 * ctypes.sizeof(ctypes.c_void_p)


def test_wrappers_exist():
    for name in ("generate", "decode_nodes"):
        assert callable(getattr(capi.Context, name, None)), name
    for name in ("generateRows", "decodeUnits", "autoEncoder"):
        assert callable(getattr(vs.Som, name, None)), name
    hpp = open(os.path.join(HOST, "include", "vsom_api.hpp")).read()
    assert re.search(r"struct\s+GeneratedRows\s*\{[^}]*std::vector<uint64_t>\s+unit\s*;[^}]*std::vector<double>\s+record\s*;"
                     r"[^}]*size_t\s+columns\b[^}]*\}\s*;", hpp)
    assert re.search(r"GeneratedRows\s+generateRows\s*\(\s*const\s+DataSet\s*&\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+std::vector<double>\s*&\s*\w+\s*,\s*const\s+std::vector<double>\s*&\s*\w+\s*,"
                     r"\s*bool\s+\w+[^)]*\)\s*const\s*;", hpp)
    assert re.search(r"std::vector<double>\s+decodeUnits\s*\(\s*const\s+std::vector<uint64_t>\s*&\s*\w+\s*,"
                     r"\s*const\s+std::vector<double>\s*&\s*\w+\s*\)\s*const\s*;", hpp)
    assert "host_generate_test" in open(os.path.join(HOST, "build.sh")).read()
    assert os.path.exists(os.path.join(HOST, "tests", "host_generate_test.cpp"))
    cpp = open(os.path.join(HOST, "src", "vsom_host.cpp")).read()
    assert "vsom_generate_batch" in cpp and "vsom_decode_nodes" in cpp


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, rows of 7 values, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100
        self.in_len = 7
        self.depth = 7


def _no_lib(monkeypatch):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)


@pytest.mark.parametrize("kw", [dict(u=np.zeros(9)), dict(u=np.zeros(11)), dict(u=np.zeros((10, 1))),
                                dict(u=np.full(10, 1.0)), dict(u=np.full(10, -0.1)), dict(u=np.full(10, np.nan)),
                                dict(l=np.full((10, 6), 0.5)), dict(l=np.full((9, 7), 0.5)), dict(l=np.full(70, 0.5)),
                                dict(rule=2), dict(rule=-1), dict(min_hits=-1),
                                dict(r0=2, r1=5), dict(r0=5, r1=4), dict(r1=11), dict(r0=-1, r1=9)])
def test_generate_refuses_before_the_library(monkeypatch, kw):
    _no_lib(monkeypatch)
    args = dict(min_hits=0, u=np.zeros(10), l=np.full((10, 7), 0.5))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().generate(**args)


@pytest.mark.parametrize("kw", [dict(nodes=[100, 0, 1]), dict(nodes=[-1, 0, 1]), dict(nodes=[0.5, 0, 1]),
                                dict(nodes=[[0, 1, 2]]), dict(l=np.full((2, 7), 0.5)), dict(l=np.full((3, 8), 0.5)),
                                dict(l=np.full(21, 0.5))])
def test_decode_nodes_refuses_before_the_library(monkeypatch, kw):
    _no_lib(monkeypatch)
    args = dict(nodes=[0, 1, 99], l=np.full((3, 7), 0.5))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().decode_nodes(**args)


def test_no_columns_refused_before_the_library(monkeypatch):
    _no_lib(monkeypatch)
    s = _Stub()
    s.depth = 0                                        # CLR of one column: J (J - 1) = 0
    with pytest.raises(ValueError):
        s.generate(0, np.zeros(10), np.zeros((10, 0)))
    with pytest.raises(ValueError):
        s.decode_nodes([0], np.zeros((1, 0)))


def test_null_context_refused():
    L = _lib()
    out = capi.GenerateOut()
    a = np.full(7, 0.5)
    p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    nodes = np.zeros(1, np.uint64)
    for rc in (L.vsom_generate_batch(None, 0, capi.GENERATE_PER_ROW, 0, 1, p, p, ctypes.byref(out)),
               L.vsom_decode_nodes(None, nodes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), 1, p, p)):
        assert rc == -1                                # VSOM_ERR_INVALID
        with pytest.raises(vsom_amd.VsomError, match="null context"):
            capi.check(rc)


# ---- the restatement the GPU tests hold the device to ----------------------------------------------------------------------
def _state():
    rng = np.random.default_rng(3)
    M = rng.uniform(-2, 2, (6, 5)).astype(np.float32)
    S = rng.uniform(0.1, 1, (6, 5)).astype(np.float32)
    return M, S


def test_reference_exact_cases():
    M, S = _state()
    units = np.array([4, 1, 5], np.uint64)
    # L = 0.5: q = 1, g = +0, the record is m
    rec, zs = ref.decode(M, S, units, np.full((3, 5), 0.5))
    assert ref.beq(rec, M[units.astype(int)].astype(np.float64)) and (zs == 0).all() and not np.signbit(zs).any()
    # s = 0 with a finite g: the record is m
    S0 = S.copy()
    S0[1] = 0
    L = np.random.default_rng(1).uniform(0.01, 0.99, (3, 5))
    rec, _ = ref.decode(M, S0, units, L)
    assert ref.beq(rec[1], M[1].astype(np.float64)) and not ref.beq(rec[0], M[4].astype(np.float64))
    # IEEE ends: L = 0 -> -inf, L = 1 -> +inf, outside [0, 1] -> NaN; s = 0 beside an infinite g -> NaN
    L = np.array([[0.0, 1.0, -0.25, 1.5, 0.25]] * 3)
    rec, _ = ref.decode(M, S0, units, L)
    assert rec[0, 0] == -np.inf and rec[0, 1] == np.inf and np.isnan(rec[0, 2:4]).all() and np.isfinite(rec[0, 4])
    assert np.isnan(rec[1, :4]).all() and rec[1, 4] == np.float64(M[1, 4])
    # no mass: the quiet NaN, bit for bit
    rec, _ = ref.decode(M, S, np.array([ref.NO_UNIT, 2], np.uint64), np.full((2, 5), 0.3))
    assert (rec[0].view(np.uint64) == ref.QNAN_BITS).all() and np.isfinite(rec[1]).all()
    # C below the depth: the first columns
    rec, _ = ref.decode(M, S, units, np.full((3, 2), 0.5))
    assert ref.beq(rec, M[units.astype(int), :2].astype(np.float64))


def test_reference_draw_and_bound():
    hits = np.array([0, 2, 2, 0, 5, 1], np.uint64)
    p = ref.bmd_p(np.float32([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]), hits, 2)
    assert (p[[0, 3, 5]] == 0).all() and (p[[1, 2, 4]] > 0).all()
    assert ref.draw(p, 0.0) == 1 and ref.draw(p, np.nextafter(1.0, 0.0)) == 4
    assert ref.draw(np.zeros(6), 0.3) == ref.NO_UNIT and ref.draw(ref.bmd_p(np.float32([1e3] * 6), hits, 0), 0.3) == ref.NO_UNIT
    assert ref.draw(np.array([1.0, np.nan]), 0.3) == ref.NO_UNIT
    # the bound: one ulp of a record value and four of z s
    assert ref.bound(np.float64(1.0), np.float64(0.0)) == 2.0 ** -52
    assert ref.bound(np.float64(0.0), np.float64(-1.0)) == 4 * 2.0 ** -52
    ok, worst = ref.within(np.array([1.0 + 2.0 ** -52]), np.array([1.0]), np.array([0.0]))
    assert ok and worst == 1.0
    ok, _ = ref.within(np.array([1.0 + 2.0 ** -51]), np.array([1.0]), np.array([0.0]))
    assert not ok
    ok, _ = ref.within(np.array([np.inf]), np.array([-np.inf]), np.array([-np.inf]))
    assert not ok
