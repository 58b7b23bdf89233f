"""vsom_umatrix / vsom_get_umatrix / vsom_ensemble_umatrix without a GPU: the prototypes are declared, exported and
bound; the Python wrappers exist and check the map's shape before reaching the library; the C calls refuse a null
context or ensemble.  No compute: there is no GPU in this tier."""
import ctypes
import os
import re

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOS = {
    "vsom_umatrix": r"int\s+vsom_umatrix\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*u_out_host\s*\)",
    "vsom_get_umatrix": r"int\s+vsom_get_umatrix\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*double\s*\*\s*u_out_host\s*\)",
    "vsom_ensemble_umatrix": r"int\s+vsom_ensemble_umatrix\s*\(\s*vsom_ensemble\s*\*\s*e\s*,\s*double\s*\*\s*const\s*\*\s*u_out\s*\)",
}


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vsom_hip.h")).read(), flags=re.S)
    L = _lib()
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name, proto in PROTOS.items():
        assert re.search(proto, txt), name
        assert name in capi.SYMBOLS, name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 2, name
    assert re.search(r"VSOM_BUF_UMATRIX\s*=\s*8\b", txt)
    assert capi.BUF_UMATRIX == 8
    assert re.search(r"VSOM_T_COUNT\s*=\s*7\b", txt) and capi.T_COUNT == 7      # callers size arrays by it


def test_wrappers_exist():
    for cls, names in ((capi.Context, ("umatrix", "get_umatrix")), (capi.Ensemble, ("umatrix",)),
                       (vs.Som, ("updateUMatrix", "getUMatrix"))):
        for n in names:
            assert callable(getattr(cls, n, None)), (cls.__name__, n)


def test_null_handles_refused():
    L = _lib()
    u = np.zeros(4, np.float64)
    up = u.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    for call, what in ((lambda: L.vsom_umatrix(None, up), "null context"),
                       (lambda: L.vsom_umatrix(None, None), "null context"),
                       (lambda: L.vsom_get_umatrix(None, up), "null context"),
                       (lambda: L.vsom_ensemble_umatrix(None, None), "null ensemble")):
        rc = call()
        assert rc == -1                                    # VSOM_ERR_INVALID
        with pytest.raises(vsom_amd.VsomError, match=what):
            capi.check(rc)


class _Stub(capi.Context):
    """a context that never reached the library"""

    def __init__(self, width, height):
        self._h = None
        self._owned = False
        self.width, self.height = width, height
        self.n_nodes = width * height


@pytest.mark.parametrize("W, H", [(1, 1), (1, 5), (5, 1), (0, 3)])
def test_wrappers_refuse_degenerate_maps_before_the_library(monkeypatch, W, H):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    for call in (lambda s: s.umatrix(), lambda s: s.umatrix(fetch=False), lambda s: s.get_umatrix()):
        with pytest.raises(ValueError, match="width >= 2 and height >= 2"):
            call(_Stub(W, H))
    e = capi.Ensemble.__new__(capi.Ensemble)
    e.members = [_Stub(4, 4), _Stub(W, H)]
    e._h = ctypes.c_void_p()
    e._pinned = None
    with pytest.raises(ValueError, match="member 1"):
        e.umatrix()
