"""vsom_bmu_masked_batch without a GPU: the entry point and its struct are declared, exported and bound; the Python wrappers
exist and check their arguments before reaching the library; the C call refuses a null context; the custom kernel text
still compiles (vsom_custom_compile_check: the feature leaves it alone)."""
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
import custom_hooks as hooks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    return capi.lib()


def test_declared_exported_bound():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert re.search(r"int\s+vsom_bmu_masked_batch\s*\(\s*vsom_ctx\s*\*\s*ctx\s*,\s*uint64_t\s+min_hits\s*,\s*size_t\s+r0\s*,"
                     r"\s*size_t\s+r1\s*,\s*const\s+uint8_t\s*\*\s*valid_host\s*,\s*int\s+one_mask\s*,"
                     r"\s*vsom_masked_out\s*\*\s*out\s*\)", txt)
    assert re.search(r"typedef\s+struct\s+vsom_masked_out\s*\{\s*uint64_t\s*\*\s*bmu\s*;\s*float\s*\*\s*dist\s*;"
                     r"\s*uint32_t\s*\*\s*nvalid\s*;\s*float\s*\*\s*fill\s*;\s*\}\s*vsom_masked_out\s*;", txt)
    assert "vsom_bmu_masked_batch" in capi.SYMBOLS
    L = _lib()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "vsom_bmu_masked_batch")
    assert len(L.vsom_bmu_masked_batch.argtypes) == 7
    assert [f[0] for f in capi.MaskedOut._fields_] == ["bmu", "dist", "nvalid", "fill"]
    assert ctypes.sizeof(capi.MaskedOut) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_wrappers_exist():
    assert callable(getattr(capi.Context, "bmu_masked", None))
    for name in ("findBmuMasked", "impute", "classify"):
        assert callable(getattr(vs.Som, name, None)), name


def test_cpp_mirror_declares_the_calls():
    txt = open(os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "include", "vsom_api.hpp")).read()
    assert re.search(r"findMaskedBmus\s*\(\s*const\s+DataSet\s*\*\s*\w+\s*,\s*size_t\s+minBmuHits\s*,"
                     r"\s*std::vector<float>\s*\*\s*dist\s*=\s*nullptr\s*\)\s*const", txt)
    assert re.search(r"std::vector<float>\s+impute\s*\(\s*const\s+DataSet\s*\*\s*\w+\s*,\s*size_t\s+minBmuHits\s*\)\s*const", txt)


class _Stub(capi.Context):
    """a context that never reached the library: 100 nodes, rows of 7 values, a chunk of 10 rows"""
    chunk_size = 10

    def __init__(self):
        self._h = None
        self._owned = False
        self.n_nodes = 100
        self.in_len = 7
        self.depth = 7


@pytest.mark.parametrize("kw", [dict(r0=5, r1=4), dict(r1=11), dict(r0=-1, r1=3), dict(min_hits=-1),
                                dict(valid=np.ones((10, 6))), dict(valid=np.ones((9, 7))), dict(valid=np.ones(6)),
                                dict(valid=np.ones(8)), dict(r0=2, r1=5, valid=np.ones((10, 7))),
                                dict(valid=np.ones((10, 7, 1)))])
def test_wrapper_refuses_before_the_library(monkeypatch, kw):
    def no_lib():
        raise AssertionError("the wrapper reached the library")
    monkeypatch.setattr(capi, "lib", no_lib)
    args = dict(valid=np.ones((10, 7)))
    args.update(kw)
    with pytest.raises(ValueError):
        _Stub().bmu_masked(**args)


def test_null_context_refused():
    L = _lib()
    out = capi.MaskedOut()
    v = (ctypes.c_uint8 * 4)(1, 1, 1, 1)
    rc = L.vsom_bmu_masked_batch(None, 0, 0, 1, v, 1, ctypes.byref(out))
    assert rc == -1                                    # VSOM_ERR_INVALID
    with pytest.raises(vsom_amd.VsomError, match="null context"):
        capi.check(rc)


@pytest.mark.parametrize("kind", ["standard", "median", "clr"])
def test_custom_kernel_text_still_compiles(kind):
    depth, rlen = hooks.shape(kind, 9)
    L = _lib()
    assert L.vsom_custom_compile_check(hooks.SOURCES[kind].encode(), depth, rlen) == 0, L.vsom_last_error().decode()
