"""The ensemble upload and scoring entry points (include/vsom_hip.h, vsom_ensemble_upload_chunks /
vsom_ensemble_bmu_batch) are declared, exported and bound; the Python wrappers refuse malformed arguments before they
reach the library, and the C calls refuse without a device -- no CPU fallback.  No compute: there is no GPU in this tier."""
import ctypes
import os
import re

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vsom_ensemble_upload_chunks", "vsom_ensemble_bmu_batch"]


def test_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vsom_hip.h")).read(), flags=re.S)
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS, n
    B = capi.lib()
    assert B.vsom_ensemble_upload_chunks.argtypes is not None and len(B.vsom_ensemble_upload_chunks.argtypes) == 6
    assert B.vsom_ensemble_bmu_batch.argtypes is not None and len(B.vsom_ensemble_bmu_batch.argtypes) == 3
    for m in ("upload_chunks", "upload_chunks_async", "bmu_batch"):
        assert callable(getattr(vsom_amd.Ensemble, m)), m


class _Member:
    """what Ensemble's packing reads of a member: its row length"""

    def __init__(self, in_len):
        self.in_len = in_len


def _stub(in_lens):
    e = capi.Ensemble.__new__(capi.Ensemble)
    e.members = [_Member(j) for j in in_lens]
    e._h = ctypes.c_void_p()
    e._pinned = None
    return e


def test_python_refusals_that_need_no_device():
    e = _stub([9, 4])
    with pytest.raises(ValueError, match="1 chunks for 2 members"):
        e.upload_chunks([np.zeros((3, 9), np.float32)])
    with pytest.raises(ValueError, match="member 1"):
        e.upload_chunks([np.zeros((3, 9), np.float32), np.zeros((3, 5), np.float32)])
    with pytest.raises(ValueError, match="member 0"):
        e.upload_chunks(np.zeros(9, np.float32))             # one 1-D array: not rows
    with pytest.raises(ValueError, match="offsets"):
        e.upload_chunks_async(np.zeros(16, np.float32), [0], [1, 1])


def test_no_cpu_path_without_a_device():
    """the C calls refuse a null ensemble and null arrays rather than compute anything on the host"""
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    L = capi.lib()
    x = np.zeros(16, np.float32)
    off = (ctypes.c_size_t * 1)(0)
    b = (ctypes.c_size_t * 1)(1)
    with pytest.raises(vsom_amd.VsomError, match="null ensemble"):
        capi.check(L.vsom_ensemble_upload_chunks(None, capi._f(x), x.size, off, b, 1))
    with pytest.raises(vsom_amd.VsomError, match="null ensemble"):
        capi.check(L.vsom_ensemble_bmu_batch(None, None, None))
    with pytest.raises(vsom_amd.VsomError):
        vsom_amd.Ensemble([vsom_amd.Context(10, 10, 9)])
