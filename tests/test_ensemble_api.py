"""The ensemble entry points (include/vsom_hip.h, vsom_ensemble_*) are declared, exported and bound, and refuse to
run without a device -- no CPU fallback.  No compute: there is no GPU in this tier."""
import ctypes
import os
import re

import pytest

import vsom_amd
from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vsom_ensemble_create", "vsom_ensemble_destroy", "vsom_ensemble_size", "vsom_ensemble_train_online_chunk_fetch",
         "vsom_ensemble_batch_epoch"]


def test_declared_exported_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vsom_hip.h")).read(), flags=re.S)
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert hasattr(L, n), n
        assert n in capi.SYMBOLS, n
    assert vsom_amd.Ensemble is capi.Ensemble


def test_refusals_that_need_no_device():
    with pytest.raises(vsom_amd.VsomError, match="no members"):
        vsom_amd.Ensemble([])
    with pytest.raises(vsom_amd.VsomError, match="member 0: null context"):
        vsom_amd.Ensemble([None])


def test_no_cpu_path_without_a_device():
    """without a device there is nothing to train on: creating an ensemble raises (there are no contexts to give it), and
    the train calls raise rather than compute anything on the host"""
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(vsom_amd.VsomError):
        vsom_amd.Ensemble([vsom_amd.Context(10, 10, 9)])
    L = capi.lib()
    one = (ctypes.c_double * 1)(0.1)
    fn = (ctypes.c_int * 1)(capi.EXPONENTIAL)
    with pytest.raises(vsom_amd.VsomError, match="null ensemble"):
        capi.check(L.vsom_ensemble_train_online_chunk_fetch(None, one, one, fn, 1, None, None))
    with pytest.raises(vsom_amd.VsomError, match="null ensemble"):
        capi.check(L.vsom_ensemble_batch_epoch(None, one, 1, None))
