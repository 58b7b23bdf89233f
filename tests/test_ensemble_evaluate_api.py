"""CPU tier of the ensemble's evaluate calls (vsom_ensemble_evaluate_batch, vsom_ensemble_evaluate_masked_batch,
vsom_ensemble_evaluate_applies): the symbols are declared, listed and exported, the ctypes signatures
are bound over the single calls' structures, and Ensemble.evaluate / evaluate_masked / validation_errors refuse wrong
arguments before any call into the library (stub contexts: no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsom_ensemble_evaluate_batch", "vsom_ensemble_evaluate_masked_batch", "vsom_ensemble_evaluate_applies")


def header():
    return open(os.path.join(ROOT, "include", "vsom_hip.h")).read()


def test_new_symbols_declared_listed_and_exported():
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    declared = set(re.findall(r"\b(vsom_[a-z0-9_]+)\s*\(", txt))
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in capi.SYMBOLS, name
        assert hasattr(L, name), name
    for name in ("evaluate", "evaluate_masked", "evaluate_applies", "validation_errors"):
        assert callable(getattr(capi.Ensemble, name)), name


def test_signatures_are_bound_over_the_single_calls_structures():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = capi.lib()
    fpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_float))
    u8pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))
    assert L.vsom_ensemble_evaluate_batch.argtypes == [ctypes.c_void_p, fpp, fpp, u8pp, ctypes.POINTER(capi.EvaluateOut)]
    assert L.vsom_ensemble_evaluate_masked_batch.argtypes == [
        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), fpp, fpp, u8pp, ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(capi.EvaluateMaskedOut)]
    assert L.vsom_ensemble_evaluate_applies.argtypes == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    # the header's prototypes take the single calls' structures, one per member
    txt = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    plain = re.search(r"int\s+vsom_ensemble_evaluate_batch\s*\((.*?)\)\s*;", txt, re.S).group(1)
    masked = re.search(r"int\s+vsom_ensemble_evaluate_masked_batch\s*\((.*?)\)\s*;", txt, re.S).group(1)
    assert "const vsom_evaluate_out *out" in plain and plain.count("const float *const *") == 2
    assert "const vsom_evaluate_masked_out *out" in masked and "const uint64_t *min_hits" in masked
    assert [n for n, _ in capi.EvaluateMaskedOut._fields_] == ["bmu", "dist", "bsum", "nrepl", "error", "nvalid"]


def test_null_arguments_are_refused_without_a_device():
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    L = capi.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    cols = (fp * 1)()
    vp = (ctypes.POINTER(ctypes.c_uint8) * 1)()
    assert L.vsom_ensemble_evaluate_batch(None, cols, cols, None, (capi.EvaluateOut * 1)()) == -1
    assert b"null ensemble" in L.vsom_last_error()
    assert L.vsom_ensemble_evaluate_masked_batch(None, None, cols, cols, vp, None, (capi.EvaluateMaskedOut * 1)()) == -1
    assert b"null ensemble" in L.vsom_last_error()
    assert L.vsom_ensemble_evaluate_applies(None, 0, 0) == -1
    assert b"null ensemble" in L.vsom_last_error()


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len
        self.width, self.height, self.n_nodes = 5, 3, 15

    def close(self):
        pass


def stub(lens=(5, 3)):
    ens = capi.Ensemble.__new__(capi.Ensemble)
    ens.members, ens._h, ens._pinned = [NoDevice(j) for j in lens], None, None
    return ens


OK = [np.ones((7, 5)), np.ones(3)]
COLS = [np.ones(5), np.ones(3)]


def test_column_checks_raise_before_the_call():
    ens = stub()
    for call in (lambda b, c: ens.evaluate(b, c), lambda b, c: ens.evaluate_masked(OK, b, c),
                 lambda b, c: ens.validation_errors(b, c), lambda b, c: ens.validation_errors(b, c, valid=OK, masked=True)):
        with pytest.raises(ValueError, match=r"binary: member 1: shape \(5,\), not \(3,\)"):
            call(np.ones(5), COLS)                         # one array for all members: the J differ
        with pytest.raises(ValueError, match=r"continuous: member 0: shape \(4,\), not \(5,\)"):
            call(COLS, [np.ones(4), np.ones(3)])
        with pytest.raises(ValueError, match="binary: 1 arrays for 2 members"):
            call([np.ones(5)], COLS)
        with pytest.raises(ValueError, match="continuous: 3 arrays for 2 members"):
            call(COLS, COLS + [np.ones(3)])
        with pytest.raises(ValueError, match="binary: member 0 is covered and has no array"):
            call([None, np.ones(3)], COLS)
        with pytest.raises(ValueError, match=r"binary: member 0: shape \(5, 1\)"):
            call([np.ones((5, 1)), np.ones(3)], COLS)


def test_member_and_validity_checks_raise_before_the_call():
    ens = stub()
    for bad in ([2], [0, 5], [-1]):
        with pytest.raises(ValueError, match="members must be indices"):
            ens.evaluate(COLS, COLS, members=bad)
    for wrong in ([np.ones((7, 5))], [None, None, None], np.ones((2, 7, 5))):
        with pytest.raises(ValueError, match=r"valid must be None or a list of one entry per member \(2\)"):
            ens.evaluate(COLS, COLS, valid=wrong)
    with pytest.raises(ValueError, match=r"valid: member 1: shape \(7, 5\), not \(7, 3\)"):
        ens.evaluate(COLS, COLS, valid=[None, np.ones((7, 5))])
    with pytest.raises(ValueError, match=r"valid: member 0: shape \(5,\), not \(7, 5\)"):
        ens.evaluate(COLS, COLS, valid=[np.ones(5), None])  # (a column mask is the masked call's)
    # the masked call: bmu_masked's validity and min_hits checks
    for bad in (np.ones(4), np.ones((7, 4)), np.ones((6, 5)), np.ones((7, 5, 1)), np.ones(())):
        with pytest.raises(ValueError, match="valid has shape"):
            ens.evaluate_masked([bad, None], COLS, COLS)
    for wrong in ([np.ones((7, 5))], [None, None, None], None):
        with pytest.raises(ValueError, match=r"one entry per member \(2\), None for a skipped member"):
            ens.evaluate_masked(wrong, COLS, COLS)
    with pytest.raises(ValueError, match="min_hits must be >= 0"):
        ens.evaluate_masked(OK, COLS, COLS, min_hits=-1)
    with pytest.raises(ValueError, match="values of min_hits for 2 members"):
        ens.evaluate_masked(OK, COLS, COLS, min_hits=[1, 2, 3])
    with pytest.raises(ValueError, match="masked=True: the members are chosen"):
        ens.validation_errors(COLS, COLS, valid=OK, members=[0], masked=True)


def test_one_array_serves_members_of_one_width():
    """binary / continuous given once reach the shape check of every covered member and of no other"""
    ens = stub((5, 5, 3))
    with pytest.raises(ValueError, match=r"binary: member 2: shape \(5,\), not \(3,\)"):
        ens.evaluate(np.ones(5), np.ones(5))
    keep, ptrs = ens._columns("binary", np.arange(5), [True, True, False])
    assert keep[2] is None and not ptrs[2] and keep[0].dtype == np.float32 and keep[0].tolist() == [0, 1, 2, 3, 4]
    assert ptrs[0] and ptrs[1]
    # a skipped member may have no array
    keep, ptrs = ens._columns("binary", [np.ones(5), None, None], [True, False, False])
    assert keep[1] is None and keep[2] is None and not ptrs[1]
