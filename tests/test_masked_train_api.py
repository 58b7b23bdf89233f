"""CPU: the checker of vsom_batch_epoch_masked (tests/masked_train_ref.py) is pinned to the oracle -- with an all-valid
mask it is OracleSom.batch_epoch bit for bit --, the symbol is declared and exported, and the Python shape checks raise
before any call."""
import ctypes
import os
import sys

import numpy as np
import pytest

from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen  # noqa: E402
import masked_train_ref as mref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


@pytest.mark.parametrize("tr", (po.STANDARD, po.MEDIAN))
def test_all_valid_helper_is_the_oracle_epoch(tr):
    W, H, J, B = 7, 5, 9, 70
    X = gen.blobs(B, J, 4, 3, 2)
    init = gen.random_map(W * H, J, seed=13)
    orc = po.OracleSom(W, H, J, tr)
    orc.set_state(map=init)
    ref = mref.MaskedOracle(W, H, J, tr, init)
    lbo = np.zeros(B, np.uint64)
    lbr = np.zeros(B, np.uint64)
    ones = np.ones((B, J), bool)
    for e, sigma in enumerate((2.5, 2.0, 1.0)):
        mo = orc.batch_epoch(X, lbo, sigma, e == 0)
        mr, _ = ref.epoch(X, ones, lbr, sigma, e == 0)
        assert (lbo == lbr).all(), e
        assert beq(np.float32(mo), np.float32(mr)), (e, mo, mr)
        for name in ("map", "sigma", "weight", "hits"):
            assert beq(getattr(orc, name), getattr(ref, name)), (e, name)


def test_helper_skips_invalid_entries():
    """a column's chain runs over its valid rows only, and what the invalid positions hold does not matter"""
    W, H, J, B = 5, 4, 3, 12
    X = gen.blobs(B, J, 3, 5, 2)
    init = gen.random_map(W * H, J, seed=2)
    valid = np.ones((B, J), bool)
    valid[::2, 1] = False
    valid[:, 2] = False
    ref = mref.MaskedOracle(W, H, J, po.STANDARD, init)
    lb = np.zeros(B, np.uint64)
    ref.epoch(X, valid, lb, 2.0, True)
    X2 = X.copy()
    X2[~valid] = np.nan
    ref2 = mref.MaskedOracle(W, H, J, po.STANDARD, init)
    lb2 = np.zeros(B, np.uint64)
    ref2.epoch(X2, valid, lb2, 2.0, True)
    assert (lb == lb2).all() and beq(ref.map, ref2.map) and beq(ref.sigma, ref2.sigma)
    assert (ref.map[:, 2].view(np.uint32) == 0).all() and np.isnan(ref.sigma[:, 2]).all()    # no valid row: +0, sqrt(0/0)
    # column 1 is the oracle's phase 2 over the odd rows alone
    col = po.OracleSom(W, H, 1, po.STANDARD)
    col.batch_phase2_range(np.ascontiguousarray(X[1::2, 1:2]), np.ascontiguousarray(lb[1::2]), 2.0, 0, W * H)
    assert beq(col.map[:, 0], ref.map[:, 1]) and beq(col.sigma[:, 0], ref.sigma[:, 1])


def test_symbol_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "vsom_hip.h")).read()
    assert "int vsom_batch_epoch_masked(vsom_ctx *ctx, double sigma, int is_first, const uint8_t *valid_host, int one_mask," in txt
    assert "vsom_batch_epoch_masked" in capi.SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        capi.build()
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "vsom_batch_epoch_masked")
    assert hasattr(vs.Som, "trainBatchSomEpochMasked") and hasattr(vs.Som, "trainBatchSomMasked")


class NoDevice(capi.Context):
    """a Context without a handle: what runs before the library is called can be tested without a device"""

    chunk_size = 7

    def __init__(self, in_len):
        self._h = None
        self.in_len = in_len

    def close(self):
        pass


def test_shape_checks_raise_before_the_call():
    ctx = NoDevice(5)
    for bad in (np.ones(4), np.ones((7, 4)), np.ones((6, 5)), np.ones((7, 5, 1)), np.ones(())):
        with pytest.raises(ValueError, match="valid has shape"):
            ctx.batch_epoch_masked(2.0, True, bad)
