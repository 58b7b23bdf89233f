"""CPU: the checker of vsom_train_online_chunk_masked (tests/online_masked_ref.py) is pinned to the oracle -- with an
all-valid mask it is po.OracleSom.train_online_chunk bit for bit, and what the rows hold at invalid positions changes nothing.
From the reference alone: on every random-mask case of tests/test_gpu_online_masked.py the mask is seen to matter (a
masked BMU differs from the oracle's BMU on the zero-filled rows) and an updated window node has both a valid and an invalid
column."""
import numpy as np
import pytest

import online_masked_cases as oc
from oracle import pyoracle as po

GRID = [s for s in oc.SMALL[:2]]          # 7x5x9 (B = 11), 12x9x20 (B = 7)
KEYS = ("map", "S", "sigma", "weight", "hits", "lastbmu", "mse")


@pytest.mark.parametrize("sigma", oc.SIGMAS)
@pytest.mark.parametrize("fn", oc.DECAYS)
@pytest.mark.parametrize("tr", oc.KINDS)
@pytest.mark.parametrize("shape", GRID)
def test_all_valid_is_the_oracle_and_invalid_entries_do_not_matter(shape, tr, fn, sigma):
    W, H, J, B = shape
    X, M, valid, S, start = oc.data(W, H, J, B)
    lb0 = oc.start_of(sigma, start, B)
    want = oc.oracle_chunk(tr, W, H, J, M, S, X, lb0, oc.ETA, sigma, fn)
    for mask in (np.ones((B, J), bool), np.ones(J, bool)):
        r = oc.ref_new(tr, W, H, J, M, S)
        lb = lb0.copy()
        mse = r.train_chunk(X, mask, lb, oc.ETA, sigma, fn)
        oc.same(r.snapshot(lb, mse), want, "all valid", KEYS)
    # zeros against NaN / inf at the invalid positions
    r = oc.ref_new(tr, W, H, J, M, S)
    lb = lb0.copy()
    mse = r.train_chunk(np.where(valid, X, np.float32(0)), valid, lb, oc.ETA, sigma, fn)
    oc.same(r.snapshot(lb, mse), oc.reference(tr, W, H, J, B, fn, sigma), "poisoned rows", KEYS)


@pytest.mark.parametrize("shape", oc.SMALL + (oc.BIG,))
def test_the_mask_matters(shape):
    W, H, J, B = shape
    tr, fn, sigma = po.STANDARD, po.EXPONENTIAL, 3.0
    X, M, valid, S, start = oc.data(W, H, J, B)
    masked = oc.reference(tr, W, H, J, B, fn, sigma)
    zero = oc.oracle_chunk(tr, W, H, J, M, S, np.where(valid, X, np.float32(0)), np.zeros(B, np.uint64), oc.ETA, sigma, fn)
    differ = int((masked["lastbmu"] != zero["lastbmu"]).sum())
    print(f"{W}x{H}x{J}: the masked BMU differs from the zero-filled one for {differ} of {B} samples")
    assert differ >= 1
    assert not oc.beq(masked["map"], zero["map"])


@pytest.mark.parametrize("shape", oc.SMALL + (oc.BIG,))
def test_a_window_node_has_valid_and_invalid_columns(shape):
    W, H, J, B = shape
    X, M, valid, S, start = oc.data(W, H, J, B)
    mixed = [j for j in range(B) if valid[j].any() and not valid[j].all()]
    assert mixed
    j = mixed[0]
    r = oc.ref_new(po.STANDARD, W, H, J, M, S)
    r.train_sample(X[j], valid[j], oc.ETA, 3.0, 0, po.EXPONENTIAL)
    nodes = np.flatnonzero(r.weight != 0)            # the window's nodes
    assert nodes.size >= 1
    changed = r.map[nodes] != M[nodes]
    assert changed[:, valid[j]].any(axis=1).all()    # every window node moved at a valid column
    assert not changed[:, ~valid[j]].any()           # and none at an invalid one
    assert oc.beq(r.S[:, ~valid[j]], S[:, ~valid[j]]) and not r.sigma[:, ~valid[j]].any()
