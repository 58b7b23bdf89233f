"""The cases of the masked online chunk shared by tests/test_online_masked_ref.py (CPU) and tests/test_gpu_online_masked.py:
shapes, rows, maps, masks, and the reference's snapshots (computed once per case; callers do not modify them)."""
import functools
import os
import sys

import numpy as np

from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_masked_ref as oref  # noqa: E402

f32 = np.float32
KINDS = (po.STANDARD, po.MEDIAN)
DECAYS = (po.EXPONENTIAL, po.INVERSE_PROPORTIONAL)
SIGMAS = (3.0, 1.5, 1.0, 0.3)        # window clipped at the edges; small window; the one-launch step; its empty window
ETA = 0.3
# W, H, J, B.  7x5x9: 35 nodes are no multiple of the 32 a scan workgroup holds, J = one packet block + a scalar tail;
# 12x9x20: a packet tail of 4; 16x16x33; 40x36x70: 45 scan workgroups, more than the 16 key slots (Standard, sigma 3 only)
SMALL = ((7, 5, 9, 11), (12, 9, 20, 7), (16, 16, 33, 37))
BIG = (40, 36, 70, 20)
POISON = (f32(np.nan), f32(np.inf), f32(-np.inf), f32(1e30))


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def same(got, want, what, keys=None):
    for k in keys or want:
        assert beq(got[k], want[k]), (what, k)


@functools.lru_cache(maxsize=None)
def data(W, H, J, B, seed=6):
    """uniform [0, 1) rows, map, SMap and a starting lastBMU, and a mask with 30 % invalid entries"""
    rng = np.random.default_rng(seed)
    X = rng.random((B, J), dtype=f32)
    M = rng.random((W * H, J), dtype=f32)
    valid = rng.random((B, J)) < 0.7
    S = (rng.random((W * H, J), dtype=f32) * f32(0.1)).astype(f32)
    start = rng.integers(0, W * H, B).astype(np.uint64)
    for a in (X, M, valid, S, start):
        a.setflags(write=False)
    return X, M, valid, S, start


def poisoned(X, valid):
    """NaN, +-inf and 1e30 at the invalid positions"""
    X2 = np.array(X)
    for i, (r, d) in enumerate(np.argwhere(~np.broadcast_to(valid, X.shape))):
        X2[r, d] = POISON[i % len(POISON)]
    return X2


def start_of(sigma, start, B):
    """lastBMU before a chunk: zero as a load leaves it (sigma > 1 ignores it), the given units for the local walk"""
    return np.array(start) if sigma <= 1 else np.zeros(B, np.uint64)


def ref_new(tr, W, H, J, M, S):
    r = oref.OnlineMasked(W, H, J, tr)
    r.set_state(map=M, S=S)
    return r


@functools.lru_cache(maxsize=None)
def reference(tr, W, H, J, B, fn, sigma):
    """snapshot of the reference after the case's random-mask chunk (poisoned rows)"""
    X, M, valid, S, start = data(W, H, J, B)
    r = ref_new(tr, W, H, J, M, S)
    lb = start_of(sigma, start, B)
    mse = r.train_chunk(poisoned(X, valid), valid, lb, ETA, sigma, fn)
    return r.snapshot(lb, mse)


def oracle_chunk(tr, W, H, J, M, S, X, lb, eta, sigma, fn, mse_start=0.0):
    """snapshot of the C oracle after one unmasked chunk"""
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=M, S=S)
    lb = np.array(lb, np.uint64)
    mse = o.train_online_chunk(X, lb, eta, sigma, fn, mse_start)
    snap = {"map": o.map.copy(), "S": o.S.copy(), "sigma": o.sigma.copy(), "weight": o.weight.copy(),
            "hits": o.hits.copy(), "lastbmu": lb, "mse": np.array([mse], f32)}
    o.close()
    return snap
