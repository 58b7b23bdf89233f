"""Reference for vsom_similarity_masked_batch / vsom_evaluate_masked_batch, composed of pieces that already exist:

search      the masked distance and findRestrictedBmu's argmin as tests/test_gpu_masked.py states them, over pyoracle's
            Comparer and dot product (restated here: importing a test module would collect its tests a second time)
similarity  similarity_ref.columns / rows_from_delta / report, with delta set to NaN at the invalid columns first
evaluate    evaluate_ref.restate32 / restate64 / bound / running_mean, with the select at the invalid columns: the term of
            an invalid column is +0 whatever the row, the model row and the column factors hold there
"""
import os
import sys

import numpy as np

from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_ref as er  # noqa: E402
import pyref  # noqa: E402
import similarity_ref as sr  # noqa: E402

f32 = np.float32
QNAN = np.uint32(0x7FC00000)
ROW_KEYS = ("dmax", "dmax_col", "first", "amax", "amax_col", "outside")
POISON = (f32(np.nan), f32(np.inf), f32(1e30), f32(-np.inf), f32(-3.5), f32(7.25))   # NaN, +-inf, 1e30, outside [0, 1]


# ---- search -------------------------------------------------------------------------------------------------------------
def masked_dists(kind, x, M, valid):
    """the masked distance of row x to every node: the oracle's Comparer, +0 at invalid columns, the oracle's dot"""
    return np.array([po.dot_self(np.where(valid, po.comparer(kind, x, m), f32(0))) for m in M], f32)


def argmin_rule(d, hits, min_hits):
    """Som::findRestrictedBmu (Som.cpp:313-332): node 0 seeds, then strict < over the nodes with enough hits"""
    best, bd = 0, d[0]
    for n in range(len(d)):
        if d[n] < bd and hits[n] >= min_hits:
            best, bd = n, d[n]
    return best, bd


def checker(kind, X, M, valid, hits, min_hits, rows=None):
    """(bmu, dist) of the rows (all of them when None); valid: rows x J or one row of J; a NaN distance is 0x7FC00000"""
    rows = range(X.shape[0]) if rows is None else rows
    bmu, dist = [], []
    with np.errstate(all="ignore"):
        for r in rows:
            v = valid if valid.ndim == 1 else valid[r]
            b, d = argmin_rule(masked_dists(kind, X[r], M, v), hits, min_hits)
            bmu.append(b)
            dist.append(d)
    dist = np.array(dist, f32)
    dist[np.isnan(dist)] = QNAN.view(f32)
    return np.array(bmu, np.uint64), dist


# ---- similarity ---------------------------------------------------------------------------------------------------------
def masked_delta(delta, valid):
    """delta with the quiet NaN at every invalid column"""
    return np.where(np.asarray(valid) != 0, delta, QNAN.view(f32)).astype(f32)


def similarity_from(delta, X, lo, hi, valid, want_delta=True):
    """the per-row results from a delta matrix (before masking), the rows and their intervals: first / dmax over the masked
    delta (similarity_ref.rows_from_delta), amax / outside over the valid columns as similarity_ref.report takes them"""
    valid = np.asarray(valid) != 0
    n = delta.shape[0]
    md = masked_delta(delta, valid)
    first, dmax, dmax_col = sr.rows_from_delta(md)
    amax = np.zeros(n, f32)
    amax_col = np.full(n, sr.NONE, np.uint32)
    with np.errstate(all="ignore"):
        for r in range(n):
            ok = np.flatnonzero(np.isfinite(md[r]))
            if ok.size:
                amax[r], amax_col[r] = sr.first_max(np.abs(md[r, ok]), ok)
        outside = (valid & ((X < lo) | (X > hi))).sum(axis=1).astype(np.uint32)
    out = {"dmax": dmax, "dmax_col": dmax_col, "first": first, "amax": amax, "amax_col": amax_col, "outside": outside}
    if want_delta:
        out["delta"] = np.where(np.isfinite(md), md, f32(0)).astype(f32)
    return out


def similarity(X, m, s, num_sigmas, floor, valid, want_delta=True):
    """what vsom_similarity_masked_batch reports for rows X (rows x J) whose units have model rows m and sigma rows s;
    valid: rows x J or one row of J.  amax / amax_col / outside are similarity_ref.report's own (asserted)"""
    X = np.asarray(X, f32)
    valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
    delta, lo, hi = sr.columns(X, m, s, num_sigmas, floor)
    out = similarity_from(delta, X, lo, hi, valid, want_delta)
    plain = sr.report(X, m, s, num_sigmas, floor, valid, want_delta=False)
    for k in ("amax", "amax_col", "outside"):
        assert sr.beq(out[k], plain[k]), k
    return out


# ---- evaluate -----------------------------------------------------------------------------------------------------------
def _neutral(X, M, valid):
    """the rows and model rows with a harmless value at the invalid columns: nothing stored there may matter"""
    return np.where(valid, X, f32(0.5)).astype(f32), np.where(valid, M, f32(0.5)).astype(f32)


def evaluate32(X, M, binary, continuous, valid):
    """evaluate_ref.restate32 with t = valid ? (be * binary) * continuous : +0.  Returns (bsum fp32 in Eigen's packet
    order, nrepl over the valid columns, exact, t)."""
    X = np.asarray(X, f32)
    valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
    Xn, Mn = _neutral(X, np.asarray(M, f32), valid)
    _, nrepl, exact, t = er.restate32(Xn, Mn, binary, continuous, valid)
    t = np.where(valid, t, f32(0)).astype(f32)         # the select (restate32 multiplied by a zero val)
    with np.errstate(all="ignore"):
        bsum = np.array([pyref.dot_self(row) for row in t], f32)
    return bsum, nrepl, exact, t


def evaluate64(X, M, binary, continuous, valid):
    """evaluate_ref.restate64 with the select: (bsum float64, nrepl).  In float64 the product of a finite term and finite
    factors cannot overflow, so its multiplication by the zero val is the select's +0."""
    X = np.asarray(X, f32)
    valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
    assert np.isfinite(np.asarray(binary, f32)).all() and np.isfinite(np.asarray(continuous, f32)).all()
    Xn, Mn = _neutral(X, np.asarray(M, f32), valid)
    return er.restate64(Xn, Mn, binary, continuous, valid)


bound = er.bound
running_mean = er.running_mean
same_double = er.same_double
beq = sr.beq
