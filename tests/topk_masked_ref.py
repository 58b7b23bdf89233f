"""Reference for vsom_bmu_topk_masked_batch, a numpy restatement of its contract:

distances   masked_score_ref.masked_dists (the oracle's Comparer, +0 at invalid columns, the oracle's dot), as
            bmd_masked_ref.masked_d collects them
candidates  node 0 always, and every node with hits >= min_hits
order       the key (bits of d, node) with NaN after +inf; when d_0 is NaN node 0 comes first and the others follow in key
            order; a NaN distance is stored as 0x7FC00000
padding     a row with fewer than k candidates: idx = UINT64_MAX, dist = 0x7FC00000 from entry count on
blend       in float64, one rounding per operation, in the order the header states: a_j = (double)d_j * (double)d_j, t = the
            a of the first entry whose distance is not NaN, q_j = exp(-(a_j - t) / 2) for finite d_j and 0 otherwise, zero
            terms skipped, Q and num_d summed sequentially in list order; (double)x at valid columns, num_d / Q at invalid
            ones, the quiet NaN where the row has no mass

The inputs are bmd_masked_ref.case / SHAPES (70 rows: one tile and 6; maps of 35, 135 and 272 nodes; J = 3, 9, 37, 70; NaN at
every invalid position; row 5 without a valid column; hits 0..5, node 0 without hits)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bmd_masked_ref as bmr  # noqa: E402

f32 = np.float32
NO_UNIT = np.uint64(2 ** 64 - 1)
QNAN32 = np.uint32(0x7FC00000)
QNAN64 = np.uint64(0x7FF8000000000000)
B = bmr.B
SHAPES = bmr.SHAPES
NO_VALID_ROW = bmr.NO_VALID_ROW
MIN_HITS = (0, 3, 6)
case = bmr.case
masked_d = bmr.masked_d


def beq(a, b):
    """bitwise equality of arrays of one type; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        w = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(w) == b.view(w)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def keys(d):
    """vsom_key over a row of fp32 distances: (bits, node), NaN -> 0xFFFFFFFF"""
    d = np.asarray(d, f32)
    bits = d.view(np.uint32).astype(np.uint64)
    bits[np.isnan(d)] = 0xFFFFFFFF
    return (bits << np.uint64(32)) | np.arange(d.size, dtype=np.uint64)


def candidates(hits, min_hits):
    """node 0, and the nodes with enough hits, in index order"""
    ok = np.asarray(hits) >= np.uint64(min_hits)
    ok[0] = True
    return np.flatnonzero(ok)


def row_list(d, hits, min_hits, k):
    """(idx uint64[k], dist float32[k], count) of one row of masked distances d (fp32 of every node)"""
    d = np.asarray(d, f32)
    cand = candidates(hits, min_hits)
    order = cand[np.argsort(keys(d)[cand], kind="stable")]
    if np.isnan(d[0]):
        order = np.concatenate([[0], order[order != 0]])
    count = min(k, order.size)
    idx = np.full(k, NO_UNIT, np.uint64)
    dist = np.full(k, QNAN32.view(f32), f32)
    idx[:count] = order[:count]
    got = d[order[:count]].copy()
    got[np.isnan(got)] = QNAN32.view(f32)
    dist[:count] = got
    return idx, dist, count


def lists(d, hits, min_hits, k):
    """(idx rows x k, dist rows x k, count rows) from the masked distances d (rows x N)"""
    n = d.shape[0]
    idx = np.empty((n, k), np.uint64)
    dist = np.empty((n, k), f32)
    count = np.empty(n, np.uint32)
    for r in range(n):
        idx[r], dist[r], count[r] = row_list(d[r], hits, min_hits, k)
    return idx, dist, count


def weights(dist, count, dtype=np.float64):
    """(q over the real entries, mass) of one row's stored distances, in `dtype`"""
    d = np.asarray(dist[:count], f32).astype(dtype)
    q = np.zeros(count, dtype)
    notnan = np.flatnonzero(~np.isnan(d))
    if notnan.size == 0 or not np.isfinite(d[notnan[0]]):
        return q, False
    a = d * d
    t = a[notnan[0]]
    with np.errstate(all="ignore"):
        for j in range(count):
            if np.isfinite(d[j]):
                q[j] = np.exp(-(a[j] - t) / dtype(2))
    return q, True


def blend_row(x, valid, M, idx, dist, count, dtype=np.float64):
    """one row of blend in `dtype` (float64: the contract's operations in their order; longdouble: the yardstick)"""
    J = x.size
    q, mass = weights(dist, count, dtype)
    out = np.empty(J, dtype)
    Q = dtype(0)
    num = np.zeros(J, dtype)
    with np.errstate(all="ignore"):
        for j in range(count):
            if q[j] != 0:
                Q = Q + q[j]
                num = num + q[j] * np.asarray(M[int(idx[j])], f32).astype(dtype)
        for c in range(J):
            if valid[c]:
                out[c] = dtype(x[c])
            elif not mass:
                out[c] = np.nan
            else:
                out[c] = num[c] / Q
    return out, mass


def blend(X, valid, M, idx, dist, count, dtype=np.float64):
    """(blend rows x J, mass rows); valid: rows x J or one row of J.  A row without mass holds the quiet NaN
    0x7FF8000000000000 at its invalid columns (float64)."""
    valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
    out = np.empty(X.shape, dtype)
    mass = np.empty(X.shape[0], bool)
    for r in range(X.shape[0]):
        out[r], mass[r] = blend_row(X[r], valid[r], M, idx[r], dist[r], int(count[r]), dtype)
    if dtype is np.float64:
        nomass = ~mass[:, None] & ~valid
        out.view(np.uint64)[nomass] = QNAN64
    return out, mass


def blend_bound(M, idx, count, k):
    """the bound on |blend - ref| per row and column at invalid columns with mass: (k + 2) * 2^-51 * max_j |m[j][d]| over
    the row's real entries.  exp is within an ulp of libm's on either side, each sequential k-term sum and each product adds
    half an ulp, the quotient one more; doubled for the two sides."""
    n = idx.shape[0]
    out = np.zeros((n, M.shape[1]), np.float64)
    for r in range(n):
        c = int(count[r])
        if c:
            out[r] = np.abs(np.asarray(M, f32)[idx[r, :c].astype(np.int64)].astype(np.float64)).max(axis=0)
    return (k + 2) * 2.0 ** -51 * out


def nvalid(valid, rows):
    valid = np.asarray(valid) != 0
    return np.broadcast_to(valid, (rows, valid.shape[-1])).sum(axis=1).astype(np.uint32)
