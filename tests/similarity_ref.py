"""Numpy restatement of Som::measureSimilarity (reference src/Som.cpp:631-714) for the similarity tests: the per-column
arithmetic in fp32 (elementwise np.float32 subtraction, division and multiplication are single IEEE roundings), the
per-row results vsom_similarity_batch returns, and the reference's literal double loop."""
import numpy as np

T = np.float32(-99999999.0)
EPS = np.float32(0.00001)
NONE = np.uint32(0xFFFFFFFF)
QNAN = np.uint32(0x7FC00000)


def beq(a, b):
    """bitwise equality; NaN equals NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


def columns(X, m, s, num_sigmas, floor):
    """delta, lo, hi (fp32, rows x C) of rows X against the gathered model rows m and sigma rows s"""
    X, m, s = (np.asarray(a, np.float32) for a in (X, m, s))
    k = np.float32(num_sigmas)
    with np.errstate(all="ignore"):
        sM = (np.where(s > EPS, s, EPS) if floor else np.where(s > EPS, EPS, s)).astype(np.float32)
        delta = ((X - m) / sM / k).astype(np.float32)
        sk = (sM * k).astype(np.float32)
        lo, hi = (m - sk).astype(np.float32), (m + sk).astype(np.float32)
    return delta, lo, hi


def first_max(vals, cols):
    """(value, column) of the largest value, the lowest column on ties (float comparison: -0 ties with +0)"""
    j = int(np.argmax(vals))
    return vals[j], np.uint32(cols[j])


def rows_from_delta(delta):
    """first and dmax (with dmax_col) of every row of a delta matrix"""
    n = delta.shape[0]
    first = np.full(n, QNAN.view(np.float32), np.float32)
    dmax = np.full(n, -np.inf, np.float32)
    dmax_col = np.full(n, NONE, np.uint32)
    with np.errstate(all="ignore"):
        for r in range(n):
            above = np.flatnonzero(delta[r] > T)
            if above.size:
                first[r] = delta[r, above[0]]
            ok = np.flatnonzero(~np.isnan(delta[r]))
            if ok.size:
                dmax[r], dmax_col[r] = first_max(delta[r, ok], ok)
    return first, dmax, dmax_col


def report(X, m, s, num_sigmas, floor, valid=None, want_delta=True):
    """what vsom_similarity_batch returns for rows X (rows x C) whose BMUs have model rows m and sigma rows s"""
    X = np.asarray(X, np.float32)
    n, C = X.shape
    delta, lo, hi = columns(X, m, s, num_sigmas, floor)
    valid = np.ones((n, C), bool) if valid is None else (np.asarray(valid)[:, :C] != 0)
    first, dmax, dmax_col = rows_from_delta(delta)
    amax = np.zeros(n, np.float32)
    amax_col = np.full(n, NONE, np.uint32)
    with np.errstate(all="ignore"):
        for r in range(n):
            ok = np.flatnonzero(valid[r] & np.isfinite(delta[r]))
            if ok.size:
                amax[r], amax_col[r] = first_max(np.abs(delta[r, ok]), ok)
        outside = (valid & ((X < lo) | (X > hi))).sum(axis=1).astype(np.uint32)
    out = {"dmax": dmax, "dmax_col": dmax_col, "first": first, "amax": amax, "amax_col": amax_col, "outside": outside}
    if want_delta:
        out["delta"] = np.where(np.isfinite(delta), delta, np.float32(0)).astype(np.float32)
    return out


def literal_loop(delta, X=None, lo=None, hi=None, valid=None):
    """Som.cpp:641-711 as written, on a given delta matrix: (maxValueDataSetRow, success).  Without X / lo / hi only the
    row is meaningful (success is True)."""
    n, C = delta.shape
    maxv, maxrow, last, success = T, 0, False, True
    i = 0
    with np.errstate(all="ignore"):
        while i < n + 1:
            if i == n:
                i, last = maxrow, True
            for c in range(C):
                if delta[i, c] > maxv:
                    maxv, maxrow = np.float32(abs(delta[i, c])), i
                if last and X is not None and (valid is None or valid[i, c]):
                    if X[i, c] < lo[i, c] or X[i, c] > hi[i, c]:
                        success = False
            if last:
                break
            i += 1
    return maxrow, success
