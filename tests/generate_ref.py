"""Restatements of Som::autoEncoder's pieces (Som.cpp:457-487, 568-623) in float64 numpy for the vsom_generate_batch tests:
the restricted best matching distribution and the draw from the fp32 distances, the decode in the order of :609, and the
tolerance of include/vsom_hip.h."""
import numpy as np

NO_UNIT = np.uint64(0xFFFFFFFFFFFFFFFF)
QNAN_BITS = np.uint64(0x7FF8000000000000)
LD_ULPS = 1        # the device double log's error bound, taken as an assumption (csrc/vsom_generate.hip names the source)
LH_ULPS = 1        # the host log's (numpy / libm), likewise
EPS = 2.0 ** -52


def bmd_p(dist, hits, min_hits):
    """p_i = hits_i >= min_hits ? exp(-(double)d_i * d_i / 2) : 0 from the fp32 distances of one row"""
    d = np.asarray(dist, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.exp(-d * d / 2)
    return np.where(np.asarray(hits, np.uint64) >= np.uint64(min_hits), p, 0.0)


def draw(p, u):
    """C = ((0 + p_0) + p_1) + ...; the smallest i whose running sum exceeds u * C, the largest i with p_i > 0 when rounding
    leaves none, NO_UNIT when C is 0 or not finite"""
    cum = np.cumsum(np.asarray(p, np.float64))          # sequential, in node order
    C = cum[-1]
    if not (C > 0 and np.isfinite(C)):
        return NO_UNIT
    above = np.nonzero(cum > u * C)[0]
    return np.uint64(above[0]) if above.size else np.uint64(np.nonzero(p > 0)[0][-1])


def decode(M, S, units, L):
    """M, S: the map and sigmaMap as vsom_get_state returns them (N x D, fp32); units: one per row; L: rows x C float64.
    q = L / (1 - L); g = log(q); z = g / 1.6; t = z * (double)s; rec = t + (double)m, one rounding per operation.
    Returns (rec, z * s): a row whose unit is not a node holds the quiet NaN 0x7FF8000000000000."""
    L = np.asarray(L, np.float64)
    units = np.asarray(units, np.uint64)
    n, C = L.shape
    rec = np.full((n, C), 0, np.uint64)
    rec[...] = QNAN_BITS
    rec = rec.view(np.float64)
    zs = np.zeros((n, C), np.float64)
    ok = units < np.uint64(M.shape[0])
    b = units[ok].astype(np.int64)
    m = np.asarray(M, np.float32)[b, :C].astype(np.float64)
    s = np.asarray(S, np.float32)[b, :C].astype(np.float64)
    with np.errstate(all="ignore"):
        q = L[ok] / (1.0 - L[ok])
        g = np.log(q)
        z = g / 1.6
        t = z * s
        rec[ok] = t + m
    zs[ok] = t
    return rec, zs


def bound(rec_ref, zs):
    """|rec_dev - rec_ref| <= (Ld + Lh + 2) * 2^-52 * |z s| + 2^-52 * |rec_ref| (include/vsom_hip.h)"""
    with np.errstate(all="ignore"):
        return (LD_ULPS + LH_ULPS + 2) * EPS * np.abs(zs) + EPS * np.abs(rec_ref)


def beq(a, b):
    """bit-equal float64 arrays, NaN equal to NaN"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def within(got, rec_ref, zs):
    """(ok, worst): every finite reference value within the bound, every other one (inf, NaN) the same value; worst = the
    largest error in units of its bound"""
    got = np.asarray(got, np.float64)
    fin = np.isfinite(rec_ref) & np.isfinite(zs)
    if not beq(np.where(fin, 0.0, got), np.where(fin, 0.0, rec_ref)):
        return False, np.inf
    if not fin.any():
        return True, 0.0
    err = np.abs(got[fin] - rec_ref[fin])
    bnd = bound(rec_ref[fin], zs[fin])
    if not np.isfinite(got[fin]).all():
        return False, np.inf
    exact = err == 0
    ratio = np.where(exact, 0.0, err / np.where(bnd > 0, bnd, 1.0))
    ratio = np.where(~exact & (bnd == 0), np.inf, ratio)
    return bool((err <= bnd).all()), float(ratio.max())
