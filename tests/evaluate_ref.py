"""Restatements of Som::evaluate's per-row binary error (Som.cpp:503-519) for the vsom_evaluate_batch tests.

restate64: from the fp32 operands in float64 -- the value the tolerance of include/vsom_hip.h is stated against.
restate32: in numpy fp32, one rounding per operation; exact wherever every counting term is replaced by -99999 or has a
zero factor (its log then decides only the class NaN / inf, never a last bit)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyref  # noqa: E402

f32 = np.float32
L_ULPS = 1                                             # the device log's error bound, taken as an assumption (csrc/vsom_evaluate.hip)
QNAN = 0x7FC00000


def bound(C):
    """relative bound of bsum against restate64 (include/vsom_hip.h): (C + 2 L + 4) * 2^-24"""
    return (C + 2 * L_ULPS + 4) * 2.0 ** -24


def factors(binary, continuous, valid, n):
    """(b [C], val [n, C]) as fp32: val = valid ? continuous : 0"""
    b = np.asarray(binary, f32)
    c = np.asarray(continuous, f32)
    val = np.broadcast_to(c, (n, c.size)).copy()
    if valid is not None:
        val[np.asarray(valid) == 0] = f32(0)
    return b, val


def restate64(X, M, binary, continuous, valid=None):
    """X, M: rows x C (M = the model rows of the BMUs).  Returns (bsum float64 [rows], nrepl)."""
    X = np.asarray(X, f32)
    M = np.asarray(M, f32)
    b, val = factors(binary, continuous, valid, X.shape[0])
    om = (f32(1) - M).astype(f32)                      # formed in fp32 first
    ox = (f32(1) - X).astype(f32)
    with np.errstate(all="ignore"):
        be = np.log(M.astype(np.float64)) * X.astype(np.float64) + np.log(om.astype(np.float64)) * ox.astype(np.float64)
    repl = ~np.isfinite(be)
    be = np.where(repl, -99999.0, be)
    with np.errstate(all="ignore"):
        t = (be * b.astype(np.float64)) * val.astype(np.float64)
    nrepl = (repl & (b != 0)[None, :] & (val != 0)).sum(axis=1).astype(np.uint32)
    return (t * t).sum(axis=1), nrepl


def restate32(X, M, binary, continuous, valid=None):
    """The same in fp32 with the reference's order of operations.  Returns (bsum fp32 [rows] in Eigen's packet order,
    nrepl, exact, t): exact[r] says every counting term of row r was replaced, so bsum[r] holds bit for bit; t are the
    terms themselves."""
    X = np.asarray(X, f32)
    M = np.asarray(M, f32)
    b, val = factors(binary, continuous, valid, X.shape[0])
    om = (f32(1) - M).astype(f32)
    ox = (f32(1) - X).astype(f32)
    with np.errstate(all="ignore"):
        be = ((np.log(M).astype(f32) * X).astype(f32) + (np.log(om).astype(f32) * ox).astype(f32)).astype(f32)
        repl = ~np.isfinite(be)
        be = np.where(repl, f32(-99999.0), be).astype(f32)
        t = ((be * b[None, :]).astype(f32) * val).astype(f32)
    counts = (b != 0)[None, :] & (val != 0)
    zero = ((b == 0)[None, :] & np.isfinite(val)) | ((val == 0) & np.isfinite(b)[None, :])
    nrepl = (repl & counts).sum(axis=1).astype(np.uint32)
    exact = (repl | zero).all(axis=1)
    with np.errstate(all="ignore"):
        bsum = np.array([pyref.dot_self(row) for row in t], f32)
    return bsum, nrepl, exact, t


def sequential(t):
    """((0 + t0^2) + t1^2) + ... per row, in fp32: what a plain loop gives, for tests that the packet order is not that"""
    t = np.asarray(t, f32)
    acc = np.zeros(t.shape[0], f32)
    with np.errstate(all="ignore"):
        for d in range(t.shape[1]):
            acc = (acc + (t[:, d] * t[:, d]).astype(f32)).astype(f32)
    return acc


def running_mean(dist, bsum):
    """Som.cpp:519 over the rows, in double"""
    err = 0.0
    for i in range(len(dist)):
        s = float(bsum[i])
        err += 1.0 / (i + 1.0) * (float(dist[i]) + (math.sqrt(s) if s >= 0 else float("nan")) - err)
    return err


def same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def beq(a, b):
    """bit-equal float arrays, NaN equal to NaN"""
    a = np.asarray(a, f32)
    b = np.asarray(b, f32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
