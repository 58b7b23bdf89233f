"""Reference for vsom_bmd_masked_batch / vsom_generate_masked_batch, composed of pieces that already exist:

distribution  masked_score_ref.masked_dists (the oracle's Comparer, +0 at invalid columns, the oracle's dot) under
              generate_ref.bmd_p / draw: p_i = hits_i >= min_hits ? exp(-(double)d_i * d_i / 2) : 0, the sequential sum, the draw
records       generate_ref.decode / bound / within, with the keep-observed select on top: a valid column of a row is the
              row's own value whatever L holds there; a draw without mass is the quiet NaN throughout

and the inputs of the GPU draw tests (case): tests/test_bmd_masked_api.py counts, on this reference alone, how many of their
draws lie within relative 1e-12 of a cumulative boundary -- the exclusion rule and cap of tests/test_gpu_bmd_batch.py."""
import functools
import os
import sys

import numpy as np

from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import generate_ref as gr  # noqa: E402
import masked_score_ref as msr  # noqa: E402

f32 = np.float32
NO_UNIT = gr.NO_UNIT
QNAN_BITS = gr.QNAN_BITS
B = 70                                    # one 64-row tile and 6 rows; no multiple of the 8 rows of a row-pass workgroup
MAPS = ((7, 5), (9, 15), (17, 16))        # 35 nodes: under one node tile; 135: two tiles and a ragged one; 272: a second
                                          # 256-node chunk of 16 nodes, so the draw's chunk search and re-walk run
DEPTHS = (3, 9, 37, 70)
KINDS = (po.STANDARD, po.MEDIAN)
SHAPES = [(tr, W, H, J) for tr in KINDS for (W, H) in MAPS for J in DEPTHS]
DRAWS = (1, 3, 7)
MIN_HITS = (0, 3)
NO_VALID_ROW = 5                          # the row of a random case without a valid column
NEAR = 1e-12                              # a draw this close (relative) to a cumulative boundary is not compared
NEAR_CAP = 1                              # at most this many per case


# ---- state and rows (as tests/test_gpu_masked_score.py states them) -------------------------------------------------------
def unit_state(W, H, J, seed):
    """a map in (0, 1), a sigmaMap with entries on both sides of 1e-5, mixed hit counts (0 .. 5, node 0 without hits)"""
    rng = np.random.default_rng(seed)
    N = W * H
    M = rng.uniform(0.02, 0.98, (N, J)).astype(f32)
    S = (rng.random((N, J)) * 0.2).astype(f32)
    S[rng.random((N, J)) < 0.15] = f32(3e-6)
    hits = rng.integers(0, 6, N).astype(np.uint64)
    hits[0] = 0
    return M, S, hits


def unit_rows(rows, J, seed):
    """rows in [0, 1] with some entries exactly 0 and some exactly 1"""
    rng = np.random.default_rng(seed)
    X = rng.random((rows, J)).astype(f32)
    X[rng.random((rows, J)) < 0.08] = f32(0)
    X[rng.random((rows, J)) < 0.08] = f32(1)
    return X


# ---- the distribution -----------------------------------------------------------------------------------------------------
def masked_d(kind, X, M, valid):
    """the fp32 masked distances, rows x N; valid: rows x J or one row of J"""
    valid = np.asarray(valid) != 0
    with np.errstate(all="ignore"):
        return np.array([msr.masked_dists(kind, X[r], M, valid if valid.ndim == 1 else valid[r]) for r in range(X.shape[0])],
                        f32)


def distribution(d, hits, min_hits):
    """(P, norm, prob) from the masked distances: P rows x N, norm the sequential sum in node order, prob = P / norm"""
    P = np.array([gr.bmd_p(row, hits, min_hits) for row in d], np.float64).reshape(len(d), -1)
    norm = np.array([np.cumsum(p)[-1] for p in P], np.float64)
    with np.errstate(all="ignore"):
        prob = P / norm[:, None]
    return P, norm, prob


def near(p, u):
    """the relative distance of t = u * C to the nearest cumulative boundary (inf for a row without mass)"""
    cum = np.cumsum(np.asarray(p, np.float64))
    C = cum[-1]
    if not (C > 0 and np.isfinite(C)):
        return np.inf
    t = u * C
    return float(np.min(np.abs(cum - t)) / max(t, np.finfo(np.float64).tiny))


def draws(P, U):
    """(unit, near) for the uniforms U (rows, or rows x K): generate_ref.draw per entry from the row's P"""
    U = np.asarray(U, np.float64)
    flat = U.reshape(U.shape[0], -1)
    unit = np.array([[gr.draw(P[r], u) for u in flat[r]] for r in range(flat.shape[0])], np.uint64).reshape(U.shape)
    nr = np.array([[near(P[r], u) for u in flat[r]] for r in range(flat.shape[0])], np.float64).reshape(U.shape)
    return unit, nr


# ---- the records ----------------------------------------------------------------------------------------------------------
def keep_select(rec, X, valid, unit, keep):
    """the keep-observed select over decoded records: rec rows x K x J, X rows x J, valid rows x J or J, unit rows x K.
    A kept column of a draw with mass is (double)x; a draw without mass stays the quiet NaN throughout."""
    rec = np.array(rec, np.float64)
    if not keep:
        return rec, np.zeros(rec.shape, bool)
    valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
    kept = valid[:, None, :] & (np.asarray(unit) != NO_UNIT)[:, :, None]
    return np.where(kept, np.asarray(X, f32).astype(np.float64)[:, None, :], rec), kept


def records(M, S, unit, L, X, valid, keep):
    """(rec, zs, kept): the float64 restatement of vsom_generate_masked_batch's records for the given units; zs = z * s of
    the sampled columns (0 at kept ones, which carry no tolerance)"""
    unit = np.asarray(unit, np.uint64)
    n, K = unit.shape
    L = np.asarray(L, np.float64).reshape(n, K, -1)
    rec, zs = gr.decode(M, S, unit.reshape(-1), L.reshape(n * K, -1))
    rec, kept = keep_select(rec.reshape(L.shape), X, valid, unit, keep)
    return rec, np.where(kept, 0.0, zs.reshape(L.shape)), kept


# ---- the inputs of the GPU draw tests ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(tr, W, H, J):
    """a random case: state, rows with NaN at every invalid position, ~70 % valid entries with one row without a valid column,
    uniforms for up to max(DRAWS) draws per row, and the masked distances of the reference.  Shared, never modified."""
    seed = 1000 * W + 10 * J + int(tr)
    M, S, hits = unit_state(W, H, J, seed)
    rng = np.random.default_rng(seed + 1)
    valid = rng.random((B, J)) < 0.7
    valid[NO_VALID_ROW, :] = False
    X = np.where(valid, unit_rows(B, J, seed + 2), f32(np.nan)).astype(f32)
    U = rng.random((B, max(DRAWS)))
    c = dict(tr=tr, W=W, H=H, J=J, M=M, S=S, hits=hits, X=X, valid=valid, U=U, d=masked_d(tr, X, M, valid))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def case_draws(c, min_hits):
    """(P, norm, prob, unit, near) of a case: the reference's distribution and its draws for every uniform of the case"""
    P, norm, prob = distribution(c["d"], c["hits"], min_hits)
    unit, nr = draws(P, c["U"])
    return P, norm, prob, unit, nr
