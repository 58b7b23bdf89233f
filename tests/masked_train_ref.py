"""CPU restatement of vsom_batch_epoch_masked (no GPU), built on oracle/pyoracle.py and tests/pyref.py only.

Phase 1 is pyref.Som with `dist` overridden by the masked distance (r_d = valid[d] ? m_d - x_d : +0, the oracle's dot): the
full search and find_local_bmu; OracleSom.batch_phase1_finish gives hits and MSE.  Phase 2, for every column d, is an
OracleSom(W, H, 1, tr).batch_phase2_range over X[rows valid at d, d] with those rows' units; weightMap comes from a run over
all rows.  (A column of the oracle's phase 2 does not depend on the other columns, and the oracle accepts zero rows: map 0,
sigma NaN.)"""
import os
import sys

import numpy as np

from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyref  # noqa: E402

f32 = np.float32


class MaskedSearch(pyref.Som):
    """pyref.Som whose distance runs over the valid columns of the row being searched (`valid`, set per row)"""

    valid = None

    def dist(self, node, v):
        with np.errstate(all="ignore"):
            r = pyref.comparer(self.tr, v, self.map[node])
        return po.dot_self(np.where(self.valid, r, f32(0)))


def phase1(tr, W, H, M, X, valid, lastbmu, is_first):
    """(lastBMU uint64[B], sqres float32[B]) of the masked phase 1; valid: bool[B, J]"""
    B, J = X.shape
    s = MaskedSearch(W, H, J, tr)
    s.map[...] = M
    lb = np.zeros(B, np.uint64)
    sq = np.zeros(B, f32)
    for r in range(B):
        s.valid = valid[r]
        idx = s.find_bmu(X[r]) if is_first else s.find_local_bmu(X[r], int(lastbmu[r]))
        lb[r] = idx
        sq[r] = s.dist(idx, X[r])
    return lb, sq


def phase2(tr, W, H, X, valid, lastbmu, sigma):
    """(map, sigmaMap float32[N, J], weightMap float32[N]) of the masked phase 2"""
    B, J = X.shape
    N = W * H
    newmap = np.zeros((N, J), f32)
    newsig = np.zeros((N, J), f32)
    col = po.OracleSom(W, H, 1, tr)
    for d in range(J):
        rows = np.flatnonzero(valid[:, d])
        xd = np.ascontiguousarray(X[rows, d:d + 1], dtype=f32).reshape(rows.size, 1)
        col.batch_phase2_range(xd, np.ascontiguousarray(lastbmu[rows], dtype=np.uint64), sigma, 0, N)
        newmap[:, d] = col.map[:, 0]
        newsig[:, d] = col.sigma[:, 0]
    # weightMap: the sum of w over ALL rows
    col.batch_phase2_range(np.zeros((B, 1), f32), np.ascontiguousarray(lastbmu, dtype=np.uint64), sigma, 0, N)
    weight = col.weight.copy()
    col.close()
    return newmap, newsig, weight


class MaskedOracle:
    """the state of a map trained by masked epochs: map, sigma, weight, hits (S is untouched in batch mode)"""

    def __init__(self, W, H, J, tr, init):
        self.W, self.H, self.J, self.tr = W, H, J, tr
        self.map = np.array(init, f32).reshape(W * H, J)
        self.sigma = np.zeros((W * H, J), f32)
        self.weight = np.zeros(W * H, f32)
        self.hits = np.zeros(W * H, np.uint64)

    def epoch(self, X, valid, lastbmu, sigma, is_first):
        """one masked epoch; lastbmu (uint64[B]) in / out; returns (mse, sqres)"""
        X = np.ascontiguousarray(X, dtype=f32)
        valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
        lb, sq = phase1(self.tr, self.W, self.H, self.map, X, valid, lastbmu, is_first)
        fin = po.OracleSom(self.W, self.H, self.J, self.tr)
        fin.set_state(hits=self.hits)
        mse = fin.batch_phase1_finish(lb, sq) if X.shape[0] else f32(0)
        self.hits = fin.hits.copy()
        fin.close()
        self.map, self.sigma, self.weight = phase2(self.tr, self.W, self.H, X, valid, lb, sigma)
        lastbmu[...] = lb
        return mse, sq
