"""CPU restatement of vsom_train_online_chunk_masked (no GPU), built on oracle/pyoracle.py and tests/pyref.py only.

OnlineMasked is pyref.Som with `dist` overridden by the masked distance (masked_train_ref.MaskedSearch: r_d = valid[d] ?
m_d - x_d : +0, the oracle's dot).  Per sample it
  runs the search (find_bmu for sigma > 1, find_local_bmu from lastBMU[j] otherwise) on that distance;
  runs pyref.Som.train_single's update with the search pinned to that BMU, on the row with its invalid entries replaced
  by 0 (weightMap moves as in the unmasked step);
  restores map, S and sigma at the invalid columns from a copy taken before the step;
  takes the masked distance to the updated BMU row for the MSE, and counts the hit.
pyref.Som.train_single is pinned to the oracle by tests/test_oracle_vs_pyref.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pyref  # noqa: E402
from masked_train_ref import MaskedSearch  # noqa: E402

f32 = np.float32


class OnlineMasked(MaskedSearch):
    """state: map, S, sigma, weight, hits (pyref.Som's); train_chunk is the masked chunk call"""

    pinned = None

    def find_bmu(self, v):
        return self.pinned if self.pinned is not None else super().find_bmu(v)

    def find_local_bmu(self, v, last):
        return self.pinned if self.pinned is not None else super().find_local_bmu(v, last)

    def set_state(self, map=None, sigma=None, S=None, weight=None, hits=None):
        for name, a in (("map", map), ("sigma", sigma), ("S", S), ("weight", weight), ("hits", hits)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).reshape(getattr(self, name).shape)

    def train_sample(self, x, valid, eta, sigma, last, fn):
        """one masked step; returns (bmu, masked distance to the updated BMU row)"""
        x = np.asarray(x, f32)
        valid = np.asarray(valid) != 0
        self.valid = valid
        self.pinned = None
        bmu = self.find_bmu(x) if sigma > 1 else self.find_local_bmu(x, int(last))
        keep = [a.copy() for a in (self.map, self.S, self.sigma)]
        self.pinned = bmu
        pyref.Som.train_single(self, np.where(valid, x, f32(0)), eta, sigma, int(last), fn)
        self.pinned = None
        for a, old in zip((self.map, self.S, self.sigma), keep):
            a[:, ~valid] = old[:, ~valid]
        return bmu, self.dist(bmu, x)

    def train_chunk(self, X, valid, lastbmu, eta, sigma, fn, mse_start=0.0):
        """B sequential masked steps; lastbmu (uint64[B]) in / out; valid: B x J or J; returns the running MSE"""
        X = np.asarray(X, f32)
        B = X.shape[0]
        valid = np.broadcast_to(np.asarray(valid) != 0, X.shape)
        mse = f32(mse_start)
        for j in range(B):
            bmu, dist = self.train_sample(X[j], valid[j], eta, sigma, lastbmu[j], fn)
            lastbmu[j] = bmu
            self.hits[bmu] += 1
            with np.errstate(all="ignore"):
                mse = f32(mse + f32(f32(dist) / f32(B)))
        return mse

    def snapshot(self, lastbmu, mse):
        return {"map": self.map.copy(), "S": self.S.copy(), "sigma": self.sigma.copy(), "weight": self.weight.copy(),
                "hits": self.hits.copy(), "lastbmu": np.array(lastbmu, np.uint64), "mse": np.array([mse], f32)}
