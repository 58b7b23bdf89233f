"""numpy fp32 restatement of the host path for custom hooks (host/src/vsom_custom.cpp: hostDist, hostFindBmu,
hostFindLocalBmu, hostBatchEpoch, hostTrainSingle) for the hooks of custom_validity_hooks.py, which use their
valueWeight argument.  Dot products are summed in Eigen's packet order (pyref.dot_self).  tests/test_custom_validity_ref.py
pins it against the bits of the host-lambda path itself (host_custom_validity_test)."""
import numpy as np

import pyref

f32 = np.float32
EXPONENTIAL, INVERSE_PROPORTIONAL = pyref.EXPONENTIAL, pyref.INVERSE_PROPORTIONAL


def dot_self_rows(R):
    """pyref.dot_self of every row of R (Eigen 3.4's Packet4f reduction order), the rows side by side"""
    R = np.asarray(R, f32)
    n = R.shape[1]
    with np.errstate(all="ignore"):
        p = (R * R).astype(f32)
        a2, a1 = (n // 8) * 8, (n // 4) * 4
        if not a1:
            res = p[:, 0].copy()
            for i in range(1, n):
                res = (res + p[:, i]).astype(f32)
            return res
        p0 = p[:, 0:4].copy()
        if a1 > 4:
            p1 = p[:, 4:8].copy()
            for i in range(8, a2, 8):
                p0 = (p0 + p[:, i:i + 4]).astype(f32)
                p1 = (p1 + p[:, i + 4:i + 8]).astype(f32)
            p0 = (p0 + p1).astype(f32)
            if a1 > a2:
                p0 = (p0 + p[:, a2:a2 + 4]).astype(f32)
        res = ((p0[:, 0] + p0[:, 2]).astype(f32) + (p0[:, 1] + p0[:, 3]).astype(f32)).astype(f32)
        for i in range(a1, n):
            res = (res + p[:, i]).astype(f32)
        return res


def compare(hook, x, model, disp, vw):
    """Comparer of custom_validity_hooks.SOURCES[hook] (J == D == R); model and disp may be several rows"""
    with np.errstate(all="ignore"):
        diff = (model - x).astype(f32)
        if hook == "standard":
            return diff
        if hook == "plain_select":
            r = diff
        else:
            r = (vw * diff).astype(f32)
            if hook == "scaled":
                r = (r / disp).astype(f32)
        return np.where(vw != 0, r, f32(0)).astype(f32)


def step(hook, x, model, vw):
    with np.errstate(all="ignore"):
        d = (x - model).astype(f32)
        return d if hook == "standard" else np.where(vw != 0, d, f32(0)).astype(f32)


def value_weights(valid, weights, rows, J):
    """(valid as 0.0f / 1.0f, valid * weights), both rows x J, from None / a J mask / a rows x J mask and None / J weights"""
    v = np.ones((rows, J), f32) if valid is None else np.broadcast_to((np.asarray(valid) != 0).astype(f32), (rows, J)).copy()
    w = np.ones(J, f32) if weights is None else np.asarray(weights, f32)
    with np.errstate(all="ignore"):
        return v, (v * w[None, :]).astype(f32)


class ValiditySom(pyref.Som):
    """pyref.Som whose distance, residual and steps go through a hook that takes value_weight; self.vw is the row the
    searches use (set by the callers below, as hostDist's validWeights is built per call)"""

    def __init__(self, W, H, J, hook):
        super().__init__(W, H, J, pyref.STANDARD)
        self.hook = hook
        self.vw = np.ones(J, f32)

    def set_state(self, map=None, sigma=None, S=None, weight=None, hits=None):
        for name, a in (("map", map), ("sigma", sigma), ("S", S), ("weight", weight), ("hits", hits)):
            if a is not None:
                getattr(self, name)[...] = np.asarray(a).reshape(getattr(self, name).shape)

    def dist(self, node, v):                          # hostDist: the floored sigmaMap, valid .* weights
        sg = self.sigma[node]
        floor = np.where(sg < f32(0.00001), f32(0.00001), sg).astype(f32)
        with np.errstate(all="ignore"):
            return pyref.dot_self(compare(self.hook, v, self.map[node], floor, self.vw))

    def find_bmu(self, v):                            # hostFindBmu, the distances of all nodes side by side
        floor = np.where(self.sigma < f32(0.00001), f32(0.00001), self.sigma).astype(f32)
        d = dot_self_rows(compare(self.hook, v[None, :], self.map, floor, self.vw[None, :]))
        best, bi = d[0], 0
        for i in range(1, len(d)):
            if d[i] < best:
                best, bi = d[i], i
        return bi

    # ---- searches of chunk rows / one vector ----
    def bmu_rows(self, X, vw, local_start=None):
        idx = np.zeros(len(X), np.uint64)
        dist = np.zeros(len(X), f32)
        for s, x in enumerate(X):
            self.vw = vw[s]
            idx[s] = self.find_bmu(x) if local_start is None else self.find_local_bmu(x, int(local_start[s]))
            dist[s] = self.dist(int(idx[s]), x)
        return idx, dist

    def dist_pairs(self, X, vw, nodes, rows):
        out = np.zeros(len(nodes), f32)
        for i, (n, r) in enumerate(zip(nodes, rows)):
            self.vw = vw[int(r)]
            out[i] = self.dist(int(n), X[int(r)])
        return out

    # ---- hostBatchEpoch: search with valid .* weights, residual (SMap rows) and Stepper with valid alone ----
    def batch_epoch(self, X, valid, vw, lastbmu, sigma, is_first):
        X = np.asarray(X, f32)
        B = X.shape[0]
        mse = f32(0)
        with np.errstate(all="ignore"):
            for s in range(B):
                self.vw = vw[s]
                idx = self.find_bmu(X[s]) if is_first else self.find_local_bmu(X[s], int(lastbmu[s]))
                lastbmu[s] = idx
                self.hits[idx] += 1
                res = compare(self.hook, X[s], self.map[idx], self.S[idx], valid[s])
                mse = f32(mse + f32(pyref.dot_self(res) / f32(B)))
            newmap = np.zeros_like(self.map)
            for node in range(self.W * self.H):
                cx, cy = self.somindex(node)
                total = f32(0)
                M = np.zeros(self.D, f32)
                S = np.zeros(self.D, f32)
                for j in range(B):
                    bx, by = self.somindex(int(lastbmu[j]))
                    w = f32(pyref.nbh(cx, cy, bx, by, sigma))
                    total = f32(total + w)
                    delta = step(self.hook, X[j], M, valid[j])
                    c = f32(w / total)
                    M = (M + (c * delta).astype(f32)).astype(f32)
                    S = (S + ((w * delta).astype(f32) * delta).astype(f32)).astype(f32)
                newmap[node] = M
                self.sigma[node] = np.sqrt((S / total).astype(f32)).astype(f32)
                self.weight[node] = total
        self.map[...] = newmap
        return mse

    # ---- hostTrainSingle: every hook call with vw = valid .* weights ----
    def train_single(self, v, vw, eta, sigma, last, fn):
        v = np.asarray(v, f32)
        W, H = self.W, self.H
        self.vw = vw
        bmu = self.find_bmu(v) if sigma > 1 else self.find_local_bmu(v, last)
        bx, by = bmu % W, bmu // W
        sx, sy = int(max(float(bx) - 2.5 * sigma, 0.0)), int(max(float(by) - 2.5 * sigma, 0.0))
        ex, ey = int(min(float(bx) + 2.5 * sigma, float(W))), int(min(float(by) + 2.5 * sigma, float(H)))
        with np.errstate(all="ignore"):
            for j in range(sy, ey):
                for i in range(sx, ex):
                    n = j * W + i
                    delta = step(self.hook, v, self.map[n], vw)
                    h = pyref.nbh(i, j, bx, by, sigma)
                    if fn == EXPONENTIAL:
                        self.weight[n] = f32(self.weight[n] + f32(h * eta))
                        k = f32(h * eta)
                    else:
                        self.weight[n] = f32(self.weight[n] + f32(h))
                        k = f32(1.0 if self.weight[n] == 0 else h / float(self.weight[n]))
                    self.map[n] = (self.map[n] + (k * delta).astype(f32)).astype(f32)
                    norm = f32(0.000001 if self.weight[n] == 0 else float(self.weight[n]))
                    after = step(self.hook, v, self.map[n], vw)
                    self.S[n] = (self.S[n] + (f32(h) * (delta * after).astype(f32)).astype(f32)).astype(f32)
                    self.sigma[n] = np.sqrt(np.abs((self.S[n] / norm).astype(f32))).astype(f32)
            res = compare(self.hook, v, self.map[bmu], self.sigma[bmu], vw)
        return bmu, res, self.dist(bmu, v), by * W + bx

    def train_chunk(self, X, vw, lastbmu, eta, sigma, fn, mse_start=0.0):
        mse = f32(mse_start)
        B = len(X)
        with np.errstate(all="ignore"):
            for s in range(B):
                bmu, res, _, last = self.train_single(X[s], vw[s], eta, sigma, int(lastbmu[s]), fn)
                lastbmu[s] = last
                self.hits[bmu] += 1
                mse = f32(mse + f32(pyref.dot_self(res) / f32(B)))
        return mse
