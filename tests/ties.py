"""Host-only generator of BMU tie cases (numpy and the CPU oracle, no GPU).

Every planted sample comes with a certificate taken from the oracle: the exact-order fp32 distances of the expected winner
and of the runner-up (OracleSom.dist), the same two distances in float64 (math.fsum of the exact squares), their gap in
fp32 ulps and the expected winner.  Kinds of case:

  mirror   x and m_a on a dyadic grid, m_b := 2x - m_a: every difference is exact, (x - m_a)_k = -(x - m_b)_k, so the two
           rows differ bit for bit but their distances are bit-equal -- the dedupe pass cannot merge them and the lower
           index must win
  ulp      a mirror pair with one value of one row moved by one ulp (np.nextafter): the distances differ by 0 to a few
           ulps; in `ulp_hi` cases the HIGHER index wins
  order    a mined perturbed pair whose fp32 exact-order winner is not its float64 winner (or that ties in float64 and
           not in fp32): only a search that sums in the reference's order gets it right

Samples are plain floats, integers in [0, 255] (the uint8 kind of the integer shortlist) or values around a large common
offset ("cancel": |M|^2 - 2<x, M> cancels and the bound's u (|M|^2 + |x|^2) term swamps the distances).  Pairs straddle
the boundaries the kernels use (see placements())."""
import math

import numpy as np

from oracle import pyoracle as po

KINDS = ("mirror", "ulp_lo", "ulp_hi", "order")


def eigen_sq(R):
    """vso_dot_self over the last axis of R, vectorised: Eigen 3.4's SSE reduction order in fp32 (oracle/vsom_oracle.c)"""
    R = np.asarray(R, np.float32)
    n = R.shape[-1]
    P = R * R
    if n < 4:
        res = P[..., 0].copy()
        for i in range(1, n):
            res = res + P[..., i]
        return res
    aligned2, aligned = n // 8 * 8, n // 4 * 4
    p0 = P[..., 0:4].copy()
    if aligned > 4:
        p1 = P[..., 4:8].copy()
        for i in range(8, aligned2, 8):
            p0 = p0 + P[..., i:i + 4]
            p1 = p1 + P[..., i + 4:i + 8]
        p0 = p0 + p1
        if aligned > aligned2:
            p0 = p0 + P[..., aligned2:aligned2 + 4]
    res = (p0[..., 0] + p0[..., 2]) + (p0[..., 1] + p0[..., 3])
    for i in range(aligned, n):
        res = res + P[..., i]
    return res


def clr_residual(M, x):
    """the CLR comparer (A .* x_i + B - x_j over the pairs i < j, lexicographic) of the rows of M, in fp32"""
    M = np.asarray(M, np.float32)
    J, P = x.size, M.shape[-1] // 2
    i, j = np.triu_indices(J, 1)
    i, j = i[:P], j[:P]
    return (M[..., :P] * x[i] + M[..., P:]) - x[j]


def residual(tr, M, x):
    return clr_residual(M, x) if tr == po.CLR else np.asarray(M, np.float32) - np.asarray(x, np.float32)


def dist32(tr, M, x):
    return eigen_sq(residual(tr, M, x))


def dist64(tr, m, x):
    """the exact distance rounded once to float64 (the residual itself is the fp32 comparer's)"""
    r = residual(tr, m[None, :], x)[0].astype(np.float64)
    return math.fsum((r * r).tolist())


def ulps(a, b):
    """b - a in fp32 ulps (both finite and >= 0)"""
    return int(np.float32(b).view(np.uint32)) - int(np.float32(a).view(np.uint32))


def placements(N, rs, count):
    """pairs (lo, hi) of distinct nodes: the boundaries first, then random pairs, far and near"""
    want = [(0, min(N - 1, 5)), (63, 64), (127, 128), (31, 32), (N - 2, N - 1), (7, N - 1), (64, 65), (100, 132),
            (200, 216), (17, 33), (190, 191), (3, N - 4), (255, 256), (320, 384), (512, 513), (N - 65, N - 64),
            (1, 64 * 7), (130, 140), (640, 641), (1023, 1024)]
    used, out = set(), []
    for a, b in want:
        if 0 <= a < b < N and a not in used and b not in used:
            out.append((a, b))
            used |= {a, b}
    while len(out) < count:
        a = int(rs.randint(0, N))
        b = a + int(rs.randint(1, 4)) if rs.rand() < 0.4 else int(rs.randint(0, N))
        a, b = min(a, b), max(a, b)
        if a == b or b >= N or a in used or b in used:
            continue
        out.append((a, b))
        used |= {a, b}
    return out[:count]


def _grid(rs, shape, step, lo, hi):
    return (np.round(rs.uniform(lo, hi, size=shape) / step) * step).astype(np.float32)


class Case:
    """one map and chunk with planted pairs; certs[s] describes sample s"""

    def __init__(self, tr, W, H, J, init, X, certs, name):
        self.tr, self.W, self.H, self.J = tr, W, H, J
        self.init, self.X, self.certs, self.name = init, X, certs, name
        self.repeat, self.decoys = 1, None

    def count(self, kind):
        return sum(1 for c in self.certs if c is not None and c["kind"] == kind)

    def order_decided(self):
        return sum(1 for c in self.certs if c is not None and c["order_decided"])

    def hi_wins(self):
        return sum(1 for c in self.certs if c is not None and c["winner"] == c["pair"][1] and c["gap_ulps"] > 0)

    def exact_ties(self):
        return sum(1 for c in self.certs if c is not None and c["gap_ulps"] == 0 and c["rows_differ"])


def _certify(tr, o, x, a, b, kind):
    """the certificate of a sample whose two nearest nodes are (a, b), from the oracle's state `o`"""
    da, db = np.float32(o.dist(a, x)), np.float32(o.dist(b, x))
    if b < a:
        a, b, da, db = b, a, db, da
    w, r = (a, b) if da <= db else (b, a)                  # strict <: the lower index wins a tie
    dw, dr = (da, db) if w == a else (db, da)
    e_a, e_b = dist64(tr, o.map[a], x), dist64(tr, o.map[b], x)
    w64 = a if e_a <= e_b else b
    return {"kind": kind, "pair": (a, b), "winner": int(w), "runner_up": int(r), "d32": (dw, dr),
            "d64": (e_a if w == a else e_b, e_b if w == a else e_a), "gap_ulps": ulps(dw, dr),
            "order_decided": bool(w64 != w or (e_a == e_b) != (da == db)),
            "rows_differ": bool((o.map[a].view(np.uint32) != o.map[b].view(np.uint32)).any())}


def _perturb(tr, x, ma, mb, kind, rs):
    """from the mirror rows (ma, mb) of x, rows giving `kind`; None when nothing was found"""
    if kind == "mirror":
        return ma, mb
    D = ma.size
    if kind in ("ulp_lo", "ulp_hi"):
        for _ in range(64):
            k, row = int(rs.randint(0, D)), int(rs.randint(0, 2))
            a, b = ma.copy(), mb.copy()
            t = (a, b)[row]
            t[k] = _bump(t[k], rs)
            d = dist32(tr, np.stack([a, b]), x)
            if (kind == "ulp_hi" and d[1] < d[0] and ulps(d[1], d[0]) <= 4) or \
               (kind == "ulp_lo" and d[0] <= d[1] and ulps(d[0], d[1]) <= 4):
                return a, b
        return None
    # order: several one-ulp moves on both rows until fp32 and float64 disagree
    for _ in range(400):
        a, b = ma.copy(), mb.copy()
        for t in (a, b):
            ks = rs.randint(0, D, size=int(rs.randint(1, 4)))
            for k in ks:
                t[k] = _bump(t[k], rs)
        d = dist32(tr, np.stack([a, b]), x)
        e_a, e_b = dist64(tr, a, x), dist64(tr, b, x)
        w32 = 0 if d[0] <= d[1] else 1
        w64 = 0 if e_a <= e_b else 1
        if w32 != w64 or (e_a == e_b) != (d[0] == d[1]):
            return a, b
    return None


def batch_case(W, H, J, B, seed, data="float", tr=po.STANDARD, name=None, spread=None, dead=(), repeat=1, decoys=0):
    """a map of W x H nodes and a chunk of B samples: every sample s has its own pair of nodes, mirrored about it and
    perturbed by the kind KINDS[s % 4], nearer to it than any other node.  data: "float" (values on a 2^-20 grid),
    "uint8" (integer samples in [0, 255]), "u8edge" (integer samples; every value of a pair's rows 7/16 of a digit step
    off the integer shortlist's grid, in opposite directions: see _u8edge) or "cancel" (values around offsets of
    1e3..1e4, spread ~1e-2).  dead: columns that are zero in every sample (retired by the column compaction).  repeat:
    the chunk is the B planted samples `repeat` times over.  decoys: up to this many near-tie rows per sample, each in a
    16-node tile of its own (sample s gets s * decoys // B of them), a little farther than the pair (see _add_decoys)."""
    rs = np.random.RandomState(seed)
    N = W * H
    assert 2 * B <= N
    if tr == po.CLR:
        return _clr_case(W, H, J, B, rs, name or f"clr_{W}x{H}x{J}")
    if data == "u8edge":
        return _u8edge(W, H, J, B, rs, name or f"u8edge_{W}x{H}x{J}", repeat)
    if data == "uint8":
        init = _grid(rs, (N, J), 2.0 ** -12, 0.0, 255.0)
        X = rs.randint(0, 256, size=(B, J)).astype(np.float32)
        dstep, dmax = 2.0 ** -12, spread or 3.0
    elif data == "cancel":
        # per column a binade [2^e, 2^(e+1)) with e in 10..12: x, m_a and 2x - m_a stay inside it (exact mirror)
        e = rs.randint(10, 13, size=J)
        base = (2.0 ** e) * rs.uniform(1.2, 1.8, size=J)
        ulp = 2.0 ** (e - 23)
        init = (np.round((base + rs.uniform(-1e-2, 1e-2, size=(N, J))) / ulp) * ulp).astype(np.float32)
        X = (np.round((base + rs.uniform(-1e-2, 1e-2, size=(B, J))) / ulp) * ulp).astype(np.float32)
        dstep, dmax = ulp, spread or 1.5e-3
    else:
        init = _grid(rs, (N, J), 2.0 ** -20, -1.0, 1.0)
        X = _grid(rs, (B, J), 2.0 ** -20, -1.0, 1.0)
        dstep, dmax = 2.0 ** -20, spread or 0.06
    X[:, list(dead)] = 0.0
    pairs = placements(N, rs, B)
    plan = []
    for s, (a, b) in enumerate(pairs):
        x = X[s]
        kind = "mirror" if data == "cancel" else KINDS[s % 4]
        for _ in range(8):
            d = np.round(rs.uniform(-dmax, dmax, size=J) / dstep) * dstep
            ma = (x.astype(np.float64) + d).astype(np.float32)
            mb = (2.0 * x.astype(np.float64) - ma.astype(np.float64)).astype(np.float32)
            assert (ma - x == -(mb - x)).all() and ((ma - x).astype(np.float64) == d).all()
            got = _perturb(tr, x, ma, mb, kind, rs)
            if got is not None:
                break
        if got is None:
            got, kind = (ma, mb), "mirror"
        init[a], init[b] = got
        plan.append((a, b, kind))
    if decoys:
        _add_decoys(init, X, plan, decoys, rs)
    certs = _certify_batch(tr, W, H, J, init, X, plan)
    case = Case(tr, W, H, J, init, X, certs, name or f"{data}_{W}x{H}x{J}")
    case.decoys = [s * decoys // B for s in range(B)] if decoys else None
    return _repeat(case, repeat)


def _repeat(case, repeat):
    case.repeat = repeat
    if repeat > 1:
        case.X = np.ascontiguousarray(np.tile(case.X, (repeat, 1)))
        case.certs = case.certs * repeat
        if getattr(case, "decoys", None):
            case.decoys = case.decoys * repeat
    return case


def _add_decoys(init, X, plan, decoys, rs):
    """sample s gets s * decoys // B rows that are copies of its pair's row a with its largest difference from x moved 512
    ulps farther: some thousand ulps farther than the pair, well inside the pruning bound, each in a 16-node tile of its own -- so the
    number of candidate tiles per sample runs from 2 to decoys + 2 across the chunk (around tmax = 64 of sl_pick_kernel)"""
    N = init.shape[0]
    used = np.zeros(N, bool)
    for a, b, _ in plan:
        used[a] = used[b] = True
    B = len(plan)
    for s, (a, b, _) in enumerate(plan):
        k = s * decoys // B
        tiles = [t for t in rs.permutation(N // 16) if not used[16 * t:16 * t + 16].all()][:k]
        assert len(tiles) == k
        for t in tiles:
            n = 16 * int(t) + int(np.nonzero(~used[16 * t:16 * t + 16])[0][0])
            row = init[a].copy()
            e = int(np.argmax(np.abs(row - X[s])))
            step = np.float32(np.inf) if row[e] >= X[s][e] else np.float32(-np.inf)
            for _ in range(512):
                row[e] = np.nextafter(row[e], step)
            init[n] = row
            used[n] = True


def _u8edge(W, H, J, B, rs, name, repeat):
    """integer samples (the uint8 kind of the integer shortlist) and mirror pairs whose rows sit at the edge of the digit
    grid: column 0 holds the row's largest value (in [128, 256): scale s = 4, digit step 2^-12, residual bound
    eps = 2^-13 for every row), every value of the lower node is x + n 2^-12 + 7 2^-16 (residual +7/8 eps), every value of
    the higher one x - n 2^-12 - 7 2^-16 (residual -7/8 eps).  The approximation then over-estimates the lower node's
    |M|^2 - 2<x, M> by 1.75 eps |x|_1 and under-estimates the higher one's by as much, while their exact distances tie:
    a select / pick threshold of less than 3.5 eps |x|_1 -- the bound's 2 * 2 eps |x|_1, halved -- drops the winner."""
    N = W * H
    init = np.concatenate([_grid(rs, (N, 1), 2.0 ** -12, 136.0, 240.0), _grid(rs, (N, J - 1), 2.0 ** -12, 0.0, 40.0)], 1)
    X = np.concatenate([rs.randint(140, 236, size=(B, 1)), rs.randint(2, 39, size=(B, J - 1))], 1).astype(np.float32)
    plan = []
    for s, (a, b) in enumerate(placements(N, rs, B)):
        d =rs.randint(-8, 8, size=J) * 2.0 ** -12 + 7 * 2.0 ** -16
        ma = (X[s].astype(np.float64) + d).astype(np.float32)
        mb = (X[s].astype(np.float64) - d).astype(np.float32)
        assert ((ma - X[s]).astype(np.float64) == d).all() and (mb - X[s] == -(ma - X[s])).all()
        init[a], init[b] = ma, mb
        plan.append((a, b, "mirror"))
    return _repeat(Case(po.STANDARD, W, H, J, init, X, _certify_batch(po.STANDARD, W, H, J, init, X, plan), name), repeat)


def _certify_batch(tr, W, H, J, init, X, plan):
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=init)
    # screen every other node in float64 (centred: no cancellation), then check the close ones in the exact order
    mu = np.concatenate([init, X]).astype(np.float64).mean(0) if tr != po.CLR else 0.0
    M64 = init.astype(np.float64) - mu
    nM = (M64 * M64).sum(1)
    certs = []
    for s0 in range(0, len(plan), 64):
        blk = plan[s0:s0 + 64]
        if tr != po.CLR:
            X64 = X[s0:s0 + len(blk)].astype(np.float64) - mu
            G = nM[None, :] - 2.0 * (X64 @ M64.T) + (X64 * X64).sum(1)[:, None]
        for t, (a, b, kind) in enumerate(blk):
            x = X[s0 + t]
            c = _certify(tr, o, x, a, b, kind)
            if tr == po.CLR:
                close = np.arange(W * H)
            else:
                close = np.nonzero(G[t] <= 1.01 * c["d64"][1] + 1e-9 * (nM.max() + 1.0))[0]
            close = close[(close != a) & (close != b)]
            c["margin_ok"] = bool((dist32(tr, o.map[close], x) > c["d32"][1]).all()) if close.size else True
            certs.append(c)
    o.close()
    return certs


def _clr_case(W, H, J, B, rs, name):
    """CLR rows A | B: x, A on a 1/16 grid, B on a 1/256 grid; the mirror keeps A and reflects the residual through the
    intercepts, B' = 2 (x_j - A x_i) - B, so r(m_b) = -r(m_a) exactly"""
    N = W * H
    D = po.length(po.CLR, J)
    P = D // 2
    i, j = np.triu_indices(J, 1)
    i, j = i[:P], j[:P]
    init = np.concatenate([_grid(rs, (N, P), 1 / 16, -1, 1), _grid(rs, (N, P), 1 / 256, -2, 2)], axis=1)
    X = _grid(rs, (B, J), 1 / 16, -2, 2)
    pairs = placements(N, rs, B)
    plan = []
    for s, (a, b) in enumerate(pairs):
        x = X[s]
        kind = KINDS[s % 4]
        A = _grid(rs, P, 1 / 16, -1, 1)
        r = _grid(rs, P, 1 / 256, -0.03, 0.03)               # the residual of m_a
        Ba = (x[j].astype(np.float64) - A * x[i].astype(np.float64) + r).astype(np.float32)
        Bb = (2.0 * (x[j].astype(np.float64) - A * x[i].astype(np.float64)) - Ba).astype(np.float32)
        ma, mb = np.concatenate([A, Ba]), np.concatenate([A, Bb])
        ra, rb = clr_residual(ma[None], x)[0], clr_residual(mb[None], x)[0]
        assert (ra == -rb).all() and (ra.astype(np.float64) == r).all()
        got = _perturb(po.CLR, x, ma, mb, kind, rs)
        if got is None:
            got, kind = (ma, mb), "mirror"
        init[a], init[b] = got
        plan.append((a, b, kind))
    return Case(po.CLR, W, H, J, init, X, _certify_batch(po.CLR, W, H, J, init, X, plan), name)


def _window(o, bmu, sigma):
    """the nodes Som::trainSingle updates around `bmu` (Som.cpp:899-903, truncating)"""
    W, H = o.width, o.height
    bx, by = bmu % W, bmu // W
    sx, sy = int(max(bx - 2.5 * sigma, 0.0)), int(max(by - 2.5 * sigma, 0.0))
    ex, ey = int(min(bx + 2.5 * sigma, float(W))), int(min(by + 2.5 * sigma, float(H)))
    return [y * W + x for y in range(sy, ey) for x in range(sx, ex)]


def _bump(v, rs):
    return np.nextafter(v, np.float32(np.inf) if rs.rand() < 0.5 else np.float32(-np.inf))


def online_case(W, H, J, B, sigma, eta, decay_fn, seed, tr=po.STANDARD, name=None):
    """one online chunk (sigma > 1: full searches) where every odd sample j meets a pair spanning both roles of the
    image-bounded search: node a, sample j-1's BMU (a window node, rewritten by sample j-1), and node b, never inside a
    window before sample j, set in the INITIAL map to the mirror of a's row after sample j-1 about x_j (or a one-ulp
    variant of it; only b's row is perturbed).  Even samples sit close to a random node, so the pairs stay the nearest
    rows.  certs[j] holds the certificate of an odd sample, None for the others; case.lb the lastBMU of the run that
    built it."""
    assert tr in (po.STANDARD, po.MEDIAN) and sigma > 1
    rs = np.random.RandomState(seed)
    N = W * H
    init = _grid(rs, (N, J), 2.0 ** -20, -1.0, 1.0)
    X = np.zeros((B, J), np.float32)
    certs = [None] * B
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=init)
    touched = np.zeros(N, bool)
    lbs = np.zeros(B, np.uint64)
    lb = np.zeros(1, np.uint64)
    mse = np.float32(0)
    kinds = ("mirror", "ulp_hi", "ulp_lo", "mirror", "ulp_hi", "order")
    dr = 0.012 if J >= 16 else 0.002                         # half-width of x_j - a (short rows: nodes lie closer)
    for j in range(B):
        free = np.nonzero(~touched)[0]
        a = int(lb[0])
        free = free[free != a]
        if j % 2 == 0 or free.size == 0:
            t = int(rs.randint(0, N))
            X[j] = (o.map[t] + _grid(rs, J, 2.0 ** -20, -dr / 6, dr / 6)).astype(np.float32)
        else:
            ma = o.map[a].copy()
            pref = [n for n in (0, 63, 64, 31, 32, 16, 127, 128, N - 1) if n < N and not touched[n] and n != a]
            b = int(pref[rs.randint(0, len(pref))] if pref and rs.rand() < 0.7 else free[rs.randint(0, free.size)])
            x = (ma + rs.uniform(-dr, dr, size=J).astype(np.float32)).astype(np.float32)
            mb = (2.0 * x.astype(np.float64) - ma.astype(np.float64)).astype(np.float32)
            exact = ((ma - x) == -(mb - x)) & ((ma - x).astype(np.float64) == ma.astype(np.float64) - x.astype(np.float64))
            x[~exact], mb[~exact] = ma[~exact], ma[~exact]
            kind = kinds[(j // 2) % len(kinds)]
            got = mb
            if kind != "mirror":
                got = None
                for _ in range(400):
                    nb = mb.copy()
                    for k in rs.randint(0, J, size=2 if kind == "order" else 1):
                        nb[k] = _bump(nb[k], rs)
                    d_a, d_b = dist32(tr, np.stack([ma, nb]), x)
                    e_a, e_b = dist64(tr, ma, x), dist64(tr, nb, x)
                    lo_d, hi_d = (d_a, d_b) if a < b else (d_b, d_a)
                    if (kind == "ulp_hi" and hi_d < lo_d and ulps(hi_d, lo_d) <= 4) or \
                       (kind == "ulp_lo" and lo_d < hi_d and ulps(lo_d, hi_d) <= 4) or \
                       (kind == "order" and ((d_a <= d_b) != (e_a <= e_b) or (e_a == e_b) != (d_a == d_b))):
                        got = nb
                        break
                if got is None:
                    got, kind = mb, "mirror"
            init[b] = got
            o.map[b] = got
            X[j] = x
            c = _certify(tr, o, x, a, b, kind)
            c["margin_ok"] = bool((np.delete(dist32(tr, o.map, x), [a, b]) > c["d32"][1]).all())
            c["window_node"], c["image_node"] = a, b
            certs[j] = c
        mse = o.train_online_chunk(X[j:j + 1], lb, eta, sigma, decay_fn, mse_start=float(mse))
        lbs[j] = lb[0]
        touched[_window(o, int(lb[0]), sigma)] = True
    final = o.map.copy()
    o.close()
    case = Case(tr, W, H, J, init, X, certs, name or f"online_{W}x{H}x{J}")
    case.sigma, case.eta, case.decay_fn, case.lb, case.final_map = sigma, eta, decay_fn, lbs, final
    return case


def online_edge_case(W, H, J, B, sigma, eta, seed, name=None):
    """an online chunk whose every sample meets a mirror pair of image nodes at the edge of the online image's digit grid
    (one int8 digit per value, q = rint(m / s)): column 0 holds each row's largest value, in [64, 128), so s = 1 for every
    row; the lower node is x + n + 31/64 in every value (residual +31/64), the higher one x - n - 31/64 (residual -31/64),
    x integers >= 0.  The image then over-estimates the lower node's d - |x|^2 by 31/32 |x|_1 and under-estimates the
    higher one's by as much while their exact distances tie; slack_n is about 2 |x|_1 max|r| = 31/32 |x|_1 as well, so an
    interval narrower than slack_n / 1.05 drops the winner.  Pair nodes are untouched by every earlier window;
    certs[j]["pair"] is sample j's pair.  sigma > 1: full searches, through the image under VSOM_BMU_SHORTLIST."""
    rs = np.random.RandomState(seed)
    N = W * H
    init = np.concatenate([_grid(rs, (N, 1), 1 / 64, 66.0, 126.0), _grid(rs, (N, J - 1), 1 / 64, 0.0, 30.0)], 1)
    X = np.concatenate([rs.randint(70, 121, size=(B, 1)), rs.randint(2, 29, size=(B, J - 1))], 1).astype(np.float32)
    o = po.OracleSom(W, H, J, po.STANDARD)
    o.set_state(map=init)
    touched = np.zeros(N, bool)
    lb = np.zeros(1, np.uint64)
    lbs, certs = np.zeros(B, np.uint64), []
    nref = -(-N // 32)
    strides = (1, 16, 32, nref, 64, 2 * nref)
    for j in range(B):
        stride = strides[j % len(strides)]
        free = [n for n in rs.permutation(N - stride) if not touched[n] and not touched[n + stride]]
        a = int(free[0])
        b = a + stride
        d = rs.randint(-2, 2, size=J) + 31 / 64
        ma = (X[j].astype(np.float64) + d).astype(np.float32)
        mb = (X[j].astype(np.float64) - d).astype(np.float32)
        assert ((ma - X[j]).astype(np.float64) == d).all() and (mb - X[j] == -(ma - X[j])).all()
        init[a], init[b] = ma, mb
        o.map[a], o.map[b] = ma, mb
        c = _certify(po.STANDARD, o, X[j], a, b, "mirror")
        c["margin_ok"] = bool((np.delete(dist32(po.STANDARD, o.map, X[j]), [a, b]) > c["d32"][1]).all())
        certs.append(c)
        o.train_online_chunk(X[j:j + 1], lb, eta, sigma, po.EXPONENTIAL)
        lbs[j] = lb[0]
        touched[_window(o, int(lb[0]), sigma)] = True
    final = o.map.copy()
    o.close()
    case = Case(po.STANDARD, W, H, J, init, X, certs, name or f"online_edge_{W}x{H}x{J}")
    case.sigma, case.eta, case.decay_fn, case.lb, case.final_map = sigma, eta, po.EXPONENTIAL, lbs, final
    return case


def replay_online(case):
    """the oracle's run of the whole chunk from the final initial map: lastBMU, running MSE and the oracle (open)"""
    o = po.OracleSom(case.W, case.H, case.J, case.tr)
    o.set_state(map=case.init)
    lb = np.zeros(case.X.shape[0], np.uint64)
    mse = o.train_online_chunk(case.X, lb, case.eta, case.sigma, case.decay_fn)
    return o, lb, mse


# the cases of tests/test_gpu_ties.py (tests/test_ties_generator.py checks what each one delivers):
# name -> (W, H, J, B, seed, keyword arguments of batch_case)
BATCH = {
    "float_40x36x24": (40, 36, 24, 200, 11, {}),
    "median_40x36x24": (40, 36, 24, 200, 12, {"tr": po.MEDIAN}),
    "u8_40x36x784": (40, 36, 784, 200, 13, {"data": "uint8"}),
    "general_40x36x784": (40, 36, 784, 200, 14, {}),
    # B = 2048 rows (256 planted, 8 times over): ceil(16384 / 128) * ceil(2048 / 256) = 1024 ring tiles, so the search
    # takes the G-less ring kernel (sl_i8_plan; ring_plan() below restates the rule)
    "u8_128x128x784": (128, 128, 784, 256, 15, {"data": "uint8", "repeat": 8}),
    "general_128x128x784": (128, 128, 784, 256, 16, {"repeat": 8}),
    "u8edge_128x128x784": (128, 128, 784, 256, 24, {"data": "u8edge", "repeat": 8}),
    # pairs at the edge of the digit grid through sl_select_kernel (G and 64-node tiles)
    "u8edge_40x36x784": (40, 36, 784, 200, 25, {"data": "u8edge"}),
    # 0 .. 127 near-tie decoy tiles per sample: sl_pick_kernel's tmax = 64 candidate tiles falls inside the chunk
    "tmax_64x64x32": (64, 64, 32, 48, 26, {"decoys": 128}),
    "k64_64x64x32": (64, 64, 32, 400, 17, {}),
    "dead_40x40x64": (40, 40, 64, 300, 18, {"dead": (0, 1, 2, 17, 18, 40, 41, 42, 43, 63)}),
    "dead_u8_40x40x64": (40, 40, 64, 300, 19, {"data": "uint8", "dead": (0, 5, 6, 7, 33, 63)}),
    "cancel_40x36x64": (40, 36, 64, 200, 20, {"data": "cancel"}),
    "clr_34x34x10": (34, 34, 10, 120, 21, {"tr": po.CLR}),
    "tiny_10x10x9": (10, 10, 9, 40, 22, {}),
    "tiny_32x32x4": (32, 32, 4, 120, 23, {"spread": 0.01}),
}
# name -> (W, H, J, B, sigma, eta, seed, transformation)
ONLINE = {
    "online_40x36x24": (40, 36, 24, 24, 1.5, 0.05, 31, po.STANDARD),
    "online_median_40x36x24": (40, 36, 24, 24, 1.5, 0.05, 32, po.MEDIAN),
    "online_10x10x9": (10, 10, 9, 16, 1.2, 0.05, 40, po.STANDARD),
    "online_32x32x4": (32, 32, 4, 16, 1.5, 0.05, 43, po.STANDARD),
}


RT_N, RT_S = 128, 256          # the ring kernel's tile (vsom_sl_i8.hip)


def ring_plan(N, B, K):
    """the form sl_i8_plan gives a search of B rows of K contracted columns over N nodes: 0 G + 64-node tiles,
    1 sl_k64 (16-node tiles, no G), 2 G-less ring kernel"""
    kp8 = (K + 63) // 64 * 64
    if kp8 == 64:
        return 1
    return 2 if kp8 <= 960 and -(-N // RT_N) * -(-B // RT_S) >= 256 else 0


def batch(name):
    W, H, J, B, seed, kw = BATCH[name]
    return batch_case(W, H, J, B, seed, name=name, **kw)


ONLINE_EDGE = {"online_edge_40x36x64": (40, 36, 64, 16, 1.5, 0.05, 35)}


def online_edge(name):
    W, H, J, B, sigma, eta, seed = ONLINE_EDGE[name]
    return online_edge_case(W, H, J, B, sigma, eta, seed, name=name)


def online(name, decay_fn=0):
    W, H, J, B, sigma, eta, seed, tr = ONLINE[name]
    return online_case(W, H, J, B, sigma, eta, decay_fn, seed, tr=tr, name=name)
