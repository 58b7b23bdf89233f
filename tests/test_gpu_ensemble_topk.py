"""GPU: vsom_ensemble_bmu_topk_batch / vsom_ensemble_bmu_topk_masked_batch -- the k best matching units of every row of
every member in one call, plain and over the valid columns, and the topographic error built on them.
Every output is held bit for bit (NaN equal to NaN) against two references: the single calls (vsom_bmu_topk_batch,
vsom_bmu_topk_masked_batch) on twin contexts that are no members, and the CPU restatement tests/topk_masked_ref.py (lists,
nvalid) over the oracle's distances -- bmd_masked_ref.masked_d for Standard / Median (the plain call: an all-valid mask and
min_hits = 0), OracleSom.dist for CLR.
Shapes where this kernel can go wrong rather than at workload size: rows of 3 values (no full packet of the 8-lane
distance), 9 (a scalar tail of 1), 13 (the 4-tail and a scalar tail), 37; maps of 5 x 3, 7 x 5, the 10 x 10 x 9 fixture, CLR
maps of 7 x 7 x 6 and 4 x 4 x 5, and one 12 x 12 x 30 member whose N * J = 4320 > 4096 takes the single call inside the
ensemble call; chunks of 1, 20 and 70 rows (two row tiles of 64, the second ragged: rows 64 .. 69 are the second row of
groups 0 .. 5 only); k of 1, 2, N (the whole ordering of the 5 x 3 map), 64 and a k above the candidate count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bmd_masked_ref as bmr  # noqa: E402
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402
import masked_score_ref as msr  # noqa: E402
import ties  # noqa: E402
import topk_masked_ref as tmr  # noqa: E402
from topk_masked_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
QNAN = tmr.QNAN32
STATE_KEYS = ("map", "S", "sigma", "weight", "hits")
PLAIN_KEYS = ("idx", "dist")
MASKED_KEYS = ("idx", "dist", "count", "nvalid")
# W, H, J, kind, rows, k, mask ("rows": rows x J bytes, "one": a column mask, None: skipped in the masked call), min_hits
SPECS = ((5, 3, 3, po.STANDARD, 1, 15, "rows", 0),          # k = N: the whole ordering
         (10, 10, 9, po.STANDARD, 20, 64, "rows", 3),
         (5, 3, 13, po.MEDIAN, 70, 2, "rows", 0),
         (10, 10, 9, po.MEDIAN, 20, 1, "one", 3),
         (7, 5, 37, po.STANDARD, 70, 7, "rows", 0),
         (7, 5, 9, po.STANDARD, 20, 30, "rows", 3),          # more than the candidates under min_hits = 3: padding
         (5, 3, 13, po.MEDIAN, 20, 4, "rows", 6),            # min_hits = 6: node 0 is the only candidate
         (12, 12, 30, po.STANDARD, 20, 5, "rows", 3),        # N * J = 4320: the single call, inside the ensemble call
         (10, 10, 9, po.STANDARD, 20, 2, None, 0),           # skipped in the masked call
         (5, 3, 9, po.MEDIAN, 0, 2, "rows", 0))              # no rows
CLR_SPECS = ((7, 7, 6, po.CLR, 20, 16, None, 0), (4, 4, 5, po.CLR, 70, 2, None, 0))
SLOW = 7                                                     # the member of SPECS off the fast path


def same(a, b, keys, what=None):
    for key in keys:
        if a[key] is None or b[key] is None:
            assert a[key] is None and b[key] is None, (what, key)
        else:
            assert beq(a[key], b[key]), (what, key)


def poisoned(X, valid, start=0):
    """X with NaN, +-inf, 1e30 and values outside [0, 1] at its invalid positions"""
    Xp = X.copy()
    inv = ~np.broadcast_to(valid, X.shape)
    Xp[inv] = np.resize(np.roll(np.array(msr.POISON, f32), start), int(inv.sum()))
    return Xp


class Member:
    """a member and its twin (the same state and chunk; the twin is driven by the single calls) with the member's
    arguments: k, valid (rows x J bool, J bool, or None: skipped in the masked call), min_hits"""

    def __init__(self, W, H, J, tr, X, M, hits, k, valid=None, min_hits=0):
        self.W, self.H, self.J, self.tr, self.N = W, H, J, tr, W * H
        self.X, self.M, self.hits = X, M, hits
        self.k, self.valid, self.min_hits = k, valid, min_hits
        self.m, self.t = self.context(), self.context()
        self._d = {}                                     # the reference distances, computed once

    def context(self):
        ctx = vsom_amd.Context(self.W, self.H, self.J, self.tr)
        ctx.set_state(map=self.M, hits=self.hits)
        ctx.upload_chunk(self.X)
        return ctx

    @property
    def rows(self):
        return self.X.shape[0]

    def twin_plain(self, k=None):
        idx, dist = self.t.bmu_topk(self.k if k is None else k)
        return {"idx": idx, "dist": dist}

    def twin_masked(self, k=None):
        return self.t.bmu_topk_masked(self.k if k is None else k, self.valid, min_hits=self.min_hits)

    def plain_d(self):
        """the oracle's distances of every row to every node"""
        if "plain" not in self._d:
            if self.tr == po.CLR:
                o = po.OracleSom(self.W, self.H, self.J, self.tr)
                o.set_state(map=self.M)
                with np.errstate(all="ignore"):
                    d = np.array([[o.dist(i, x) for i in range(self.N)] for x in self.X], f32)
            else:
                d = bmr.masked_d(self.tr, self.X, self.M, np.ones(self.J, bool))
            self._d["plain"] = d.reshape(self.rows, self.N)
        return self._d["plain"]

    def masked_d(self):
        if "masked" not in self._d:
            self._d["masked"] = bmr.masked_d(self.tr, self.X, self.M, self.valid).reshape(self.rows, self.N)
        return self._d["masked"]

    def cpu_plain(self, k=None):
        idx, dist, _ = tmr.lists(self.plain_d(), self.hits, 0, self.k if k is None else k)
        return {"idx": idx, "dist": dist}

    def cpu_masked(self, k=None):
        idx, dist, count = tmr.lists(self.masked_d(), self.hits, self.min_hits, self.k if k is None else k)
        return {"idx": idx, "dist": dist, "count": count, "nvalid": tmr.nvalid(self.valid, self.rows)}

    def close(self):
        self.m.close()
        self.t.close()


def clr_member(W, H, J, rows, k, seed):
    X = (np.abs(gen.blobs(rows, J, 4, seed, 2)) + 0.5).astype(f32)
    M = gen.random_map(W * H, po.length(po.CLR, J), seed=seed + 10)
    return Member(W, H, J, po.CLR, X, M, np.zeros(W * H, np.uint64), k)


def build(frac, seed, poison=True, specs=SPECS):
    """the members of `specs` with random masks of about `frac` invalid entries (poison stored at the invalid positions of
    the rows), hits 0 .. 5 with node 0 without hits"""
    mems = []
    for i, (W, H, J, tr, rows, k, how, min_hits) in enumerate(specs):
        if tr == po.CLR:
            mems.append(clr_member(W, H, J, rows, k, seed + 10 * i))
            continue
        M, _, hits = bmr.unit_state(W, H, J, seed + 10 * i)
        X = bmr.unit_rows(rows, J, seed + 10 * i + 1)
        rng = np.random.default_rng(seed + 10 * i + 2)
        valid = None if how is None else rng.random(J if how == "one" else (rows, J)) >= frac
        if how == "one":
            valid[J // 2] = True
        if poison and valid is not None:
            X = poisoned(X, valid, i)
        mems.append(Member(W, H, J, tr, X, M, hits, k, valid, min_hits))
    return mems


def plain_call(ens, mems, **kw):
    return ens.bmu_topk([m.k for m in mems], **kw)


def masked_call(ens, mems, **kw):
    return ens.bmu_topk_masked([m.k for m in mems], [m.valid for m in mems], [m.min_hits for m in mems], **kw)


def check_plain(mems, got, what, cpu=True):
    for i, m in enumerate(mems):
        assert got[i]["idx"].shape == (m.rows, m.k) and got[i]["dist"].shape == (m.rows, m.k), (what, i)
        if m.rows == 0:                                  # (the single call refuses a chunk without rows)
            continue
        same(got[i], m.twin_plain(), PLAIN_KEYS, (what, i, "twin"))
        if cpu:
            same(got[i], m.cpu_plain(), PLAIN_KEYS, (what, i, "CPU"))
        assert (got[i]["dist"].view(np.uint32)[np.isnan(got[i]["dist"])] == QNAN).all(), (what, i)


def check_masked(mems, got, what, cpu=True):
    for i, m in enumerate(mems):
        if m.valid is None:
            assert got[i] is None, (what, i)
            continue
        assert got[i]["idx"].shape == (m.rows, m.k) and got[i]["count"].shape == (m.rows,), (what, i)
        if m.rows == 0:
            continue
        same(got[i], m.twin_masked(), MASKED_KEYS, (what, i, "twin"))
        if cpu:
            same(got[i], m.cpu_masked(), MASKED_KEYS, (what, i, "CPU"))
        assert (got[i]["dist"].view(np.uint32)[np.isnan(got[i]["dist"])] == QNAN).all(), (what, i)


def close_all(ens, mems):
    ens.close()
    for m in mems:
        m.close()


# ---- 1. the plain call: every shape and kind in one ensemble (three launches) -------------------------------------------
def test_plain_every_shape_and_kind():
    mems = build(0.0, 100, poison=False, specs=SPECS + CLR_SPECS)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for i, m in enumerate(mems):
        want = m.rows > 0 and i != SLOW
        assert ens.topk_applies(i, m.k) == want, i
    got = plain_call(ens, mems)
    check_plain(mems, got, "plain")
    # the whole ordering of the 5 x 3 map is a permutation of its nodes
    assert sorted(got[0]["idx"][0].tolist()) == list(range(15))
    # entry 0 is vsom_ensemble_bmu_batch's answer on the bits
    idx, dist = ens.bmu_batch()
    for i, m in enumerate(mems):
        assert beq(got[i]["idx"][:, 0], idx[i]) and beq(got[i]["dist"][:, 0], dist[i]), i
    # without distances, and over a subset: the others are skipped
    sub = plain_call(ens, mems, dist=False, members=[1, SLOW, 10])
    for i, m in enumerate(mems):
        if i in (1, SLOW, 10):
            assert sub[i]["dist"] is None and beq(sub[i]["idx"], got[i]["idx"]), i
        else:
            assert sub[i] is None, i
    # another k per member in the same ensemble: 1 everywhere, then 2
    for k in (1, 2):
        for i, r in enumerate(ens.bmu_topk(k)):
            if mems[i].rows:
                same(r, mems[i].twin_plain(k), PLAIN_KEYS, ("k for all", k, i, "twin"))
                same(r, mems[i].cpu_plain(k), PLAIN_KEYS, ("k for all", k, i, "CPU"))
    close_all(ens, mems)


# ---- 2. the masked call: random masks, every shape in one ensemble (two launches) ---------------------------------------
@pytest.mark.parametrize("frac", [0.12, 0.6])
def test_masked_random_masks(frac):
    mems = build(frac, 200 + int(frac * 100))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for i, m in enumerate(mems):
        want = m.rows > 0 and i != SLOW
        assert ens.topk_applies(i, m.k, masked=True) == want, i
    got = masked_call(ens, mems)
    check_masked(mems, got, ("masked", frac))
    # padding: the members whose k exceeds their candidates hold NO_UNIT / the quiet NaN from entry count on
    for i in (5, 6):
        m, r = mems[i], got[i]
        cand = tmr.candidates(m.hits, m.min_hits).size
        assert cand < m.k and (r["count"] == cand).all(), i
        assert (r["idx"][:, cand:] == tmr.NO_UNIT).all() and (r["dist"][:, cand:].view(np.uint32) == QNAN).all(), i
        assert (r["idx"][:, :cand] != tmr.NO_UNIT).all(), i
    assert (got[6]["idx"][:, 0] == 0).all()                 # node 0 seeds without hits
    # the poison at the invalid positions of the rows reaches no output
    for i, m in enumerate(mems):
        if m.valid is not None and m.rows:
            real = got[i]["idx"] != tmr.NO_UNIT
            assert np.isfinite(got[i]["dist"][real]).all(), i
    # entry 0 is vsom_ensemble_bmu_masked_batch's answer on the bits
    first = ens.bmu_masked([m.valid for m in mems], [m.min_hits for m in mems])
    for i, m in enumerate(mems):
        if m.valid is not None:
            assert beq(got[i]["idx"][:, 0], first[i]["bmu"]) and beq(got[i]["dist"][:, 0], first[i]["dist"]), i
            assert beq(got[i]["nvalid"], first[i]["nvalid"]), i
    nod = masked_call(ens, mems, dist=False)
    for i, m in enumerate(mems):
        if m.valid is not None:
            assert nod[i]["dist"] is None
            same(nod[i], got[i], ("idx", "count", "nvalid"), ("no dist", i))
    close_all(ens, mems)


# ---- 3. the all-valid mask is the plain call ------------------------------------------------------------------------------
def test_all_valid_mask_equals_the_plain_call():
    mems = build(0.0, 300, poison=False)
    for m in mems:
        m.min_hits = 0
        m.valid = np.ones(m.J, bool) if m.valid is None or m.valid.ndim == 1 else np.ones((m.rows, m.J), bool)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    plain, masked = plain_call(ens, mems), masked_call(ens, mems)
    for i, m in enumerate(mems):
        same(plain[i], masked[i], PLAIN_KEYS, ("all valid", i))
        assert (masked[i]["nvalid"] == m.J).all() and (masked[i]["count"] == m.k).all(), i
    close_all(ens, mems)


# ---- 4. ties and near-ties ------------------------------------------------------------------------------------------------
def test_ties_and_near_ties():
    """mirror pairs (bit-equal distances of different rows: the lower index first), pairs a few ulps apart with the nearer
    one at the higher index (tests/ties.py, certified by the oracle), bit-identical model rows (each appears, in index
    order) and samples equal to a model row held twice (distance exactly 0, twice)"""
    cases = (ties.batch_case(10, 10, 9, 20, 5), ties.batch_case(7, 5, 13, 16, 6, tr=po.MEDIAN),
             ties.batch_case(7, 7, 6, 16, 7, tr=po.CLR))
    assert all(c.hi_wins() > 0 and c.exact_ties() > 0 for c in cases)
    mems = [Member(c.W, c.H, c.J, c.tr, c.X, c.init, np.zeros(c.W * c.H, np.uint64), 3) for c in cases]
    # a member of duplicates: nodes 2, 9, 20 hold one row, rows 0 and 69 of the chunk equal it
    M, _, hits = bmr.unit_state(7, 5, 13, 41)
    X = bmr.unit_rows(70, 13, 42)
    M[9] = M[20] = M[2]
    X[0] = X[69] = M[2]
    dup = Member(7, 5, 13, po.STANDARD, X, M, hits, 35, np.ones((70, 13), bool), 0)
    mems.append(dup)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got = plain_call(ens, mems)
    check_plain(mems, got, "ties")
    for i, c in enumerate(cases):
        for s, cert in enumerate(c.certs):
            if cert is None:
                continue
            assert int(got[i]["idx"][s, 0]) == cert["winner"] and int(got[i]["idx"][s, 1]) == cert["runner_up"], (i, s, cert)
            assert beq(got[i]["dist"][s, :2], np.array(cert["d32"], f32)), (i, s, cert)
    r = got[3]
    for s in (0, 69):
        assert r["idx"][s, :3].tolist() == [2, 9, 20] and (r["dist"][s, :3].view(np.uint32) == 0).all(), s
    for s in range(70):                                       # everywhere: the three copies side by side, in index order
        at = r["idx"][s].tolist().index(2)
        assert r["idx"][s, at:at + 3].tolist() == [2, 9, 20], s
        assert len(set(r["dist"][s, at:at + 3].view(np.uint32).tolist())) == 1, s
    # the masked call over the Standard / Median members: the same lists under an all-valid mask
    for m in mems:
        m.valid = None if m.tr == po.CLR else np.ones((m.rows, m.J), bool)
    masked = masked_call(ens, mems)
    for i, m in enumerate(mems):
        if m.valid is not None:
            same(masked[i], got[i], PLAIN_KEYS, ("ties, masked", i))
    close_all(ens, mems)


# ---- 5. NaN and infinity --------------------------------------------------------------------------------------------------
def nan_members():
    """0: a NaN at node 0 only, and an infinite node; 1: NaN at other nodes only, an infinite node, a NaN row (NaN at every
    node) and a row that is infinitely far from every node; 2: a NaN in every node's row; 3: a small map listed whole, with
    an infinite node and two NaN nodes"""
    mems = []
    c = 1
    for i, (W, H, J, tr, rows, k) in enumerate(((7, 5, 13, po.STANDARD, 70, 35), (10, 10, 9, po.MEDIAN, 20, 64),
                                                (5, 3, 9, po.STANDARD, 20, 15), (5, 3, 9, po.MEDIAN, 20, 15))):
        M, _, hits = bmr.unit_state(W, H, J, 500 + i)
        X = bmr.unit_rows(rows, J, 510 + i)
        valid = np.random.default_rng(520 + i).random((rows, J)) < 0.8
        valid[:, c] = True
        valid[3::7, c] = False                              # these rows do not see column c
        valid[:, 2] = True
        if i == 0:
            M[0, c] = np.nan
            M[7, 2] = 1e30                                  # (1e30)^2 overflows: +inf to every row
        elif i == 1:
            M[3, c] = M[9, c] = M[99, c] = np.nan
            M[5, 2] = 1e30
            X[2, 2] = np.nan                                # every node NaN for this row
            X[4, 2] = 3e38                                  # every node +inf for this row
        elif i == 2:
            M[:, c] = np.nan
        else:
            M[4, c] = M[11, c] = np.nan
            M[6, 2] = 1e30
        mems.append(Member(W, H, J, tr, X, M, hits, k, valid, 0))
    return mems


def test_nan_and_infinity_plain():
    mems = nan_members()
    own = [m.k for m in mems]
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for ks in ([1, 2, 2, 1], [2, 9, 1, 14], own):
        for m, k in zip(mems, ks):
            m.k = k
        got = plain_call(ens, mems)
        check_plain(mems, got, ("NaN, plain", ks))
        # node 0 NaN: entry 0 is node 0 with the quiet NaN
        for i in (0, 2):
            assert (got[i]["idx"][:, 0] == 0).all() and (got[i]["dist"][:, 0].view(np.uint32) == QNAN).all(), i
    a, b, c, d = got
    # member 0: behind the pinned node 0 every finite node, then the infinite one (k = N)
    assert (a["idx"][:, -1] == 7).all() and np.isinf(a["dist"][:, -1]).all() and np.isfinite(a["dist"][:, 1:-1]).all()
    # member 1: the NaN row lists the nodes in index order; the infinite row lists the nodes that are not NaN, in index order
    assert b["idx"][2].tolist() == list(range(64)) and (b["dist"][2].view(np.uint32) == QNAN).all()
    assert b["idx"][4].tolist() == [n for n in range(100) if n not in (3, 9, 99)][:64] and np.isinf(b["dist"][4]).all()
    # member 2: every node NaN: node order
    assert (c["idx"] == np.arange(15, dtype=np.uint64)).all() and (c["dist"].view(np.uint32) == QNAN).all()
    # member 3: +inf before NaN, the NaN nodes in index order at the very end
    assert (d["idx"][:, -3:] == np.array([6, 4, 11], np.uint64)).all() and np.isfinite(d["dist"][:, :-3]).all()
    assert np.isinf(d["dist"][:, -3]).all() and (d["dist"][:, -2:].view(np.uint32) == QNAN).all()
    idx, dist = ens.bmu_batch()
    for i in range(len(mems)):
        assert beq(got[i]["idx"][:, 0], idx[i]) and beq(got[i]["dist"][:, 0], dist[i]), i
    close_all(ens, mems)


def test_nan_and_infinity_masked():
    """the same members over their masks, poison (NaN, +-inf, 1e30) at every invalid position of the rows: a row that does
    not see column c does not see the NaN"""
    mems = nan_members()
    for i, m in enumerate(mems):
        m.X = poisoned(m.X, m.valid, i)
        m.min_hits = (0, 3, 0, 0)[i]
        for ctx in (m.m, m.t):
            ctx.upload_chunk(m.X)
    own = [m.k for m in mems]
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for ks in ([1, 2, 2, 1], own):
        for m, k in zip(mems, ks):
            m.k = k
        got = masked_call(ens, mems)
        check_masked(mems, got, ("NaN, masked", ks))
        for i in (0, 2):
            sees = mems[i].valid[:, 1]
            assert sees.any() and (~sees).any()
            assert (got[i]["idx"][sees, 0] == 0).all() and (got[i]["dist"][sees, 0].view(np.uint32) == QNAN).all(), i
            assert np.isfinite(got[i]["dist"][~sees, 0]).all(), i
        first = ens.bmu_masked([m.valid for m in mems], [m.min_hits for m in mems])
        for i in range(len(mems)):
            assert beq(got[i]["idx"][:, 0], first[i]["bmu"]) and beq(got[i]["dist"][:, 0], first[i]["dist"]), i
    d = got[3]
    sees = mems[3].valid[:, 1]
    assert (d["idx"][sees, -3:] == np.array([6, 4, 11], np.uint64)).all()      # +inf, then the NaN nodes
    assert (d["idx"][~sees, -1] == 6).all() and np.isfinite(d["dist"][~sees, :-1]).all()
    close_all(ens, mems)


# ---- 6. a row without a valid column; poison in the map under invalid columns ---------------------------------------------
def test_row_without_valid_column_and_poisoned_map():
    """rows 5 and 65 have no valid column: every distance is +0, the list is the first candidates in index order, nvalid 0.
    Columns that no row has valid hold NaN, +-inf and 1e30 in every node's map row: every output equals that of the clean
    map."""
    mems, clean = [], []
    for i, (W, H, J, tr, rows, k, one, mh) in enumerate(((7, 5, 13, po.STANDARD, 70, 7, False, 3),
                                                         (10, 10, 9, po.MEDIAN, 20, 64, True, 0))):
        M, _, hits = bmr.unit_state(W, H, J, 600 + i)
        X = bmr.unit_rows(rows, J, 610 + i)
        valid = np.random.default_rng(620 + i).random(J if one else (rows, J)) < 0.7
        dead = [1, J - 1]
        valid[..., dead] = False
        if not one:
            valid[5] = valid[65] = False
        Mp = M.copy()
        for j, c in enumerate(dead):
            Mp[:, c] = np.resize(np.roll(np.array(msr.POISON[:4], f32), j), M.shape[0])
        mems.append(Member(W, H, J, tr, poisoned(X, valid, i), Mp, hits, k, valid, mh))
        clean.append(M)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    dirty = masked_call(ens, mems)
    check_masked(mems, dirty, "poisoned map")
    a = dirty[0]
    cand = tmr.candidates(mems[0].hits, 3)[:7]
    for r in (5, 65):
        assert a["idx"][r].tolist() == cand.tolist() and (a["dist"][r].view(np.uint32) == 0).all(), r
        assert a["nvalid"][r] == 0 and a["count"][r] == 7, r
    for i, m in enumerate(mems):
        real = dirty[i]["idx"] != tmr.NO_UNIT
        assert np.isfinite(dirty[i]["dist"][real]).all(), i
    for m, M in zip(mems, clean):
        m.m.set_state(map=M)
    for i, r in enumerate(masked_call(ens, mems)):
        same(dirty[i], r, MASKED_KEYS, ("poisoned against clean", i))
    close_all(ens, mems)


# ---- 7. read-only ---------------------------------------------------------------------------------------------------------
def test_both_calls_are_read_only():
    mems = build(0.3, 700, specs=SPECS + CLR_SPECS)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    ens.bmu_batch()                                         # lastBMU and sqres hold the search's values
    for m in mems:
        if m.rows:
            m.t.bmu_batch()

    def snapshot():
        return [(m.m.get_state(), m.m.get_last_bmu(), m.m.get_sqres()) for m in mems]

    before = snapshot()
    plain_call(ens, mems)
    masked_call(ens, mems)
    masked_call(ens, mems, dist=False)
    for i, ((s0, l0, q0), (s1, l1, q1)) in enumerate(zip(before, snapshot())):
        for key in STATE_KEYS:
            assert beq(s0[key], s1[key]), (i, key)
        assert beq(l0, l1) and beq(q0, q1), i
    # ... and the chunk and lastBMU as an epoch sees them: a batch epoch made afterwards equals the twin's (the members
    # whose rows are clean: a poisoned row would only compare NaN with NaN)
    clean = [i for i, m in enumerate(mems) if m.rows and (m.valid is None or m.tr == po.CLR)]
    assert clean
    for i in clean:
        m = mems[i]
        assert m.m.batch_epoch(1.5, False) == m.t.batch_epoch(1.5, False), i
        m.t.sigma_flush()                                   # (a twin may leave its sigmaMap pending; a member never does)
        a, b = m.m.get_state(), m.t.get_state()
        for key in STATE_KEYS:
            assert beq(a[key], b[key]), (i, key)
    close_all(ens, mems)


# ---- 8. members on two streams --------------------------------------------------------------------------------------------
def test_members_on_two_streams():
    import torch
    mems = build(0.3, 800, specs=SPECS + CLR_SPECS)
    dev = torch.device("cuda", 0)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for m in mems:
        m.m.set_stream(s0.cuda_stream)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    one = (plain_call(ens, mems), masked_call(ens, mems))
    ens.close()
    for i, m in enumerate(mems):
        m.m.set_stream((s1 if i % 2 else s0).cuda_stream)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    two = (plain_call(ens, mems), masked_call(ens, mems))
    for i, m in enumerate(mems):
        same(one[0][i], two[0][i], PLAIN_KEYS, ("two streams", i))
        if m.valid is None:
            assert one[1][i] is None and two[1][i] is None
        else:
            same(one[1][i], two[1][i], MASKED_KEYS, ("two streams, masked", i))
    check_plain(mems, two[0], "two streams", cpu=False)
    check_masked(mems, two[1], "two streams", cpu=False)
    ens.close()
    for m in mems:
        m.m.synchronize()
        m.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member_and_change_nothing():
    mems = build(0.3, 900, specs=SPECS[:5])
    n = len(mems)
    L = capi.lib()
    u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    valid = [np.ascontiguousarray(np.broadcast_to(m.valid, m.X.shape), dtype=np.uint8) for m in mems]
    idx = [np.zeros((m.rows, 64), np.uint64) for m in mems]

    def arrays(ks):
        outs = (capi.EnsembleTopkOut * len(ks))()
        for i in range(len(ks)):
            outs[i].idx = idx[i % n].ctypes.data_as(u64p)
        return (C.c_uint32 * len(ks))(*ks), (u8p * n)(*[v.ctypes.data_as(u8p) for v in valid]), outs

    def refused(rc, *patterns):
        assert rc == -1, rc                                 # VSOM_ERR_INVALID
        msg = L.vsom_last_error().decode()
        for p in patterns:
            assert p in msg, msg

    ens = vsom_amd.Ensemble([m.m for m in mems])
    before = [(m.m.get_state(), m.m.get_last_bmu(), m.m.get_sqres()) for m in mems]
    good = [m.k for m in mems]
    kp, vp, outs = arrays(good)
    refused(L.vsom_ensemble_bmu_topk_batch(None, kp, outs), "null ensemble")
    refused(L.vsom_ensemble_bmu_topk_masked_batch(None, kp, None, vp, None, outs), "null ensemble")
    refused(L.vsom_ensemble_bmu_topk_batch(ens._h, None, outs), "null k")
    refused(L.vsom_ensemble_bmu_topk_masked_batch(ens._h, None, None, vp, None, outs), "null k")
    refused(L.vsom_ensemble_bmu_topk_batch(ens._h, kp, None), "null out")
    refused(L.vsom_ensemble_bmu_topk_masked_batch(ens._h, kp, None, vp, None, None), "null out")
    refused(L.vsom_ensemble_bmu_topk_masked_batch(ens._h, kp, None, None, None, outs), "null valid_host")
    assert L.vsom_ensemble_topk_applies(None, 0, 2, 0) == -1 and L.vsom_ensemble_topk_applies(ens._h, n, 2, 0) == -1
    for at, bad in ((3, 0), (1, 65), (2, 16), (4, 36)):    # k = 0, k = 65, k = N + 1 (the 5 x 3 and the 7 x 5 map)
        ks = list(good)
        ks[at] = bad
        kp, vp, outs = arrays(ks)
        refused(L.vsom_ensemble_bmu_topk_batch(ens._h, kp, outs), f"member {at}: k must be in [1, min(64, N)]")
        refused(L.vsom_ensemble_bmu_topk_masked_batch(ens._h, kp, None, vp, None, outs),
                f"member {at}: k must be in [1, min(64, N)]")
        assert not ens.topk_applies(at, bad) and not ens.topk_applies(at, bad, masked=True)
        # ... a member that is not covered may hold any k
        outs[at].idx = u64p()
        vp[at] = u8p()
        assert L.vsom_ensemble_bmu_topk_batch(ens._h, kp, outs) == 0
        assert L.vsom_ensemble_bmu_topk_masked_batch(ens._h, kp, None, vp, None, outs) == 0
    kp, vp, outs = arrays(good)
    outs[2].idx = u64p()
    refused(L.vsom_ensemble_bmu_topk_masked_batch(ens._h, kp, None, vp, None, outs), "member 2: out->idx is null")
    ens.close()

    # a member the calls do not take -- CLR in the masked call, custom, without a chunk -- is refused when covered, by name,
    # and skipped when not
    clr = clr_member(4, 4, 5, 8, 2, 3)
    d, r = hooks.shape("standard", 9)
    custom = capi.Context(5, 3, 9, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    custom.upload_chunk(bmr.unit_rows(8, 9, 2))
    fresh = vsom_amd.Context(5, 3, 9)
    for odd, rows, J, why, plain_too in ((clr.m, 8, 5, "CLR contexts are not supported", False),
                                         (custom, 8, 9, "custom contexts are not supported", True),
                                         (fresh, 1, 9, "no chunk loaded", True)):
        e2 = vsom_amd.Ensemble([mems[1].m, mems[2].m, odd])
        keep = [valid[1], valid[2], np.ones((rows, J), np.uint8)]
        vp3 = (u8p * 3)(*[a.ctypes.data_as(u8p) for a in keep])
        ks3 = (C.c_uint32 * 3)(mems[1].k, mems[2].k, 2)
        o3 = (capi.EnsembleTopkOut * 3)()
        for i in range(3):
            o3[i].idx = idx[i].ctypes.data_as(u64p)
        refused(L.vsom_ensemble_bmu_topk_masked_batch(e2._h, ks3, None, vp3, None, o3), "member 2", why)
        if plain_too:
            refused(L.vsom_ensemble_bmu_topk_batch(e2._h, ks3, o3), "member 2", why)
        got = e2.bmu_topk_masked([mems[1].k, mems[2].k, 2], [mems[1].valid, mems[2].valid, None],
                                 [mems[1].min_hits, mems[2].min_hits, 0])
        assert got[2] is None
        same(got[0], mems[1].twin_masked(), MASKED_KEYS, ("beside", why))
        same(got[1], mems[2].twin_masked(), MASKED_KEYS, ("beside", why))
        got = e2.bmu_topk([mems[1].k, mems[2].k, 2], members=[0, 1])
        assert got[2] is None
        same(got[0], mems[1].twin_plain(), PLAIN_KEYS, ("beside, plain", why))
        e2.close()
    clr.close()
    for ctx in (custom, fresh):
        ctx.close()

    # nothing changed: the state is what it was, and a legal call on the first ensemble's members gives the right answer
    for i, m in enumerate(mems):
        s0, l0, q0 = before[i]
        s1 = m.m.get_state()
        for key in STATE_KEYS:
            assert beq(s0[key], s1[key]), (i, key)
        assert beq(l0, m.m.get_last_bmu()) and beq(q0, m.m.get_sqres()), i
    ens = vsom_amd.Ensemble([m.m for m in mems])
    check_plain(mems, plain_call(ens, mems), "after the refusals")
    check_masked(mems, masked_call(ens, mems), "after the refusals")
    close_all(ens, mems)


def test_a_chunk_staged_ahead_is_refused():
    """a map whose batch epoch frees the staged rows early, so that a prefetch stages the next chunk over them (the shape of
    tests/test_gpu_ensemble_masked_query.py's case): both calls refuse the member by name, as the single calls refuse its
    twin, the other member is untouched, and after the commit both answer what the twins answer"""
    W = H = 48
    J, rows = 196, 1100
    xs = [gen.mnist_like(rows, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * f32(100) + f32(100)).astype(f32)
    _, _, hits = bmr.unit_state(W, H, J, 4)
    big = Member(W, H, J, po.STANDARD, xs[0], init, hits, 2, np.random.default_rng(5).random((rows, J)) < 0.7)
    small = build(0.3, 1200, specs=SPECS[1:2])[0]
    pin = capi.PinnedBuffer(xs[1].shape)
    pin.array[...] = xs[1]
    ens = vsom_amd.Ensemble([small.m, big.m])
    for ctx in (big.m, big.t):
        ctx.batch_epoch_async(10.0, True)
        ctx.prefetch_chunk(pin.array)                       # staged beside the chains of chunk 0
    before = (small.m.get_state(), small.m.get_last_bmu(), small.m.get_sqres())
    with pytest.raises(vsom_amd.VsomError, match="staged ahead"):
        big.twin_plain()
    with pytest.raises(vsom_amd.VsomError, match="staged ahead"):
        big.twin_masked()
    mems = [small, big]
    with pytest.raises(vsom_amd.VsomError, match="member 1: the next chunk is staged ahead"):
        plain_call(ens, mems)
    with pytest.raises(vsom_amd.VsomError, match="member 1: the next chunk is staged ahead"):
        masked_call(ens, mems)
    after = (small.m.get_state(), small.m.get_last_bmu(), small.m.get_sqres())
    for key in STATE_KEYS:
        assert beq(before[0][key], after[0][key]), key
    assert beq(before[1], after[1]) and beq(before[2], after[2])
    only_small = ens.bmu_topk([small.k, 2], members=[0])     # the member that is not covered does not stop the call
    same(only_small[0], small.twin_plain(), PLAIN_KEYS, "beside a staged-ahead member")
    for ctx in (big.m, big.t):
        ctx.commit_chunk()
    big.X = xs[1]
    assert not ens.topk_applies(1, 2) and ens.topk_applies(0, small.k)
    check_plain(mems, plain_call(ens, mems), "after the commit", cpu=False)
    check_masked(mems, masked_call(ens, mems), "after the commit", cpu=False)
    ens.close()
    big.m.synchronize()
    for m in mems:
        m.close()
    pin.free()


# ---- 10. the topographic error --------------------------------------------------------------------------------------------
def test_topographic_error_of_every_member():
    mems = build(0.3, 1000, specs=SPECS + CLR_SPECS)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    te = ens.topographic_error()
    assert te.dtype == np.float64 and te.shape == (len(mems),)
    for i, m in enumerate(mems):
        if m.rows == 0:
            assert np.isnan(te[i]), i
        else:
            assert te[i] == vs.topographic_error(m.twin_plain(2)["idx"], m.W), i
    assert 0 < np.nanmax(te) <= 1
    tem, counted = ens.topographic_error_masked([m.valid for m in mems], [m.min_hits for m in mems])
    assert tem.dtype == np.float64 and counted.shape == (len(mems),)
    for i, m in enumerate(mems):
        if m.rows == 0 or m.valid is None:
            assert np.isnan(tem[i]) and counted[i] == 0, i
            continue
        rep = m.twin_masked(2)
        keep = (rep["nvalid"] >= 1) & (rep["count"] >= 2)
        assert counted[i] == int(keep.sum()) and tem[i] == vs.topographic_error(rep["idx"][keep], m.W), i
    assert counted[6] == 0 and tem[6] == 0.0                # min_hits = 6: no row has a second unit
    assert counted[1] == mems[1].rows
    # a map of one node has no topographic error
    one = vsom_amd.Context(1, 1, 3)
    one.upload_chunk(bmr.unit_rows(4, 3, 1))
    e2 = vsom_amd.Ensemble([mems[2].m, one])
    te2 = e2.topographic_error()
    assert te2[0] == te[2] and np.isnan(te2[1])
    tem2, c2 = e2.topographic_error_masked([mems[2].valid, np.ones(3, bool)])
    assert np.isnan(tem2[1]) and c2[1] == 0 and c2[0] > 0
    e2.close()
    one.close()
    close_all(ens, mems)
