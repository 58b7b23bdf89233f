"""GPU: vsom_ensemble_bmu_masked_batch / vsom_ensemble_similarity_masked_batch -- every member's chunk searched over its
valid columns, imputed and scored in one call.  Every output is held bit for bit (NaN equal to NaN)
against two references: the single calls (vsom_bmu_masked_batch, vsom_similarity_masked_batch) on twin contexts that are no
members, and the CPU restatements of tests/masked_score_ref.py (the masked search, similarity_ref with delta NaN at invalid
columns; fill restated here: x where valid, the unit's row where not).
Shapes where this kernel can go wrong rather than at workload size: rows of 3 values (no full packet of the 8-lane
distance), 9 (a scalar tail of 1), 13 (the 4-tail and a scalar tail), 37; maps of 5 x 3 (non-square), 7 x 5, the 10 x 10 x 9
fixture, and one 12 x 12 x 30 member whose N * J = 4320 > 4096 takes the single call inside the ensemble call; chunks of 1,
20 and 70 rows (two row tiles of 64, the second ragged; 70 rows are also no multiple of the 4 wavefronts that share a
tile's epilogue); Standard and Median members in one ensemble (two launches); a skipped member, a member with a column
mask beside per-row masks, a member without rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402
import masked_score_ref as ref  # noqa: E402
import similarity_ref as sr  # noqa: E402
from similarity_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
RULES = ((capi.SIGMA_AS_WRITTEN, False), (capi.SIGMA_FLOOR, True))
BMU_KEYS = ("bmu", "dist", "nvalid", "fill")
SIM_KEYS = ("bmu", "dist", "nvalid") + ref.ROW_KEYS + ("delta",)
STATE_KEYS = ("map", "S", "sigma", "weight", "hits")
# W, H, J, kind, rows, mask ("rows": rows x J bytes, "one": a column mask, None: the member is skipped), min_hits, num_sigmas
SPECS = ((5, 3, 3, po.STANDARD, 1, "rows", 0, 3),
         (10, 10, 9, po.STANDARD, 20, "rows", 3, 2),
         (5, 3, 13, po.MEDIAN, 70, "rows", 0, 3),
         (10, 10, 9, po.MEDIAN, 20, "one", 2, 1),
         (7, 5, 37, po.STANDARD, 70, "rows", 3, 3),
         (12, 12, 30, po.STANDARD, 20, "rows", 2, 2),      # N * J = 4320: the single call, inside the ensemble call
         (10, 10, 9, po.STANDARD, 20, None, 0, 3),          # skipped
         (5, 3, 9, po.MEDIAN, 0, "rows", 0, 3))             # no rows


def same(a, b, keys, what=None):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
        else:
            assert beq(a[k], b[k]), (what, k)


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


def special_sigmas():
    """the sigma values of tests/test_gpu_similarity.py's engineered case, restated: below, at and above 1e-5, NaN, ..."""
    e = f32(0.00001)
    return np.array([0.0, 1e-42, 1.4e-45, e, np.nextafter(e, f32(1)), np.nextafter(e, f32(0)), np.nan, np.inf, -1.0, -0.0,
                     0.5, 3.0e-6, 2.0, 1e-30, -np.inf, 7.0e-3], f32)


def poisoned(X, valid, start=0):
    """X with NaN, +-inf, 1e30 and values outside [0, 1] at its invalid positions"""
    Xp = X.copy()
    inv = ~np.broadcast_to(valid, X.shape)
    Xp[inv] = np.resize(np.roll(np.array(ref.POISON, f32), start), int(inv.sum()))
    return Xp


class Member:
    """a member and its twin (the same state and chunk; the twin is driven by the single calls) with the member's
    arguments: valid (rows x J bool, J bool, or None: skipped), min_hits, num_sigmas"""

    def __init__(self, W, H, J, tr, X, M, S, hits, valid, min_hits=0, ns=3):
        self.W, self.H, self.J, self.tr = W, H, J, tr
        self.X, self.M, self.S, self.hits = X, M, S, hits
        self.valid, self.min_hits, self.ns = valid, min_hits, ns
        self.m, self.t = self.context(), self.context()

    def context(self):
        ctx = vsom_amd.Context(self.W, self.H, self.J, self.tr)
        ctx.set_state(map=self.M, sigma=self.S, hits=self.hits)
        ctx.upload_chunk(self.X)
        return ctx

    @property
    def rows(self):
        return self.X.shape[0]

    def twin_bmu(self, fill=True):
        return self.t.bmu_masked(self.valid, min_hits=self.min_hits, fill=fill)

    def twin_similarity(self, rule, delta=True):
        return self.t.similarity_masked(self.valid, self.min_hits, self.ns, rule, delta=delta)

    def cpu(self, floor):
        """the CPU restatement of both calls: (search dict with fill, similarity dict)"""
        bmu, dist = ref.checker(self.tr, self.X, self.M, self.valid, self.hits, self.min_hits)
        b = bmu.astype(np.int64)
        v = np.broadcast_to(self.valid, self.X.shape)
        nvalid = v.sum(axis=1).astype(np.uint32)
        search = {"bmu": bmu, "dist": dist, "nvalid": nvalid, "fill": np.where(v, self.X, self.M[b]).astype(f32)}
        rep = ref.similarity(self.X, self.M[b], self.S[b], self.ns, floor, self.valid)
        rep.update(bmu=bmu, dist=dist, nvalid=nvalid)
        return search, rep

    def close(self):
        self.m.close()
        self.t.close()


def build(frac, seed, poison=True, specs=SPECS):
    """the members of SPECS with random masks of about `frac` invalid entries, poison stored at the invalid positions"""
    mems = []
    for k, (W, H, J, tr, rows, how, min_hits, ns) in enumerate(specs):
        M, S, hits = unit_state(W, H, J, seed + 10 * k)
        X = unit_rows(rows, J, seed + 10 * k + 1)
        rng = np.random.default_rng(seed + 10 * k + 2)
        valid = None if how is None else rng.random(J if how == "one" else (rows, J)) >= frac
        if how == "one":
            valid[J // 2] = True
        if poison and valid is not None:
            X = poisoned(X, valid, k)
        mems.append(Member(W, H, J, tr, X, M, S, hits, valid, min_hits, ns))
    return mems


def ensemble_calls(ens, mems, rule, fill=True, delta=True):
    return (ens.bmu_masked([m.valid for m in mems], [m.min_hits for m in mems], fill=fill),
            ens.similarity_masked([m.valid for m in mems], [m.min_hits for m in mems], [m.ns for m in mems], rule, delta=delta))


def check_against_twins(mems, got_b, got_s, rule, what, fill=True, delta=True):
    for k, m in enumerate(mems):
        if m.valid is None:
            assert got_b[k] is None and got_s[k] is None, (what, k)
            continue
        assert got_b[k]["bmu"].shape == (m.rows,) and got_s[k]["bmu"].shape == (m.rows,), (what, k)
        if m.rows == 0:                                  # (the single calls refuse a chunk without rows)
            assert got_b[k]["fill"] is None or got_b[k]["fill"].shape == (0, m.J)
            continue
        same(got_b[k], m.twin_bmu(fill), BMU_KEYS, (what, k, "search"))
        same(got_s[k], m.twin_similarity(rule, delta), SIM_KEYS, (what, k, "similarity", rule))


def check_against_cpu(mems, got_b, got_s, floor, what):
    for k, m in enumerate(mems):
        if m.valid is None or m.rows == 0:
            continue
        search, rep = m.cpu(floor)
        same(got_b[k], search, BMU_KEYS, (what, k, "search, CPU"))
        same(got_s[k], rep, SIM_KEYS, (what, k, "similarity, CPU"))


def close_all(ens, mems):
    ens.close()
    for m in mems:
        m.close()


# ---- 1. random masks, every shape in one ensemble ------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.1, 0.6])
def test_random_masks(frac):
    mems = build(frac, 100 + int(frac * 10))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    # the mask matters: on the zero-filled rows the unmasked search finds other units (the CPU checker alone shows it)
    moved = 0
    for m in mems:
        if m.valid is None or m.rows == 0:
            continue
        v = np.broadcast_to(m.valid, m.X.shape)
        X0 = np.where(v, m.X, f32(0)).astype(f32)
        unmasked = ref.checker(m.tr, X0, m.M, np.ones(m.J, bool), m.hits, m.min_hits)[0]
        masked = ref.checker(m.tr, X0, m.M, m.valid, m.hits, m.min_hits)[0]
        moved += int((unmasked != masked).sum())
    assert moved > 0
    for rule, floor in RULES:
        got_b, got_s = ensemble_calls(ens, mems, rule)
        check_against_twins(mems, got_b, got_s, rule, ("random", frac))
        check_against_cpu(mems, got_b, got_s, floor, ("random", frac))
        # the poison at the invalid positions of x reaches no output, fill included
        for k, m in enumerate(mems):
            if m.valid is None or m.rows == 0:
                continue
            assert np.isfinite(got_b[k]["dist"]).all() and np.isfinite(got_b[k]["fill"]).all(), k
            assert np.isfinite(got_s[k]["delta"]).all() and np.isfinite(got_s[k]["amax"]).all(), k
            assert (got_s[k]["delta"][~np.broadcast_to(m.valid, m.X.shape)].view(np.uint32) == 0).all(), k
    # without the dense outputs: the same words, no fill and no delta
    got_b, got_s = ensemble_calls(ens, mems, capi.SIGMA_FLOOR, fill=False, delta=False)
    check_against_twins(mems, got_b, got_s, capi.SIGMA_FLOOR, ("random, no dense output", frac), fill=False, delta=False)
    assert all(r is None or r["fill"] is None for r in got_b) and all(r is None or r["delta"] is None for r in got_s)
    imp = ens.impute([m.valid for m in mems], [m.min_hits for m in mems])
    for k, m in enumerate(mems):
        if m.valid is None:
            assert imp[k] is None
        elif m.rows:
            assert beq(imp[k], m.twin_bmu()["fill"]), k
    close_all(ens, mems)


# ---- 2. the all-valid mask is the unmasked ensemble search ---------------------------------------------------------------
def test_all_valid_equals_bmu_batch():
    mems = build(0.0, 300, poison=False)
    for m in mems:
        m.min_hits = 0
        if m.valid is None:
            m.valid = np.ones(m.J, bool)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got_b, got_s = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    idx, dist = ens.bmu_batch()
    for k, m in enumerate(mems):
        assert beq(got_b[k]["bmu"], idx[k]) and beq(got_b[k]["dist"], dist[k]), k
        assert beq(got_s[k]["bmu"], idx[k]) and beq(got_s[k]["dist"], dist[k]), k
        assert (got_b[k]["nvalid"] == m.J).all() and beq(got_b[k]["fill"], m.X), k
        if m.rows:
            same(got_s[k], m.t.similarity(0, m.ns, capi.SIGMA_FLOOR, delta=True), ("bmu", "dist") + ref.ROW_KEYS + ("delta",), k)
    close_all(ens, mems)


# ---- 3. min_hits ----------------------------------------------------------------------------------------------------------
def test_min_hits_restricts_and_node_0_seeds():
    mems = []
    for k, (W, H, J, tr, rows) in enumerate(((10, 10, 9, po.STANDARD, 20), (5, 3, 13, po.MEDIAN, 70))):
        M, S, hits = unit_state(W, H, J, 400 + k)          # (node 0 has no hits)
        X = unit_rows(rows, J, 410 + k)
        valid = np.random.default_rng(420 + k).random((rows, J)) < 0.8
        near = [0, rows // 2, rows - 1]                    # rows that sit on node 0 in their valid columns
        X[near] = M[0]
        valid[near, 0] = True
        mems.append(Member(W, H, J, tr, poisoned(X, valid), M, S, hits, valid, min_hits=3))
        mems[-1].near = near
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got_b, got_s = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    check_against_twins(mems, got_b, got_s, capi.SIGMA_FLOOR, "min_hits = 3")
    check_against_cpu(mems, got_b, got_s, True, "min_hits = 3")
    free = ens.bmu_masked([m.valid for m in mems], 0)
    for k, m in enumerate(mems):
        b = got_b[k]["bmu"]
        assert m.hits[0] < 3 and (b[m.near] == 0).all() and (got_b[k]["dist"][m.near].view(np.uint32) == 0).all(), k
        assert ((b == 0) | (m.hits[b.astype(np.int64)] >= 3)).all(), k        # only node 0 may lack the hits
        assert (b != free[k]["bmu"]).any(), k                                 # the restriction restricts
    # per member: the same call with min_hits [0, 3] restricts member 1 alone
    mixed = ens.bmu_masked([m.valid for m in mems], [0, 3])
    assert beq(mixed[0]["bmu"], free[0]["bmu"]) and beq(mixed[1]["bmu"], got_b[1]["bmu"])
    close_all(ens, mems)


# ---- 4. engineered edge cases ---------------------------------------------------------------------------------------------
def test_engineered_edges():
    """duplicate model rows (the lowest index wins), a row without a valid column, a NaN in node 0's row at a valid column
    (node 0 is pinned, the distance is the quiet NaN) -- in a Standard member of 70 rows and a Median member with a
    column mask"""
    mems = []
    for k, (W, H, J, tr, rows, one) in enumerate(((7, 5, 13, po.STANDARD, 70, False), (5, 3, 9, po.MEDIAN, 20, True))):
        M, S, hits = unit_state(W, H, J, 500 + k)
        hits[:] = 5
        X = unit_rows(rows, J, 510 + k)
        rng = np.random.default_rng(520 + k)
        valid = rng.random(J if one else (rows, J)) < 0.75
        M[9] = M[4]                                         # duplicates: rows on node 4 / 9 report 4
        X[2] = X[rows - 1] = M[9]
        c = 1                                               # node 0 holds a NaN in column c
        M[0, c] = np.nan
        if one:
            valid[c] = True                                 # every row sees the NaN: node 0 everywhere
        else:
            valid[2, c] = valid[rows - 1, c] = False        # (these two do not see it)
            valid[5] = False                                # no valid column: every distance is +0, node 0 wins
            valid[65] = False
            valid[7, c] = True
        mems.append(Member(W, H, J, tr, poisoned(X, valid), M, S, hits, valid, min_hits=2))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for rule, floor in RULES:
        got_b, got_s = ensemble_calls(ens, mems, rule)
        check_against_twins(mems, got_b, got_s, rule, "edges")
        check_against_cpu(mems, got_b, got_s, floor, "edges")
    a, b = got_b
    sa = got_s[0]
    va = mems[0].valid
    assert a["bmu"][2] == 4 and a["bmu"][69] == 4 and a["dist"][2].view(np.uint32) == 0
    sees = va[:, 1]
    assert sees.any() and (~sees).any()
    assert (a["bmu"][sees] == 0).all() and (a["dist"][sees].view(np.uint32) == sr.QNAN).all()
    assert np.isfinite(a["dist"][~sees]).all()
    for r in (5, 65):
        assert a["bmu"][r] == 0 and a["dist"][r].view(np.uint32) == 0 and a["nvalid"][r] == 0
        assert beq(a["fill"][r], mems[0].M[0])
        assert sa["dmax"][r] == -np.inf and sa["dmax_col"][r] == sr.NONE and sa["first"][r].view(np.uint32) == sr.QNAN
        assert sa["amax"][r].view(np.uint32) == 0 and sa["amax_col"][r] == sr.NONE and sa["outside"][r] == 0
        assert (sa["delta"][r].view(np.uint32) == 0).all()
    assert (b["bmu"] == 0).all() and (b["dist"].view(np.uint32) == sr.QNAN).all()
    close_all(ens, mems)


# ---- 5. poison under invalid columns of map and sigmaMap ------------------------------------------------------------------
def test_poison_in_map_and_sigma_map():
    """columns that no row of the member has valid hold NaN, +-inf and 1e30 in every node's map and sigmaMap rows: every
    similarity output equals that of the clean state (no fill is asked for: fill copies the map by definition)"""
    mems, clean = [], []
    for k, (W, H, J, tr, rows, one) in enumerate(((10, 10, 9, po.STANDARD, 20, True), (7, 5, 37, po.MEDIAN, 70, False))):
        M, S, hits = unit_state(W, H, J, 600 + k)
        X = unit_rows(rows, J, 610 + k)
        rng = np.random.default_rng(620 + k)
        valid = rng.random(J if one else (rows, J)) < 0.7
        dead = [1, J - 1]
        valid[..., dead] = False
        Mp, Sp = M.copy(), S.copy()
        for i, c in enumerate(dead):
            Mp[:, c] = np.resize(np.roll(np.array(ref.POISON[:4], f32), i), M.shape[0])
            Sp[:, c] = np.resize(np.roll(np.array(ref.POISON[:4], f32), i + 1), M.shape[0])
        mems.append(Member(W, H, J, tr, poisoned(X, valid), Mp, Sp, hits, valid, min_hits=2))
        clean.append((M, S))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    args = ([m.valid for m in mems], 2, 3)
    for rule, floor in RULES:
        dirty = ens.similarity_masked(*args, rule, delta=True)
        for k, m in enumerate(mems):
            same(dirty[k], m.twin_similarity(rule), SIM_KEYS, ("poisoned state", k))
            same(dirty[k], m.cpu(floor)[1], SIM_KEYS, ("poisoned state, CPU", k))
            assert np.isfinite(dirty[k]["dist"]).all() and np.isfinite(dirty[k]["delta"]).all(), k
        for m, (M, S) in zip(mems, clean):
            m.m.set_state(map=M, sigma=S)
        for k, r in enumerate(ens.similarity_masked(*args, rule, delta=True)):
            same(dirty[k], r, SIM_KEYS, ("poisoned against clean", k))
        for m in mems:
            m.m.set_state(map=m.M, sigma=m.S)
    close_all(ens, mems)


# ---- 6. both sigma rules on the engineered sigmaMap -----------------------------------------------------------------------
def test_special_sigmas_both_rules():
    mems = []
    for k, (W, H, J, tr, rows) in enumerate(((5, 4, 16, po.STANDARD, 48), (5, 3, 13, po.MEDIAN, 70))):
        N = W * H
        M, _, hits = unit_state(W, H, J, 700 + k)
        S = np.stack([np.roll(np.resize(special_sigmas(), J), n) for n in range(N)]).astype(f32)
        X = unit_rows(rows, J, 710 + k)
        X[:N] = M                                           # rows that sit on a node: delta = 0 and 0-over-0 columns
        valid = np.random.default_rng(720 + k).random((rows, J)) < 0.8
        mems.append(Member(W, H, J, tr, X, M, S, hits, valid, min_hits=0, ns=2 + k))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    seen = []
    for rule, floor in RULES:
        got_b, got_s = ensemble_calls(ens, mems, rule)
        check_against_twins(mems, got_b, got_s, rule, "special sigmas")
        check_against_cpu(mems, got_b, got_s, floor, "special sigmas")
        seen.append(got_s)
    assert any(not beq(a["amax"], b["amax"]) for a, b in zip(*seen))       # the rule decides something
    close_all(ens, mems)


# ---- 7. read-only ---------------------------------------------------------------------------------------------------------
def test_both_calls_are_read_only():
    mems = build(0.3, 800)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    ens.bmu_batch()                                         # lastBMU and sqres hold the unmasked search's values

    def snapshot():
        return [(m.m.get_state(), m.m.get_last_bmu(), m.m.get_sqres()) for m in mems]

    before = snapshot()
    ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    ensemble_calls(ens, mems, capi.SIGMA_AS_WRITTEN, fill=False, delta=False)
    for k, ((s0, l0, q0), (s1, l1, q1)) in enumerate(zip(before, snapshot())):
        for key in STATE_KEYS:
            assert beq(s0[key], s1[key]), (k, key)
        assert beq(l0, l1) and beq(q0, q1), k
    # ... and the chunk: the unmasked search gives what it gave
    idx, dist = ens.bmu_batch()
    for k, (_, l0, q0) in enumerate(before):
        assert beq(idx[k], l0) and beq(dist[k], q0), k
    close_all(ens, mems)


# ---- 8. a sigmaMap written by a batch epoch -------------------------------------------------------------------------------
def test_similarity_reads_the_sigma_map_of_the_last_epoch():
    """A member cannot have a pending sigmaMap: vsom_ensemble_create materialises one and a member's epochs are eager from
    then on, so the issue's "pending sigmaMap" case has no pending record on the member's side.  What is held here is the
    other half: a batch epoch under VSOM_SIGMA_LAZY on every member and twin (a twin may leave its sigmaMap pending), then
    the ensemble's similarity gives what the twins give after sigma_flush, and no member reports a pending record."""
    mems = build(0.2, 900, poison=False)
    for m in mems:
        for ctx in (m.m, m.t):
            ctx.set_sigma_mode(capi.SIGMA_LAZY)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for m in mems:
        if m.rows:
            for ctx in (m.m, m.t):
                ctx.batch_epoch(1.5, True)
    got_b, got_s = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    for m in mems:
        m.t.sigma_flush()
        assert not m.m.sigma_stats()["pending"]
    check_against_twins(mems, got_b, got_s, capi.SIGMA_FLOOR, "after a batch epoch")
    for m in mems:
        assert beq(m.m.get_state()["sigma"], m.t.get_state()["sigma"])
    close_all(ens, mems)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member_and_change_nothing():
    mems = build(0.3, 1000, specs=SPECS[:5])
    n = len(mems)
    L = capi.lib()
    u8p = C.POINTER(C.c_uint8)
    valid = [np.ascontiguousarray(np.broadcast_to(m.valid, m.X.shape), dtype=np.uint8) for m in mems]

    def arrays(k_null=None):
        vp = (u8p * n)(*[u8p() if k == k_null else v.ctypes.data_as(u8p) for k, v in enumerate(valid)])
        return vp, (capi.MaskedOut * n)(), (capi.SimilarityMaskedOut * n)(), (C.c_int * n)(*[3] * n)

    def refused(rc, *patterns):
        assert rc == -1, rc                                 # VSOM_ERR_INVALID
        msg = L.vsom_last_error().decode()
        for p in patterns:
            assert p in msg, msg

    ens = vsom_amd.Ensemble([m.m for m in mems])
    vp, bo, so, ns = arrays()
    refused(L.vsom_ensemble_bmu_masked_batch(None, None, vp, None, bo), "null ensemble")
    refused(L.vsom_ensemble_similarity_masked_batch(None, None, ns, 1, vp, None, so), "null ensemble")
    refused(L.vsom_ensemble_bmu_masked_batch(ens._h, None, None, None, bo), "null valid_host")
    refused(L.vsom_ensemble_similarity_masked_batch(ens._h, None, ns, 1, None, None, so), "null valid_host")
    refused(L.vsom_ensemble_bmu_masked_batch(ens._h, None, vp, None, None), "null out")
    refused(L.vsom_ensemble_similarity_masked_batch(ens._h, None, ns, 1, vp, None, None), "null out")
    refused(L.vsom_ensemble_similarity_masked_batch(ens._h, None, None, 1, vp, None, so), "null num_sigmas")
    for rule in (2, -1):
        refused(L.vsom_ensemble_similarity_masked_batch(ens._h, None, ns, rule, vp, None, so), "unknown sigma_rule")
    assert L.vsom_ensemble_bmu_masked_batch(ens._h, None, vp, None, bo) == 0        # (all-null outputs are accepted)
    ens.close()

    # a member the masked calls do not take -- CLR, custom, without a chunk -- is refused when it has a validity, by name,
    # and skipped when it has none
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    clr.upload_chunk(unit_rows(8, 5, 1))
    d, r = hooks.shape("standard", 9)
    custom = capi.Context(5, 3, 9, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    custom.upload_chunk(unit_rows(8, 9, 2))
    fresh = vsom_amd.Context(5, 3, 9)
    for odd, rows, J, why in ((clr, 8, 5, "CLR contexts are not supported"), (custom, 8, 9, "custom contexts are not supported"),
                              (fresh, 1, 9, "no chunk loaded")):
        e2 = vsom_amd.Ensemble([mems[1].m, mems[2].m, odd])
        v = [mems[1].valid, mems[2].valid, np.ones((rows, J), bool)]
        keep = [np.ascontiguousarray(a, dtype=np.uint8) for a in v]
        vp3 = (u8p * 3)(*[a.ctypes.data_as(u8p) for a in keep])
        refused(L.vsom_ensemble_bmu_masked_batch(e2._h, None, vp3, None, (capi.MaskedOut * 3)()), "member 2", why)
        refused(L.vsom_ensemble_similarity_masked_batch(e2._h, None, (C.c_int * 3)(3, 3, 3), 1, vp3, None,
                                                        (capi.SimilarityMaskedOut * 3)()), "member 2", why)
        got = e2.bmu_masked([mems[1].valid, mems[2].valid, None], [mems[1].min_hits, mems[2].min_hits, 0], fill=True)
        assert got[2] is None
        same(got[0], mems[1].twin_bmu(), BMU_KEYS, ("beside", why))
        same(got[1], mems[2].twin_bmu(), BMU_KEYS, ("beside", why))
        e2.close()
    for ctx in (clr, custom, fresh):
        ctx.close()

    # nothing changed: a valid call on the first ensemble's members gives the right answer
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got_b, got_s = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    check_against_twins(mems, got_b, got_s, capi.SIGMA_FLOOR, "after the refusals")
    close_all(ens, mems)


def test_a_chunk_staged_ahead_is_refused():
    """a map whose batch epoch frees the staged rows early, so that a prefetch stages the next chunk over them (the shape of
    tests/test_gpu_tiny_masked.py's case): both queries refuse the member by name, as the single calls refuse its twin, the
    other member is untouched, and after the commit both answer what the twins answer"""
    W = H = 48
    J, rows = 196, 1100
    xs = [gen.mnist_like(rows, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * f32(100) + f32(100)).astype(f32)
    _, S, hits = unit_state(W, H, J, 4)
    big = Member(W, H, J, po.STANDARD, xs[0], init, S, hits, np.random.default_rng(5).random((rows, J)) < 0.7)
    small = build(0.3, 1200, specs=SPECS[1:2])[0]
    pin = capi.PinnedBuffer(xs[1].shape)
    pin.array[...] = xs[1]
    ens = vsom_amd.Ensemble([small.m, big.m])
    for ctx in (big.m, big.t):
        ctx.batch_epoch_async(10.0, True)
        ctx.prefetch_chunk(pin.array)                       # staged beside the chains of chunk 0
    before = (small.m.get_state(), small.m.get_last_bmu(), small.m.get_sqres())
    with pytest.raises(vsom_amd.VsomError, match="staged ahead"):
        big.twin_bmu()
    with pytest.raises(vsom_amd.VsomError, match="staged ahead"):
        big.twin_similarity(capi.SIGMA_FLOOR)
    valids = [small.valid, big.valid]
    with pytest.raises(vsom_amd.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.bmu_masked(valids, [small.min_hits, 0], fill=True)
    with pytest.raises(vsom_amd.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.similarity_masked(valids, [small.min_hits, 0], [small.ns, 3], delta=True)
    L = capi.lib()
    u8p = C.POINTER(C.c_uint8)
    keep = [np.ascontiguousarray(v, dtype=np.uint8) for v in valids]
    vp = (u8p * 2)(*[a.ctypes.data_as(u8p) for a in keep])
    assert L.vsom_ensemble_bmu_masked_batch(ens._h, None, vp, None, (capi.MaskedOut * 2)()) == -1      # VSOM_ERR_INVALID
    assert L.vsom_ensemble_similarity_masked_batch(ens._h, None, (C.c_int * 2)(3, 3), 1, vp, None,
                                                   (capi.SimilarityMaskedOut * 2)()) == -1
    after = (small.m.get_state(), small.m.get_last_bmu(), small.m.get_sqres())
    for key in STATE_KEYS:
        assert beq(before[0][key], after[0][key]), key
    assert beq(before[1], after[1]) and beq(before[2], after[2])
    for ctx in (big.m, big.t):
        ctx.commit_chunk()
    mems = [small, big]
    got_b, got_s = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    check_against_twins(mems, got_b, got_s, capi.SIGMA_FLOOR, "after the commit")
    ens.close()
    big.m.synchronize()
    for m in mems:
        m.close()
    pin.free()


# ---- 10. members on two streams -------------------------------------------------------------------------------------------
def test_members_on_two_streams():
    import torch
    mems = build(0.3, 1100)
    dev = torch.device("cuda", 0)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for k, m in enumerate(mems):
        m.m.set_stream(s0.cuda_stream)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    one = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    ens.close()
    for k, m in enumerate(mems):
        m.m.set_stream((s1 if k % 2 else s0).cuda_stream)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    two = ensemble_calls(ens, mems, capi.SIGMA_FLOOR)
    for keys, a, b in ((BMU_KEYS, one[0], two[0]), (SIM_KEYS, one[1], two[1])):
        for k, m in enumerate(mems):
            if m.valid is None:
                assert a[k] is None and b[k] is None
            else:
                same(a[k], b[k], keys, ("two streams", k))
    check_against_twins(mems, two[0], two[1], capi.SIGMA_FLOOR, "two streams")
    ens.close()
    for m in mems:
        m.m.synchronize()
        m.close()
