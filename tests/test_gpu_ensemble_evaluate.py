"""GPU: vsom_ensemble_evaluate_batch / vsom_ensemble_evaluate_masked_batch -- the validation loss (Som::evaluate) of every
member on its own chunk in one call, over all columns and over the valid columns only.  Every output
is held against two references: bit for bit (NaN equal to NaN, bsum and error included) against the single calls
(vsom_evaluate_batch, vsom_evaluate_masked_batch) on twin contexts that are no members, and against the CPU: bmu, dist,
nrepl and nvalid exact against the oracle's search and the restatements of tests/evaluate_ref.py / tests/masked_score_ref.py,
bsum within evaluate_ref.bound(C) of the float64 restatement -- the project's one tolerance for the device log; no other
is introduced here.
Shapes where this kernel can go wrong rather than at workload size: rows of 3 values (C < 4), 5 (4 <= C < 8), 9 (a scalar
tail of 1), 13 (the packet tail and a scalar tail), 37 (rest 5, two column walks); maps of 5 x 3, 7 x 5, the 10 x 10 x 9
fixture, CLR members (two-part model rows, the plain call only) and one 12 x 12 x 30 member whose N * J = 4320 > 4096 takes
the single call inside the ensemble call; chunks of 1, 9, 20 and 70 rows (two row tiles of 64, the second ragged, its last
eight partly dead; 9 rows leave the second scoring pass without rows); Standard, Median and CLR members in one ensemble
(three launches); a skipped member, a member with a column mask beside per-row masks, a member without rows."""
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
import evaluate_ref as er  # noqa: E402
import gen  # noqa: E402
import masked_score_ref as ref  # noqa: E402
from similarity_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
QNAN = 0x7FC00000
PLAIN_KEYS = ("bmu", "dist", "bsum", "nrepl")
MASKED_KEYS = PLAIN_KEYS + ("nvalid",)
STATE_KEYS = ("map", "S", "sigma", "weight", "hits")
# W, H, J, kind, rows, mask ("rows": rows x J bytes, "one": a column mask), min_hits, skipped, fast path (plain, masked)
SPECS = ((5, 3, 3, po.STANDARD, 1, "rows", 0, False, (1, 1)),
         (10, 10, 9, po.STANDARD, 20, "rows", 3, False, (1, 1)),
         (5, 3, 13, po.MEDIAN, 70, "rows", 0, False, (1, 1)),
         (5, 3, 5, po.STANDARD, 9, "rows", 2, False, (1, 1)),
         (7, 5, 37, po.STANDARD, 70, "rows", 3, False, (1, 1)),
         (10, 10, 9, po.MEDIAN, 20, "one", 2, False, (1, 1)),       # a column mask (the plain call takes it row by row)
         (12, 12, 30, po.STANDARD, 20, "rows", 2, False, (0, 0)),   # N * J = 4320: the single call, inside the ensemble call
         (10, 10, 9, po.STANDARD, 20, "rows", 0, True, (1, 1)),     # skipped
         (5, 3, 9, po.MEDIAN, 0, "rows", 0, False, (0, 0)))         # no rows
# the shapes of tests/test_gpu_ensemble_topk.py; the masked call takes no CLR member: there they are skipped
CLR_SPECS = ((7, 7, 6, po.CLR, 20, "rows", 0, False, (1, 0)), (4, 4, 5, po.CLR, 70, "rows", 0, False, (1, 0)))


def same(a, b, keys, what=None):
    for k in keys:
        assert beq(a[k], b[k]), (what, k)
    assert er.same_double(a["error"], b["error"]), (what, "error", a["error"], b["error"])


def unit_state(W, H, D, seed):
    """a map in (0, 1), mixed hit counts (0 .. 5, node 0 without hits)"""
    rng = np.random.default_rng(seed)
    N = W * H
    M = rng.uniform(0.02, 0.98, (N, D)).astype(f32)
    hits = rng.integers(0, 6, N).astype(np.uint64)
    hits[0] = 0
    return M, hits


def unit_rows(rows, J, seed):
    """rows in [0, 1] with some entries exactly 0 and some exactly 1"""
    rng = np.random.default_rng(seed)
    X = rng.random((rows, J)).astype(f32)
    X[rng.random((rows, J)) < 0.08] = f32(0)
    X[rng.random((rows, J)) < 0.08] = f32(1)
    return X


def column_factors(J, seed):
    """0 / 1 indicator columns as the reference's data sets have them (tests/test_gpu_evaluate.py), two binary ones at least
    where J allows"""
    rng = np.random.default_rng(seed)
    binary = (rng.random(J) < 0.5).astype(f32)
    binary[[0, J - 1]] = f32(1)
    continuous = (rng.random(J) < 0.85).astype(f32)
    continuous[[0, J - 1]] = f32(1)
    return binary, continuous


def poisoned(X, valid, start=0):
    """X with NaN, +-inf, 1e30 and values outside [0, 1] at its invalid positions"""
    Xp = X.copy()
    inv = ~np.broadcast_to(valid, X.shape)
    Xp[inv] = np.resize(np.roll(np.array(ref.POISON, f32), start), int(inv.sum()))
    return Xp


class Member:
    """a member and its twin (the same state and chunk; the twin is driven by the single calls) with the member's
    arguments: valid (rows x J bool, or J bool), min_hits, the column factors; skip: the ensemble calls leave it out"""

    def __init__(self, W, H, J, tr, X, M, hits, valid, min_hits, binary, continuous, skip=False, fast=(1, 1)):
        self.W, self.H, self.J, self.tr = W, H, J, tr
        self.X, self.M, self.hits = X, M, hits
        self.valid, self.min_hits, self.binary, self.continuous = valid, min_hits, binary, continuous
        self.skip, self.fast = skip, fast
        self.C = min(J, M.shape[1])
        self.m, self.t = self.context(), self.context()
        self._cpu = {}

    def context(self):
        ctx = vsom_amd.Context(self.W, self.H, self.J, self.tr)
        ctx.set_state(map=self.M, hits=self.hits)
        ctx.upload_chunk(self.X)
        return ctx

    @property
    def rows(self):
        return self.X.shape[0]

    @property
    def maskable(self):
        return self.tr != po.CLR

    @property
    def valid_rows(self):
        return np.ascontiguousarray(np.broadcast_to(self.valid, self.X.shape))

    def twin_plain(self, with_valid=True):
        return self.t.evaluate(self.binary, self.continuous, valid=self.valid_rows if with_valid else None)

    def twin_masked(self):
        return self.t.evaluate_masked(self.valid, self.binary, self.continuous, min_hits=self.min_hits)

    def search(self, masked):
        """the oracle's search, computed once: findBmu over all columns, or findRestrictedBmu over the valid ones"""
        if masked not in self._cpu:
            if self.tr == po.CLR:
                o = po.OracleSom(self.W, self.H, self.J, self.tr)
                o.set_state(map=self.M)
                with np.errstate(all="ignore"):
                    d = np.array([[o.dist(i, x) for i in range(self.W * self.H)] for x in self.X], f32)
                got = [ref.argmin_rule(row, self.hits, 0) for row in d]
                bmu, dist = np.array([g[0] for g in got], np.uint64), np.array([g[1] for g in got], f32)
                dist[np.isnan(dist)] = np.uint32(QNAN).view(f32)
            elif masked:
                bmu, dist = ref.checker(self.tr, self.X, self.M, self.valid, self.hits, self.min_hits)
            else:
                bmu, dist = ref.checker(self.tr, self.X, self.M, np.ones(self.J, bool), self.hits, 0)
            self._cpu[masked] = (bmu, dist)
        return self._cpu[masked]

    def check_cpu(self, got, masked, with_valid, what):
        """bmu, dist, nrepl, nvalid exact; bsum within bound(C) of the float64 restatement; error the running mean of the
        returned values on the bits"""
        bmu, dist = self.search(masked)
        assert (got["bmu"] == bmu).all() and beq(got["dist"], dist), what
        Mb = self.M[bmu.astype(np.int64)][:, :self.C]
        X, b, c = self.X[:, :self.C], self.binary[:self.C], self.continuous[:self.C]
        v = self.valid_rows[:, :self.C]
        if masked:
            b64, n64 = ref.evaluate64(X, Mb, b, c, v)
            assert (got["nvalid"] == self.valid_rows.sum(axis=1)).all(), what
        else:
            b64, n64 = er.restate64(X, Mb, b, c, v if with_valid else None)
        assert (got["nrepl"] == n64).all(), (what, got["nrepl"][:8], n64[:8])
        zero = b64 == 0
        assert (got["bsum"][zero].view(np.uint32) == 0).all(), what
        rel = np.abs(got["bsum"][~zero].astype(np.float64) - b64[~zero]) / b64[~zero]
        if rel.size:
            print(f"ensemble evaluate {what}: C = {self.C}, worst relative distance {rel.max() * 2 ** 24:.2f} x 2^-24, "
                  f"bound {er.bound(self.C) * 2 ** 24:.0f} x 2^-24")
            assert rel.max() <= er.bound(self.C), (what, float(rel.max()))
        assert er.same_double(got["error"], er.running_mean(got["dist"], got["bsum"])), what

    def close(self):
        self.m.close()
        self.t.close()


def build(frac, seed, poison=False, specs=SPECS):
    """the members of `specs` with random masks of about `frac` invalid entries; poison: NaN, inf, ... stored at the invalid
    positions of the rows (for the masked call: the plain call searches over every column)"""
    mems = []
    for i, (W, H, J, tr, rows, how, min_hits, skip, fast) in enumerate(specs):
        if tr == po.CLR:
            X = (np.abs(gen.blobs(rows, J, 4, seed + 10 * i, 2)) + 0.5).astype(f32)
            X = (X / X.max()).astype(f32)
            M, hits = unit_state(W, H, po.length(po.CLR, J), seed + 10 * i)
        else:
            M, hits = unit_state(W, H, J, seed + 10 * i)
            X = unit_rows(rows, J, seed + 10 * i + 1)
        rng = np.random.default_rng(seed + 10 * i + 2)
        valid = rng.random(J if how == "one" else (rows, J)) >= frac
        if how == "one":
            valid[J // 2] = True
        if poison:
            X = poisoned(X, valid, i)
        binary, continuous = column_factors(J, seed + 10 * i + 3)
        mems.append(Member(W, H, J, tr, X, M, hits, valid, min_hits, binary, continuous, skip, fast))
    return mems


def call_plain(ens, mems, with_valid=True):
    return ens.evaluate([m.binary for m in mems], [m.continuous for m in mems],
                        valid=[m.valid_rows for m in mems] if with_valid else None,
                        members=[k for k, m in enumerate(mems) if not m.skip])


def masked_valids(mems):
    return [None if m.skip or not m.maskable else m.valid for m in mems]


def call_masked(ens, mems):
    return ens.evaluate_masked(masked_valids(mems), [m.binary for m in mems], [m.continuous for m in mems],
                               min_hits=[m.min_hits for m in mems])


def check_against_twins(mems, got, masked, what, with_valid=True):
    for k, m in enumerate(mems):
        if m.skip or (masked and not m.maskable):
            assert got[k] is None, (what, k)
            continue
        assert got[k]["bmu"].shape == (m.rows,), (what, k)
        if m.rows == 0:                                  # (the single calls refuse a chunk without rows)
            assert got[k]["error"] == 0.0, (what, k)
            continue
        twin = m.twin_masked() if masked else m.twin_plain(with_valid)
        same(got[k], twin, MASKED_KEYS if masked else PLAIN_KEYS, (what, k))


def check_against_cpu(mems, got, masked, what, with_valid=True):
    for k, m in enumerate(mems):
        if got[k] is not None and m.rows:
            m.check_cpu(got[k], masked, with_valid, (what, k))


def close_all(ens, mems):
    ens.close()
    for m in mems:
        m.close()


# ---- 1, 2. random masks, every shape in one ensemble: the twins and the CPU ----------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("frac", [0.1, 0.6])
def test_random_masks(frac, masked):
    mems = build(frac, 100 + int(frac * 10), poison=masked, specs=SPECS + CLR_SPECS)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for k, m in enumerate(mems):
        assert ens.evaluate_applies(k, masked) == bool(m.fast[masked]), k
    got = call_masked(ens, mems) if masked else call_plain(ens, mems)
    what = ("random", frac, "masked" if masked else "plain")
    check_against_twins(mems, got, masked, what)
    check_against_cpu(mems, got, masked, what)
    scored = [r for r, m in zip(got, mems) if r is not None and m.rows]
    assert all((r["bsum"] > 0).any() and np.isfinite(r["bsum"]).all() and np.isfinite(r["dist"]).all() for r in scored)
    # what a sweep sorts by
    cols = ([m.binary for m in mems], [m.continuous for m in mems])
    if masked:
        ve = ens.validation_errors(*cols, valid=masked_valids(mems), masked=True, min_hits=[m.min_hits for m in mems])
    else:
        ve = ens.validation_errors(*cols, valid=[m.valid_rows for m in mems],
                                   members=[k for k, m in enumerate(mems) if not m.skip])
    for k, r in enumerate(got):
        assert np.isnan(ve[k]) if r is None else er.same_double(ve[k], r["error"]), k
    close_all(ens, mems)


# ---- 3. exact cases --------------------------------------------------------------------------------------------------------
def test_no_binary_column_gives_the_search_alone():
    mems = build(0.3, 300, specs=SPECS + CLR_SPECS)
    for m in mems:
        m.binary = np.zeros(m.J, f32)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got = call_plain(ens, mems)
    idx, dist = ens.bmu_batch()
    for k, m in enumerate(mems):
        if m.skip:
            continue
        assert (got[k]["bmu"] == idx[k]).all() and beq(got[k]["dist"], dist[k]), k
        assert (got[k]["bsum"].view(np.uint32) == 0).all() and (got[k]["nrepl"] == 0).all(), k
        assert er.same_double(got[k]["error"], er.running_mean(dist[k], np.zeros(m.rows, f32))), k
    gm = call_masked(ens, mems)
    for k, m in enumerate(mems):
        if gm[k] is not None:
            assert (gm[k]["bsum"].view(np.uint32) == 0).all() and (gm[k]["nrepl"] == 0).all(), k
            assert er.same_double(gm[k]["error"], er.running_mean(gm[k]["dist"], np.zeros(m.rows, f32))), k
    close_all(ens, mems)


def test_every_counting_term_replaced_is_exact():
    """model values 0 and 1 in the binary columns: log gives -inf or 0 there, every counting term is NaN or -inf and is
    replaced by -99999, so no last bit of a log reaches bsum -- it equals the fp32 restatement in Eigen's packet order"""
    mems = build(0.3, 400, specs=SPECS[:7])
    for i, m in enumerate(mems):
        rng = np.random.default_rng(410 + i)
        cols = np.flatnonzero(m.binary)
        m.binary[cols] = rng.choice(np.array([1.0, 0.5, 2.0, 3.0], f32), cols.size)
        m.continuous[:] = f32(1)
        for n in range(m.M.shape[0]):
            m.M[n, cols] = np.roll(np.resize(np.array([0.0, 1.0, 1.0, 0.0, 0.0], f32), cols.size), n)
        for ctx in (m.m, m.t):
            ctx.set_state(map=m.M)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    for masked in (False, True):
        got = call_masked(ens, mems) if masked else call_plain(ens, mems)
        check_against_twins(mems, got, masked, ("replaced", masked))
        for k, m in enumerate(mems):
            b = got[k]["bmu"].astype(np.int64)
            if masked:
                b32, n32, exact, _ = ref.evaluate32(m.X, m.M[b], m.binary, m.continuous, m.valid_rows)
            else:
                b32, n32, exact, _ = er.restate32(m.X, m.M[b], m.binary, m.continuous, m.valid_rows)
            assert exact.all(), k
            assert beq(got[k]["bsum"], b32) and (got[k]["nrepl"] == n32).all(), (k, masked)
        assert sum(int(r["nrepl"].sum()) for r in got) > 0 and any((r["bsum"] > 0).any() for r in got)
    close_all(ens, mems)


# ---- 4. the all-valid mask is the plain call -------------------------------------------------------------------------------
def test_all_valid_masked_equals_plain():
    mems = build(0.0, 500, specs=SPECS)
    for m in mems:
        m.min_hits = 0
        m.skip = False
        m.valid = np.ones(m.J, bool) if m.valid.ndim == 1 else np.ones(m.X.shape, bool)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    plain = call_plain(ens, mems, with_valid=False)
    per_member_null = ens.evaluate([m.binary for m in mems], [m.continuous for m in mems], valid=[None] * len(mems))
    with_bytes = call_plain(ens, mems)
    masked = call_masked(ens, mems)
    for k, m in enumerate(mems):
        same(plain[k], per_member_null[k], PLAIN_KEYS, ("NULL array against NULL entries", k))
        same(plain[k], with_bytes[k], PLAIN_KEYS, ("NULL against all-valid bytes", k))
        same(plain[k], masked[k], PLAIN_KEYS, ("masked against plain", k))
        assert (masked[k]["nvalid"] == m.J).all(), k
    check_against_twins(mems, plain, False, "valid = NULL", with_valid=False)
    check_against_cpu(mems, plain, False, "valid = NULL", with_valid=False)
    close_all(ens, mems)


# ---- 5. edges --------------------------------------------------------------------------------------------------------------
def test_min_hits_restricts_and_node_0_seeds():
    mems = []
    for k, (W, H, J, tr, rows) in enumerate(((10, 10, 9, po.STANDARD, 20), (5, 3, 13, po.MEDIAN, 70))):
        M, hits = unit_state(W, H, J, 600 + k)             # (node 0 has no hits)
        X = unit_rows(rows, J, 610 + k)
        valid = np.random.default_rng(620 + k).random((rows, J)) < 0.8
        near = [0, rows // 2, rows - 1]                    # rows that sit on node 0 in their valid columns
        X[near] = M[0]
        valid[near, 0] = True
        binary, continuous = column_factors(J, 630 + k)
        mems.append(Member(W, H, J, tr, poisoned(X, valid), M, hits, valid, 3, binary, continuous))
        mems[-1].near = near
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got = call_masked(ens, mems)
    check_against_twins(mems, got, True, "min_hits = 3")
    check_against_cpu(mems, got, True, "min_hits = 3")
    for m in mems:
        m.min_hits = 0
    free = call_masked(ens, mems)
    for k, m in enumerate(mems):
        b = got[k]["bmu"]
        assert m.hits[0] < 3 and (b[m.near] == 0).all() and (got[k]["dist"][m.near].view(np.uint32) == 0).all(), k
        assert ((b == 0) | (m.hits[b.astype(np.int64)] >= 3)).all(), k        # only node 0 may lack the hits
        assert (b != free[k]["bmu"]).any(), k                                 # the restriction restricts
    # min_hits NULL in the C call is all 0
    n = len(mems)
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    keep = [np.ascontiguousarray(m.valid, dtype=np.uint8) for m in mems]
    outs = (capi.EvaluateMaskedOut * n)()
    bmu = [np.empty(m.rows, np.uint64) for m in mems]
    for k in range(n):
        outs[k].bmu = bmu[k].ctypes.data_as(C.POINTER(C.c_uint64))
    assert capi.lib().vsom_ensemble_evaluate_masked_batch(
        ens._h, None, (fp * n)(*[m.binary.ctypes.data_as(fp) for m in mems]),
        (fp * n)(*[m.continuous.ctypes.data_as(fp) for m in mems]), (u8p * n)(*[a.ctypes.data_as(u8p) for a in keep]),
        None, outs) == 0
    for k in range(n):
        assert (bmu[k] == free[k]["bmu"]).all(), k
    close_all(ens, mems)


def test_engineered_edges():
    """a row without a valid column (node 0, distance +0, nvalid 0, bsum +0), a NaN in node 0's row at a column that some
    rows have valid (node 0 is pinned, the distance is the quiet NaN, and the scoring reads node 0's row), duplicate model
    rows (the lowest index wins) -- in a Standard member of 70 rows and a Median member with a column mask; then the plain
    call on the same state: every row sees the NaN"""
    mems = []
    for k, (W, H, J, tr, rows, one) in enumerate(((7, 5, 13, po.STANDARD, 70, False), (5, 3, 9, po.MEDIAN, 20, True))):
        M, hits = unit_state(W, H, J, 700 + k)
        hits[:] = 5
        X = unit_rows(rows, J, 710 + k)
        rng = np.random.default_rng(720 + k)
        valid = rng.random(J if one else (rows, J)) < 0.75
        M[9] = M[4]
        X[2] = X[rows - 1] = M[9]
        c = 1                                               # node 0 holds a NaN in column c
        M[0, c] = np.nan
        if one:
            valid[c] = True                                 # every row sees the NaN: node 0 everywhere
        else:
            valid[2, c] = valid[rows - 1, c] = False        # (these two do not see it)
            valid[5] = False                                # no valid column
            valid[65] = False
            valid[7, c] = True
        binary, continuous = column_factors(J, 730 + k)
        binary[c] = f32(1)                                  # the NaN model value is scored: a replaced term
        continuous[c] = f32(1)
        mems.append(Member(W, H, J, tr, poisoned(X, valid), M, hits, valid, 2, binary, continuous))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    got = call_masked(ens, mems)
    check_against_twins(mems, got, True, "edges")
    check_against_cpu(mems, got, True, "edges")
    a, b = got
    assert a["bmu"][2] == 4 and a["bmu"][69] == 4 and a["dist"][2].view(np.uint32) == 0
    sees = mems[0].valid[:, 1]
    assert sees.any() and (~sees).any()
    assert (a["bmu"][sees] == 0).all() and (a["dist"][sees].view(np.uint32) == QNAN).all() and (a["nrepl"][sees] >= 1).all()
    assert np.isfinite(a["dist"][~sees]).all() and np.isfinite(a["bsum"]).all()
    for r in (5, 65):
        assert a["bmu"][r] == 0 and a["dist"][r].view(np.uint32) == 0 and a["nvalid"][r] == 0
        assert a["bsum"][r].view(np.uint32) == 0 and a["nrepl"][r] == 0
    assert (b["bmu"] == 0).all() and (b["dist"].view(np.uint32) == QNAN).all() and np.isnan(b["error"])
    close_all(ens, mems)
    # the plain call: clean rows, the same maps
    plain = [Member(m.W, m.H, m.J, m.tr, unit_rows(m.rows, m.J, 740 + k), m.M, m.hits, m.valid, 0, m.binary, m.continuous)
             for k, m in enumerate(mems)]
    ens = vsom_amd.Ensemble([m.m for m in plain])
    got = call_plain(ens, plain)
    check_against_twins(plain, got, False, "edges, plain")
    check_against_cpu(plain, got, False, "edges, plain")
    for r in got:
        assert (r["bmu"] == 0).all() and (r["dist"].view(np.uint32) == QNAN).all() and np.isnan(r["error"])
    close_all(ens, plain)


def test_poison_in_rows_and_map_reaches_no_output():
    """columns that no row of the member has valid hold NaN, +-inf and 1e30 in every node's map row, and the rows hold
    poison at every invalid position: every output of the masked call equals that of the clean map and clean rows"""
    mems, clean = [], []
    for k, (W, H, J, tr, rows, one) in enumerate(((10, 10, 9, po.STANDARD, 20, True), (7, 5, 37, po.MEDIAN, 70, False))):
        M, hits = unit_state(W, H, J, 800 + k)
        X = unit_rows(rows, J, 810 + k)
        rng = np.random.default_rng(820 + k)
        valid = rng.random(J if one else (rows, J)) < 0.7
        dead = [1, J - 1]
        valid[..., dead] = False
        Mp = M.copy()
        for i, c in enumerate(dead):
            Mp[:, c] = np.resize(np.roll(np.array(ref.POISON[:4], f32), i), M.shape[0])
        binary, continuous = column_factors(J, 830 + k)     # (columns 0 and J - 1 are binary: a dead one among them)
        mems.append(Member(W, H, J, tr, poisoned(X, valid), Mp, hits, valid, 2, binary, continuous))
        clean.append((M, np.where(np.broadcast_to(valid, X.shape), X, f32(0.5)).astype(f32)))
    ens = vsom_amd.Ensemble([m.m for m in mems])
    dirty = call_masked(ens, mems)
    check_against_twins(mems, dirty, True, "poisoned state")
    for k, m in enumerate(mems):
        assert np.isfinite(dirty[k]["dist"]).all() and np.isfinite(dirty[k]["bsum"]).all() and np.isfinite(dirty[k]["error"]), k
    for m, (M, X) in zip(mems, clean):
        m.m.set_state(map=M)
        m.m.upload_chunk(X)
    for k, r in enumerate(call_masked(ens, mems)):
        same(dirty[k], r, MASKED_KEYS, ("poisoned against clean", k))
    close_all(ens, mems)


# ---- 6. side effects -------------------------------------------------------------------------------------------------------
def test_plain_call_leaves_the_search_results_and_masked_call_nothing():
    mems = build(0.3, 900, specs=SPECS + CLR_SPECS)
    ens = vsom_amd.Ensemble([m.m for m in mems])

    def snapshot():
        return [(m.m.get_state(), m.m.get_last_bmu(), m.m.get_sqres()) for m in mems]

    fresh = snapshot()
    got = call_plain(ens, mems)
    after_eval = snapshot()
    for k, m in enumerate(mems):
        if m.skip:                                         # not touched: lastBMU as the upload left it
            assert beq(fresh[k][1], after_eval[k][1]) and beq(fresh[k][2], after_eval[k][2]), k
            continue
        assert (after_eval[k][1] == got[k]["bmu"]).all() and beq(after_eval[k][2], got[k]["dist"]), k
        for key in STATE_KEYS:
            assert beq(fresh[k][0][key], after_eval[k][0][key]), (k, key)
    assert any((s[1] != 0).any() for s in after_eval)
    ens.bmu_batch()
    after_bmu = snapshot()
    for k, m in enumerate(mems):
        if not m.skip:
            assert beq(after_eval[k][1], after_bmu[k][1]) and beq(after_eval[k][2], after_bmu[k][2]), k
    # the masked call: lastBMU, sqres and the whole state stay
    call_masked(ens, mems)
    for k, (a, b) in enumerate(zip(after_bmu, snapshot())):
        for key in STATE_KEYS:
            assert beq(a[0][key], b[0][key]), (k, key)
        assert beq(a[1], b[1]) and beq(a[2], b[2]), k
    close_all(ens, mems)


def test_a_following_epoch_starts_from_the_call_s_last_bmu():
    mems = build(0.3, 1000, specs=SPECS[:7] + CLR_SPECS)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    call_plain(ens, mems)
    call_masked(ens, mems)                                  # (read-only: changes nothing for the epoch)
    mse = ens.batch_epoch(1.5, False)
    for k, m in enumerate(mems):
        m.twin_plain()
        tm = m.t.batch_epoch(1.5, False)
        a, b = m.m.get_state(), m.t.get_state()
        for key in STATE_KEYS:
            assert beq(a[key], b[key]), (k, key)
        assert beq(m.m.get_last_bmu(), m.t.get_last_bmu()) and beq(np.array([mse[k]], f32), np.array([tm], f32)), k
    close_all(ens, mems)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_member_and_change_nothing():
    mems = build(0.3, 1100, specs=SPECS[:5])
    n = len(mems)
    L = capi.lib()
    fp, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    valid = [m.valid_rows.astype(np.uint8) for m in mems]

    def arrays(b_null=None, c_null=None):
        return ((fp * n)(*[fp() if k == b_null else m.binary.ctypes.data_as(fp) for k, m in enumerate(mems)]),
                (fp * n)(*[fp() if k == c_null else m.continuous.ctypes.data_as(fp) for k, m in enumerate(mems)]),
                (u8p * n)(*[v.ctypes.data_as(u8p) for v in valid]), (capi.EvaluateOut * n)(), (capi.EvaluateMaskedOut * n)())

    def refused(rc, *patterns):
        assert rc == -1, rc                                 # VSOM_ERR_INVALID
        msg = L.vsom_last_error().decode()
        for p in patterns:
            assert p in msg, msg

    ens = vsom_amd.Ensemble([m.m for m in mems])
    ens.bmu_batch()
    before = [(m.m.get_state(), m.m.get_last_bmu(), m.m.get_sqres()) for m in mems]
    bp, cp, vp, po_, mo = arrays()
    refused(L.vsom_ensemble_evaluate_batch(None, bp, cp, vp, po_), "null ensemble")
    refused(L.vsom_ensemble_evaluate_masked_batch(None, None, bp, cp, vp, None, mo), "null ensemble")
    refused(L.vsom_ensemble_evaluate_batch(ens._h, None, cp, vp, po_), "null binary_host or continuous_host")
    refused(L.vsom_ensemble_evaluate_batch(ens._h, bp, None, vp, po_), "null binary_host or continuous_host")
    refused(L.vsom_ensemble_evaluate_batch(ens._h, bp, cp, vp, None), "null out")
    refused(L.vsom_ensemble_evaluate_masked_batch(ens._h, None, None, cp, vp, None, mo), "null binary_host or continuous_host")
    refused(L.vsom_ensemble_evaluate_masked_batch(ens._h, None, bp, None, vp, None, mo), "null binary_host or continuous_host")
    refused(L.vsom_ensemble_evaluate_masked_batch(ens._h, None, bp, cp, None, None, mo), "null valid_host")
    refused(L.vsom_ensemble_evaluate_masked_batch(ens._h, None, bp, cp, vp, None, None), "null out")
    # a covered member without a column array
    bp3, cp3, _, _, _ = arrays(b_null=3, c_null=2)
    refused(L.vsom_ensemble_evaluate_batch(ens._h, bp, cp3, vp, po_), "member 2", "binary_host or continuous_host is null")
    refused(L.vsom_ensemble_evaluate_masked_batch(ens._h, None, bp3, cp, vp, None, mo), "member 3",
            "binary_host or continuous_host is null")
    refused(L.vsom_ensemble_evaluate_masked_batch(ens._h, None, bp, cp3, vp, None, mo), "member 2",
            "binary_host or continuous_host is null")
    assert L.vsom_ensemble_evaluate_batch(ens._h, bp3, cp, vp, po_) == 0     # (plain: a null binary_host[k] skips member 3;
    assert L.vsom_ensemble_evaluate_masked_batch(ens._h, None, bp, cp, vp, None, mo) == 0   # all-null outputs are accepted)
    ens.bmu_batch()
    for k, (m, (s0, l0, q0)) in enumerate(zip(mems, before)):
        s1 = m.m.get_state()
        for key in STATE_KEYS:
            assert beq(s0[key], s1[key]), (k, key)
        assert beq(l0, m.m.get_last_bmu()) and beq(q0, m.m.get_sqres()), k
    ens.close()

    # a member the calls do not take -- CLR in the masked call, custom, without a chunk -- is refused when covered, by name,
    # and skipped when not
    clr = build(0.3, 1150, specs=CLR_SPECS[:1])[0]
    d, r = hooks.shape("standard", 9)
    custom = capi.Context(5, 3, 9, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    custom.upload_chunk(unit_rows(8, 9, 2))
    fresh = vsom_amd.Context(5, 3, 9)
    for odd, rows, J, why, plain_too in ((clr.m, clr.rows, clr.J, "CLR contexts are not supported", False),
                                          (custom, 8, 9, "custom contexts are not supported", True),
                                          (fresh, 1, 9, "no chunk loaded", True)):
        e2 = vsom_amd.Ensemble([mems[1].m, mems[2].m, odd])
        ones = np.ones(J, f32)
        keep = [valid[1], valid[2], np.ones((rows, J), np.uint8)]
        b3 = (fp * 3)(mems[1].binary.ctypes.data_as(fp), mems[2].binary.ctypes.data_as(fp), ones.ctypes.data_as(fp))
        c3 = (fp * 3)(mems[1].continuous.ctypes.data_as(fp), mems[2].continuous.ctypes.data_as(fp), ones.ctypes.data_as(fp))
        v3 = (u8p * 3)(*[a.ctypes.data_as(u8p) for a in keep])
        refused(L.vsom_ensemble_evaluate_masked_batch(e2._h, None, b3, c3, v3, None, (capi.EvaluateMaskedOut * 3)()),
                "member 2", why)
        if plain_too:
            refused(L.vsom_ensemble_evaluate_batch(e2._h, b3, c3, v3, (capi.EvaluateOut * 3)()), "member 2", why)
        pair = [mems[1], mems[2]]
        gm = e2.evaluate_masked([mems[1].valid, mems[2].valid, None], [mems[1].binary, mems[2].binary, None],
                                [mems[1].continuous, mems[2].continuous, None], min_hits=[mems[1].min_hits, mems[2].min_hits, 0])
        gp = e2.evaluate([mems[1].binary, mems[2].binary, None], [mems[1].continuous, mems[2].continuous, None],
                         valid=[mems[1].valid_rows, mems[2].valid_rows, None], members=[0, 1])
        assert gm[2] is None and gp[2] is None
        check_against_twins(pair, gm[:2], True, ("beside", why))
        check_against_twins(pair, gp[:2], False, ("beside", why))
        e2.close()
    clr.close()
    for ctx in (custom, fresh):
        ctx.close()
    for m in mems:
        m.close()


def test_a_chunk_staged_ahead_is_refused():
    """a map whose batch epoch frees the staged rows early, so that a prefetch stages the next chunk over them (the shape of
    tests/test_gpu_ensemble_masked_query.py's case): both calls refuse the member by name, as the single calls refuse its
    twin, the other member is untouched, and after the commit both answer what the twins answer"""
    W = H = 48
    J, rows = 196, 1100
    xs = [gen.mnist_like(rows, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * f32(100) + f32(100)).astype(f32)
    _, hits = unit_state(W, H, J, 4)
    binary, continuous = column_factors(J, 6)
    big = Member(W, H, J, po.STANDARD, xs[0], init, hits, np.random.default_rng(5).random((rows, J)) < 0.7, 0, binary,
                 continuous, fast=(0, 0))
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
        call_plain(ens, mems)
    with pytest.raises(vsom_amd.VsomError, match="member 1: the next chunk is staged ahead"):
        call_masked(ens, mems)
    after = (small.m.get_state(), small.m.get_last_bmu(), small.m.get_sqres())
    for key in STATE_KEYS:
        assert beq(before[0][key], after[0][key]), key
    assert beq(before[1], after[1]) and beq(before[2], after[2])
    for ctx in (big.m, big.t):
        ctx.commit_chunk()
    big.X = xs[1]                                           # (the committed chunk; the twins hold it too)
    check_against_twins(mems, call_plain(ens, mems), False, "after the commit")
    check_against_twins(mems, call_masked(ens, mems), True, "after the commit")
    ens.close()
    big.m.synchronize()
    for m in mems:
        m.close()
    pin.free()


# ---- 8. members on two streams ---------------------------------------------------------------------------------------------
def test_members_on_two_streams():
    import torch
    mems = build(0.3, 1300, specs=SPECS + CLR_SPECS)
    dev = torch.device("cuda", 0)
    s0, s1 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    for m in mems:
        m.m.set_stream(s0.cuda_stream)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    one = (call_plain(ens, mems), call_masked(ens, mems))
    ens.close()
    for k, m in enumerate(mems):
        m.m.set_stream((s1 if k % 2 else s0).cuda_stream)
    ens = vsom_amd.Ensemble([m.m for m in mems])
    two = (call_plain(ens, mems), call_masked(ens, mems))
    for masked, keys in ((False, PLAIN_KEYS), (True, MASKED_KEYS)):
        for k, (a, b) in enumerate(zip(one[masked], two[masked])):
            if a is None:
                assert b is None, k
            else:
                same(a, b, keys, ("two streams", masked, k))
        check_against_twins(mems, two[masked], masked, ("two streams", masked))
    ens.close()
    for m in mems:
        m.m.synchronize()
        m.close()
