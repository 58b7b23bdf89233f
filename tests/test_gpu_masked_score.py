"""GPU: vsom_similarity_masked_batch / vsom_evaluate_masked_batch -- chunk rows searched over their valid columns only and
scored against that unit in those columns, in one call.  Expected values come from tests/masked_score_ref.py: the masked
search as tests/test_gpu_masked.py restates it, similarity_ref with delta set to NaN at invalid columns, evaluate_ref with
the select at invalid columns.  Everything is held bit for bit (NaN equal to NaN) except bsum where the device's log
decides a last bit: there evaluate_ref.bound(C) against the float64 restatement, the project's derived bound.
Shapes as tests/test_gpu_masked.py: maps of 35 nodes (less than one node tile) and 135 (two tiles and a ragged one), J of
3 / 9 / 37 / 70 (no whole quad, C < 64, tails that are no multiple of 4, more than one lane step of the scorer), 70 rows
(one row tile and 6 rows; no multiple of the 4 rows of a scoring workgroup)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402
import masked_score_ref as ref  # noqa: E402
import similarity_ref as sr  # noqa: E402
from similarity_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
f32 = np.float32
B = 70
MAPS = ((7, 5), (9, 15))
DEPTHS = (3, 9, 37, 70)
KINDS = (po.STANDARD, po.MEDIAN)
SHAPES = [(tr, W, H, J) for tr in KINDS for (W, H) in MAPS for J in DEPTHS]
SIM_KEYS = ("bmu", "dist", "nvalid") + ref.ROW_KEYS + ("delta",)
EV_KEYS = ("bmu", "dist", "nvalid", "bsum", "nrepl")
RULES = ((capi.SIGMA_AS_WRITTEN, False), (capi.SIGMA_FLOOR, True))
MODES = (capi.BMU_AUTO, capi.BMU_EXACT, capi.BMU_SHORTLIST)


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


def column_factors(J, seed):
    rng = np.random.default_rng(seed)
    binary = rng.choice(np.array([0.0, 1.0, 0.5, 2.0], f32), J).astype(f32)
    binary[rng.integers(0, J)] = f32(1)                 # at least one binary column
    continuous = (rng.random(J) < 0.85).astype(f32)
    continuous[np.flatnonzero(binary)[0]] = f32(1)
    return binary, continuous


def make(tr, W, H, J, seed=3, rows=B):
    M, S, hits = unit_state(W, H, J, seed + 10)
    X = unit_rows(rows, J, seed)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M, sigma=S, hits=hits)
    ctx.upload_chunk(X)
    return ctx, X, M, S, hits


def expect_similarity(tr, X, M, S, valid, hits, min_hits, ns, floor, rows=None):
    """(bmu, dist, report) of the reference for the rows (all when None)"""
    idx = np.arange(X.shape[0]) if rows is None else np.asarray(rows)
    bmu, dist = ref.checker(tr, X, M, valid, hits, min_hits, idx)
    b = bmu.astype(np.int64)
    v = valid if valid.ndim == 1 else valid[idx]
    rep = ref.similarity(X[idx], M[b], S[b], ns, floor, v)
    rep.update(bmu=bmu, dist=dist, nvalid=np.broadcast_to(v, X[idx].shape).sum(axis=1).astype(np.uint32))
    return rep


def check_evaluate(got, X, Mb, binary, continuous, valid, what):
    """bsum within the derived bound of the float64 restatement; nrepl, zero sums, rows whose every counting term is
    replaced or has a zero factor, and the running mean exact"""
    C = X.shape[1]
    b64, n64 = ref.evaluate64(X, Mb, binary, continuous, valid)
    b32, n32, exact, _ = ref.evaluate32(X, Mb, binary, continuous, valid)
    assert (got["nrepl"] == n64).all() and (n32 == n64).all(), (what, got["nrepl"][:8], n64[:8])
    zero = b64 == 0
    assert (got["bsum"][zero].view(np.uint32) == 0).all(), what
    assert beq(got["bsum"][exact], b32[exact]), (what, "exact rows")
    rel = np.abs(got["bsum"][~zero].astype(np.float64) - b64[~zero]) / b64[~zero]
    if rel.size:
        print(f"evaluate_masked {what}: C = {C}, worst relative distance {rel.max() * 2 ** 24:.2f} x 2^-24, "
              f"bound {ref.bound(C) * 2 ** 24:.0f} x 2^-24, {int(exact.sum())} exact rows")
        assert rel.max() <= ref.bound(C), (what, int(np.flatnonzero(~zero)[int(np.argmax(rel))]))
    assert ref.same_double(got["error"], ref.running_mean(got["dist"], got["bsum"])), what
    return exact


# ---- 1. the all-valid mask is the unmasked call ---------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", SHAPES)
def test_all_valid_equals_the_unmasked_calls(tr, W, H, J):
    ctx, X, M, S, hits = make(tr, W, H, J)
    ones = np.ones((B, J), np.uint8)
    keys = ("bmu", "dist") + ref.ROW_KEYS + ("delta",)
    for min_hits in (0, 3):
        for rule, _ in RULES:
            for delta in (True, False):
                a = ctx.similarity_masked(ones, min_hits, 3, rule, delta=delta)
                b = ctx.similarity(min_hits, 3, rule, delta=delta)
                same(a, b, keys, (min_hits, rule, delta))
                assert (a["nvalid"] == J).all()
            same(ctx.similarity_masked(np.ones(J, np.uint8), min_hits, 3, rule, delta=True),
                 ctx.similarity_masked(ones, min_hits, 3, rule, delta=True), SIM_KEYS, "column mask of ones")
    assert (ctx.similarity_masked(ones, 3, 3)["bmu"] != ctx.similarity_masked(ones, 0, 3)["bmu"]).any()   # the restriction restricts
    binary, continuous = column_factors(J, J + 3)
    for mode in MODES:
        ctx.set_bmu_mode(mode)
        e = ctx.evaluate(binary, continuous)
        m = ctx.evaluate_masked(ones, binary, continuous)
        same(m, e, ("bmu", "dist", "bsum", "nrepl"), mode)
        assert ref.same_double(m["error"], e["error"]), mode
        assert (m["nvalid"] == J).all() and (m["bsum"] > 0).any()
    ctx.close()


# ---- 2. random masks against the reference --------------------------------------------------------------------------------
def random_case(tr, W, H, J):
    """70 %-valid masks with a row without a valid column, a row with exactly one and a column no row has valid; poison at
    invalid positions of x (Xp; X holds the rows without it); model columns R that are 0 in every node (their binary
    terms are replaced by -99999 whatever x holds)"""
    M, S, hits = unit_state(W, H, J, 15)
    X = unit_rows(B, J, 5)
    R = [1] if J < 9 else [1, J - 2]
    M[:, R] = f32(0)
    rng = np.random.default_rng(100 + J)
    valid = rng.random((B, J)) < 0.7
    valid[:, J - 1] = False
    valid[11] = False
    valid[12] = False
    valid[12, J // 2] = True
    Xp = X.copy()
    for i, r in enumerate((3, 11, 20, 37, 64, 66, 69)):   # poison stored at invalid positions (rows of the ragged row tile,
        valid[r, r % J] = False                           # the row without a valid column among them)
        cols = np.flatnonzero(~valid[r])
        Xp[r, cols] = ref.POISON[i % len(ref.POISON)]
        if cols.size > 1:
            Xp[r, cols[-1]] = ref.POISON[(i + 1) % len(ref.POISON)]
    return X, Xp, M, S, hits, valid, R


def moved_by_the_mask(tr, X, M, valid, hits, min_hits):
    """(units of the unmasked search on the zero-filled rows, units of the masked search): the CPU checker alone"""
    X0 = np.where(valid, X, f32(0)).astype(f32)
    return (ref.checker(tr, X0, M, np.ones(X.shape[1], bool), hits, min_hits)[0],
            ref.checker(tr, X0, M, valid, hits, min_hits)[0])


@pytest.mark.parametrize("tr, W, H, J", SHAPES)
def test_random_masks(tr, W, H, J):
    X, Xp, M, S, hits, valid, R = random_case(tr, W, H, J)
    ctx = vsom_amd.Context(W, H, J, tr)
    binary, continuous = column_factors(J, J + 3)
    only_r = np.zeros(J, f32)
    only_r[R] = f32(2)                                 # binary columns whose every term is replaced: bsum is exact
    # the mask matters: on the zero-filled rows the unmasked search finds other units (the CPU checker alone shows it)
    X0 = np.where(valid, X, f32(0)).astype(f32)
    ctx.set_state(map=M, sigma=S, hits=hits)
    ctx.upload_chunk(X0)
    for min_hits in (0, 3):
        unmasked = ctx.similarity(min_hits, 3)["bmu"]
        cpu_unmasked, cpu_masked = moved_by_the_mask(tr, X, M, valid, hits, min_hits)
        assert (unmasked == cpu_unmasked).all()
        assert (cpu_masked != cpu_unmasked).any()
        masked = ctx.similarity_masked(valid, min_hits, 3)["bmu"]
        assert (masked == cpu_masked).all() and (masked != unmasked).any()
    # NaN at an invalid position of a winning unit's map and sigmaMap rows: row r_star's unit b_star; and in every node at
    # the column that no row has valid
    r_star = 20
    b_star = int(ref.checker(tr, Xp, M, valid, hits, 0, [r_star])[0][0])
    c_star = int(np.flatnonzero(~valid[r_star])[0])
    Mn, Sn = M.copy(), S.copy()
    Mn[b_star, c_star] = Sn[b_star, c_star] = np.nan
    Mn[:, J - 1] = Sn[:, J - 1] = np.nan
    ctx.set_state(map=Mn, sigma=Sn)
    ctx.upload_chunk(Xp)
    for min_hits in (0, 3):
        bmu, dist = ref.checker(tr, Xp, Mn, valid, hits, min_hits)
        if min_hits == 0:
            assert bmu[r_star] == b_star
        b = bmu.astype(np.int64)
        for rule, floor in RULES:
            exp = ref.similarity(Xp, Mn[b], Sn[b], 3, floor, valid)
            exp.update(bmu=bmu, dist=dist, nvalid=valid.sum(axis=1).astype(np.uint32))
            got = ctx.similarity_masked(valid, min_hits, 3, rule, delta=True)
            same(got, exp, SIM_KEYS, (min_hits, rule))
            nod = ctx.similarity_masked(valid, min_hits, 3, rule)
            assert nod["delta"] is None
            same(nod, exp, SIM_KEYS[:-1], (min_hits, rule, "no delta"))
            # a row without a valid column, a row with exactly one
            assert got["bmu"][11] == 0 and got["dist"][11].view(np.uint32) == 0 and got["nvalid"][11] == 0
            assert got["dmax"][11] == -np.inf and got["dmax_col"][11] == sr.NONE and got["first"][11].view(np.uint32) == sr.QNAN
            assert got["amax"][11].view(np.uint32) == 0 and got["amax_col"][11] == sr.NONE and got["outside"][11] == 0
            assert (got["delta"][11].view(np.uint32) == 0).all()
            assert got["nvalid"][12] == 1 and got["dmax_col"][12] == J // 2
            assert np.isfinite(got["dist"]).all() and np.isfinite(got["delta"]).all()
            assert (got["delta"][~valid].view(np.uint32) == 0).all()
        for bn, what in ((binary, "mixed"), (only_r, "replaced")):
            got = ctx.evaluate_masked(valid, bn, continuous, min_hits=min_hits)
            assert (got["bmu"] == bmu).all() and beq(got["dist"], dist) and (got["nvalid"] == valid.sum(axis=1)).all()
            exact = check_evaluate(got, Xp, Mn[b], bn, continuous, valid, (tr, W, H, J, min_hits, what))
            if what == "replaced":
                assert exact.all() and (got["nrepl"] > 0).any()
            assert got["bsum"][11].view(np.uint32) == 0 and got["nrepl"][11] == 0
            assert np.isfinite(got["bsum"]).all() and np.isfinite(got["error"])
    ctx.close()


def test_evaluate_select_is_not_a_multiplication():
    """under an invalid column, a factor whose fp32 product with a replaced term overflows, and an infinite one: the term is
    +0 by select, where the unmasked call's multiplication by a zero val gives NaN"""
    tr, W, H, J = po.STANDARD, 7, 5, 9
    ctx, X, M, S, hits = make(tr, W, H, J, seed=21)
    Xp = X.copy()
    Xp[:, 4] = np.nan                                   # be of column 4 is NaN: replaced by -99999
    col = np.ones(J, bool)
    col[4] = False
    binary, continuous = column_factors(J, 2)
    binary[4] = f32(1e35)
    ctx.upload_chunk(Xp)
    bmu, dist = ref.checker(tr, Xp, M, col, hits, 0)
    got = ctx.evaluate_masked(col, binary, continuous)
    assert (got["bmu"] == bmu).all() and beq(got["dist"], dist)
    check_evaluate(got, Xp, M[bmu.astype(np.int64)], binary, continuous, col, "overflowing factor")
    assert np.isfinite(got["bsum"]).all()
    # an infinite factor: the unmasked call multiplies it by the zero val of the invalid column (NaN), the select does not
    Xq = Xp.copy()
    Xq[:, 4] = f32(0.5)                                 # (the unmasked search takes every value as present)
    ctx.upload_chunk(Xq)
    inf_b, zero_b = binary.copy(), binary.copy()
    inf_b[4], zero_b[4] = np.inf, 0
    assert np.isnan(ctx.evaluate(inf_b, continuous, valid=np.tile(col, (B, 1)))["bsum"]).all()
    a, b = ctx.evaluate_masked(col, inf_b, continuous), ctx.evaluate_masked(col, zero_b, continuous)
    same(a, b, EV_KEYS, "infinite factor under an invalid column")
    assert np.isfinite(a["bsum"]).all() and (a["bsum"] > 0).any() and ref.same_double(a["error"], b["error"])
    ctx.close()


# ---- 3. one_mask and sub-ranges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", SHAPES)
def test_one_mask_and_sub_ranges(tr, W, H, J):
    ctx, X, M, S, hits = make(tr, W, H, J, seed=11)
    rng = np.random.default_rng(J + 1)
    binary, continuous = column_factors(J, J + 3)
    col = rng.random(J) < 0.6
    col[0] = True
    a = ctx.similarity_masked(col, 2, 3, delta=True)
    same(a, ctx.similarity_masked(np.tile(col, (B, 1)), 2, 3, delta=True), SIM_KEYS, "column mask")
    assert (a["nvalid"] == col.sum()).all()
    ea = ctx.evaluate_masked(col, binary, continuous, min_hits=2)
    eb = ctx.evaluate_masked(np.tile(col, (B, 1)), binary, continuous, min_hits=2)
    same(ea, eb, EV_KEYS, "column mask")
    assert ref.same_double(ea["error"], eb["error"])
    valid = rng.random((B, J)) < 0.7
    full = ctx.similarity_masked(valid, 2, 3, delta=True)
    efull = ctx.evaluate_masked(valid, binary, continuous, min_hits=2)
    for r0, r1 in ((0, 70), (5, 69), (64, 70), (33, 34)):
        part = ctx.similarity_masked(valid[r0:r1], 2, 3, r0=r0, r1=r1, delta=True)     # the mask counts from r0
        one = ctx.similarity_masked(col, 2, 3, r0=r0, r1=r1, delta=True)
        epart = ctx.evaluate_masked(valid[r0:r1], binary, continuous, min_hits=2, r0=r0, r1=r1)
        eone = ctx.evaluate_masked(col, binary, continuous, min_hits=2, r0=r0, r1=r1)
        for k in SIM_KEYS:
            assert part[k].shape[0] == r1 - r0 and beq(part[k], full[k][r0:r1]), (k, r0, r1)
            assert beq(one[k], a[k][r0:r1]), (k, r0, r1)
        for k in EV_KEYS:
            assert beq(epart[k], efull[k][r0:r1]) and beq(eone[k], ea[k][r0:r1]), (k, r0, r1)
        assert ref.same_double(epart["error"], ref.running_mean(epart["dist"], epart["bsum"]))      # counted from r0
    empty = ctx.similarity_masked(valid[7:7], 2, 3, r0=7, r1=7, delta=True)
    assert empty["bmu"].shape == (0,) and empty["delta"].shape == (0, J)
    e = ctx.evaluate_masked(valid[7:7], binary, continuous, r0=7, r1=7)
    assert e["bsum"].shape == (0,) and e["error"] == 0.0
    err = np.full(1, 5.0)
    out = capi.EvaluateMaskedOut()
    out.error = err.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    v = np.ones(J, np.uint8)
    assert capi.lib().vsom_evaluate_masked_batch(ctx._h, 0, 7, 7, capi._f(binary), capi._f(continuous),
                                                 v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 1, ctypes.byref(out)) == 0
    assert err[0] == 0.0                               # an empty range writes *error = 0
    ctx.close()


# ---- 4. slices ------------------------------------------------------------------------------------------------------------
def test_row_slices(monkeypatch):
    """a slice forced to 100 rows (VSOM_MASKED_SLICE_ROWS, read at every call): 333 rows cross it three times, the last
    slice ragged in rows, in its row tile and in the scorer's workgroups"""
    tr, W, H, J, rows = po.STANDARD, 9, 15, 37, 333
    ctx, X, M, S, hits = make(tr, W, H, J, seed=17, rows=rows)
    rng = np.random.default_rng(9)
    valid = rng.random((rows, J)) < 0.7
    col = rng.random(J) < 0.6
    binary, continuous = column_factors(J, 4)
    masks = {"valid": valid, "col": col}

    def run():
        return ({k: ctx.similarity_masked(m, 2, 3, delta=True) for k, m in masks.items()},
                {k: ctx.similarity_masked(m, 2, 3) for k, m in masks.items()},
                {k: ctx.evaluate_masked(m, binary, continuous, min_hits=2) for k, m in masks.items()})

    whole = run()
    monkeypatch.setenv("VSOM_MASKED_SLICE_ROWS", "100")
    sliced = run()
    part = ctx.similarity_masked(valid[50:301], 2, 3, r0=50, r1=301, delta=True)
    epart = ctx.evaluate_masked(valid[50:301], binary, continuous, min_hits=2, r0=50, r1=301)
    monkeypatch.delenv("VSOM_MASKED_SLICE_ROWS")
    for k in masks:
        same(sliced[0][k], whole[0][k], SIM_KEYS, (k, "delta"))
        same(sliced[1][k], whole[1][k], SIM_KEYS, (k, "no delta"))
        same(sliced[2][k], whole[2][k], EV_KEYS, (k, "evaluate"))
        assert ref.same_double(sliced[2][k]["error"], whole[2][k]["error"])
    for k in SIM_KEYS:
        assert beq(part[k], whole[0]["valid"][k][50:301]), k
    for k in EV_KEYS:
        assert beq(epart[k], whole[2]["valid"][k][50:301]), k
    sample = [0, 63, 64, 99, 100, 101, 127, 128, 199, 200, 255, 256, 299, 300, 320, 332]   # 16 rows around the borders
    for k, m in masks.items():
        exp = expect_similarity(tr, X, M, S, m, hits, 2, 3, True, sample)
        for f in SIM_KEYS:
            assert beq(sliced[0][k][f][sample], exp[f]), (k, f)
        b = exp["bmu"].astype(np.int64)
        v = m if m.ndim == 1 else m[sample]
        b64, n64 = ref.evaluate64(X[sample], M[b], binary, continuous, v)
        got = sliced[2][k]
        assert (got["bmu"][sample] == exp["bmu"]).all() and (got["nrepl"][sample] == n64).all()
        nz = b64 != 0
        assert (np.abs(got["bsum"][sample][nz] - b64[nz]) / b64[nz] <= ref.bound(J)).all()
    ctx.close()


# ---- 5. engineered sigma rows ---------------------------------------------------------------------------------------------
def special_sigmas():
    """the sigma values of tests/test_gpu_similarity.py's engineered case, restated"""
    e = f32(0.00001)
    return np.array([0.0, 1e-42, 1.4e-45, e, np.nextafter(e, f32(1)), np.nextafter(e, f32(0)), np.nan, np.inf, -1.0, -0.0,
                     0.5, 3.0e-6, 2.0, 1e-30, -np.inf, 7.0e-3], f32)


@pytest.mark.parametrize("tr", KINDS)
def test_engineered_sigma_map_and_rows(tr):
    W, H, J, rows = 5, 4, 16, 48
    N = W * H
    rng = np.random.default_rng(11)
    m = gen.random_map(N, J, seed=8)
    sg = np.stack([np.roll(np.resize(special_sigmas(), J), n) for n in range(N)]).astype(f32)
    m[3, 1] = np.nan
    m[5, 2] = np.inf
    m[7, 0] = -np.inf
    hits = (np.arange(N) % 3).astype(np.uint64)
    X = gen.blobs(rows, J, 4, 4, 2)
    X[:N] = np.where(np.isfinite(m), m, f32(0.25))     # rows that sit on a node: delta = 0 / 0-over-0 columns
    X[2, 1] = np.nan
    X[4, 3] = np.inf
    X[6, 0] = -np.inf
    X[9, :] = np.nan
    valid = rng.random((rows, J)) < 0.8
    # row 30 sits on node 11 but for +0.25 in columns 5 and 9, which share one model value and one sigma: a tie for amax
    # between column 5 (invalid) and column 9 (valid); column 0 invalid as well: `first` comes from column 1
    tie, node = 30, 11
    m[node, 5] = m[node, 9] = f32(0.5)
    sg[node, 5] = sg[node, 9] = f32(0.5)
    m[node, :2] = f32(0.25)
    sg[node, :2] = f32(2.0)
    X[tie] = m[node]
    X[tie, [5, 9]] = f32(0.75)
    X[tie, 0] = f32(0.75)
    X[tie, 1] = f32(0.375)
    valid[tie] = True
    valid[tie, [0, 5]] = False
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=m, sigma=sg, hits=hits)
    ctx.upload_chunk(X)
    for ns in (1, 3, 1000000, 0, -2):
        for rule, floor in RULES:
            for min_hits in (0, 1, 2):
                exp = expect_similarity(tr, X, m, sg, valid, hits, min_hits, ns, floor)
                got = ctx.similarity_masked(valid, min_hits, ns, rule, delta=True)
                same(got, exp, SIM_KEYS, (tr, ns, floor, min_hits))
                for k in ("dist", "first"):            # NaN is stored as the quiet NaN 0x7FC00000
                    assert (got[k].view(np.uint32)[np.isnan(got[k])] == sr.QNAN).all(), k
    got = ctx.similarity_masked(valid, 2, 1, capi.SIGMA_FLOOR, delta=True)
    assert got["bmu"][tie] == node                     # (hits[11] = 2)
    assert got["amax_col"][tie] == 9 and got["amax"][tie] == f32(0.5)
    assert got["first"][tie] == f32(0.0625) and got["first"][tie] == got["delta"][tie, 1] and got["delta"][tie, 0] == 0
    allv = ctx.similarity_masked(np.ones((rows, J), bool), 2, 1, capi.SIGMA_FLOOR)
    assert allv["bmu"][tie] == node and allv["amax_col"][tie] == 5      # with every column valid the lower one wins the tie
    ctx.close()


def test_on_the_interval_bounds_counts_as_inside():
    tr, W, H, J = po.STANDARD, 3, 3, 8
    m = gen.random_map(W * H, J, seed=2)
    sg = (np.abs(gen.random_map(W * H, J, seed=3)) + f32(0.01)).astype(f32)
    hits = np.ones(W * H, np.uint64)
    sk = (sg * f32(3)).astype(f32)
    up = f32(np.inf)
    X = np.concatenate([(m + sk).astype(f32), (m - sk).astype(f32), np.nextafter((m + sk).astype(f32), up),
                        np.nextafter((m - sk).astype(f32), -up)])
    valid = np.random.default_rng(5).random((36, J)) < 0.7
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=m, sigma=sg, hits=hits)
    ctx.upload_chunk(X)
    got = ctx.similarity_masked(valid, 1, 3, capi.SIGMA_FLOOR, delta=True)
    exp = expect_similarity(tr, X, m, sg, valid, hits, 1, 3, True)
    same(got, exp, SIM_KEYS, "bounds")
    own = got["bmu"] == np.tile(np.arange(9), 4)       # rows whose unit is the node they were built from
    assert own[:18].any() and own[18:].any()
    assert (got["outside"][:18][own[:18]] == 0).all()
    assert (got["outside"][18:][own[18:]] == got["nvalid"][18:][own[18:]]).all()
    ctx.close()


# ---- 6. NaN d_0 pins node 0 under a mask ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9)])
def test_nan_node_zero_pins_the_bmu(tr, W, H, J):
    ctx, X, M, S, hits = make(tr, W, H, J, seed=9)
    rng = np.random.default_rng(J)
    binary, continuous = column_factors(J, 1)
    valid = rng.random((B, J)) < 0.7
    valid[:, 1] = True
    valid[:35, 4] = False                              # column 4: invalid for the first half of the rows
    M0 = M.copy()
    M0[0, 1] = np.nan                                  # NaN at a valid column of node 0: node 0, NaN distance
    ctx.set_state(map=M0)
    for min_hits in (0, 3):
        got = ctx.similarity_masked(valid, min_hits, 3, delta=True)
        same(got, expect_similarity(tr, X, M0, S, valid, hits, min_hits, 3, True), SIM_KEYS, ("node 0 NaN", min_hits))
        assert (got["bmu"] == 0).all() and (got["dist"].view(np.uint32) == sr.QNAN).all()
        assert (got["delta"][:, 1] == 0).all() and (got["dmax_col"] != 1).all()
        ev = ctx.evaluate_masked(valid, binary, continuous, min_hits=min_hits)
        assert (ev["bmu"] == 0).all() and (ev["dist"].view(np.uint32) == sr.QNAN).all() and np.isnan(ev["error"])
    M1 = M.copy()
    M1[0, 4] = np.nan                                  # the same under an invalid column is ignored
    ctx.set_state(map=M1)
    got = ctx.similarity_masked(valid, 0, 3, delta=True)
    same(got, expect_similarity(tr, X, M1, S, valid, hits, 0, 3, True), SIM_KEYS, "node 0 NaN, masked")
    assert np.isfinite(got["dist"][:35]).all() and (got["bmu"][:35] != 0).any()
    assert (got["bmu"][35:][valid[35:, 4]] == 0).all()
    ctx.close()


# ---- 7. read-only ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J", [(po.STANDARD, 9, 15, 37), (po.MEDIAN, 7, 5, 9)])
def test_read_only(tr, W, H, J):
    X = gen.blobs(B, J, 4, 15, 2)
    init = gen.random_map(W * H, J, seed=16)
    ctx = vsom_amd.Context(W, H, J, tr)
    o = po.OracleSom(W, H, J, tr)
    ctx.set_state(map=init)
    o.set_state(map=init)
    ctx.upload_chunk(X)
    lbo = np.zeros(B, np.uint64)
    assert f32(ctx.batch_epoch(3.0, True)) == f32(o.batch_epoch(X, lbo, 3.0, True))
    before, lb, sq = ctx.get_state(), ctx.get_last_bmu(), ctx.get_sqres()
    valid = np.random.default_rng(3).random((B, J)) < 0.7
    binary, continuous = column_factors(J, 2)
    a = ctx.similarity_masked(valid, 1, 3, delta=True)
    ea = ctx.evaluate_masked(valid, binary, continuous, min_hits=1)
    ctx.similarity_masked(valid[0], 0, 3, r0=10, r1=50)
    ctx.evaluate_masked(valid[0], binary, continuous, r0=10, r1=50)
    same(ctx.similarity_masked(valid, 1, 3, delta=True), a, SIM_KEYS, "repeated")
    same(ctx.evaluate_masked(valid, binary, continuous, min_hits=1), ea, EV_KEYS, "repeated")
    assert (a["bmu"] != lb).any()                      # (the calls did search: their units are not lastBMU's)
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    assert (ctx.get_last_bmu() == lb).all() and (lb == lbo).all() and beq(ctx.get_sqres(), sq)
    assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], X)      # the chunk, read back
    assert f32(ctx.batch_epoch(2.0, False)) == f32(o.batch_epoch(X, lbo, 2.0, False))
    st = ctx.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want), ("the epoch after the masked scorers", k)
    assert (ctx.get_last_bmu() == lbo).all()
    ctx.close()


# ---- 8. a pending sigmaMap is materialised --------------------------------------------------------------------------------
def test_lazy_sigma_is_materialised():
    W = H = 40
    J, rows = 300, 77
    init = gen.random_map(W * H, J, 42) * f32(100)
    X = gen.mnist_like(rows, 3, J)
    valid = np.random.default_rng(8).random((rows, J)) < 0.7
    binary, continuous = column_factors(J, 5)
    res = {}
    for mode in (capi.SIGMA_LAZY, capi.SIGMA_EAGER):
        for call in ("similarity", "evaluate"):
            ctx = vsom_amd.Context(W, H, J, capi.STANDARD)
            ctx.set_sigma_mode(mode)
            ctx.set_column_compaction(1)
            ctx.set_state(map=init)
            ctx.upload_chunk(X)
            ctx.batch_epoch(6.0, True)
            s = ctx.sigma_stats()
            assert s["pending"] == (mode == capi.SIGMA_LAZY), (mode, s)
            if call == "similarity":
                out = ctx.similarity_masked(valid, 1, 3, delta=True)
            else:
                out = ctx.evaluate_masked(valid, binary, continuous)
            s = ctx.sigma_stats()
            assert not s["pending"] and s["materialised"] == (1 if mode == capi.SIGMA_LAZY else 0), (mode, call, s)
            res[mode, call] = (out, ctx.get_state(S=False))
            ctx.close()
    same(res[capi.SIGMA_LAZY, "similarity"][0], res[capi.SIGMA_EAGER, "similarity"][0], SIM_KEYS, "lazy against eager")
    same(res[capi.SIGMA_LAZY, "evaluate"][0], res[capi.SIGMA_EAGER, "evaluate"][0], EV_KEYS, "lazy against eager")
    assert np.isfinite(res[capi.SIGMA_LAZY, "similarity"][0]["amax"]).all()
    for call in ("similarity", "evaluate"):
        a, b = res[capi.SIGMA_LAZY, call][1], res[capi.SIGMA_EAGER, call][1]
        for k in ("map", "sigma", "weight", "hits"):
            assert beq(a[k], b[k]), (call, k)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, rows = 6, 5, 7, 20
    init = gen.random_map(W * H, J, seed=1)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    L = capi.lib()
    u8 = ctypes.POINTER(ctypes.c_uint8)
    valid = np.ones((rows, J), np.uint8)
    binary, continuous = np.ones(J, f32), np.ones(J, f32)
    bmu, ebmu = np.zeros(rows, np.uint64), np.zeros(rows, np.uint64)
    sout, eout = capi.SimilarityMaskedOut(), capi.EvaluateMaskedOut()
    sout.bmu = capi._u(bmu)
    eout.bmu = capi._u(ebmu)
    NULL = object()

    def sim(r0, r1, h=ctx._h, v=valid, o=sout, rule=1):
        return L.vsom_similarity_masked_batch(h, 0, 3, rule, r0, r1, None if v is None else v.ctypes.data_as(u8), 0,
                                              None if o is None else ctypes.byref(o))

    def ev(r0, r1, h=ctx._h, v=valid, o=eout, b=binary, c=continuous):
        return L.vsom_evaluate_masked_batch(h, 0, r0, r1, capi._f(b), capi._f(c), None if v is None else v.ctypes.data_as(u8), 0,
                                            None if o is None else ctypes.byref(o))

    def refused(code, word):
        assert code == -1, word
        assert word in L.vsom_last_error().decode(), (word, L.vsom_last_error().decode())

    for call in (sim, ev):
        refused(call(0, 0), "no chunk")
        refused(call(0, 1, h=None), "null context")
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.similarity_masked(valid, 0, 3, delta=True)
    egood = ctx.evaluate_masked(valid, binary, continuous)
    for call in (sim, ev):
        refused(call(0, rows, v=None), "valid_host")
        refused(call(0, rows, o=None), "out is null")
        for r0, r1 in ((5, 4), (0, rows + 1), (rows + 1, rows + 2)):
            refused(call(r0, r1), "row range")
    refused(sim(0, rows, rule=2), "sigma_rule")
    refused(sim(0, rows, rule=-1), "sigma_rule")
    refused(ev(0, rows, b=None), "binary_host")
    refused(ev(0, rows, c=None), "binary_host or continuous_host")
    same(ctx.similarity_masked(valid, 0, 3, delta=True), good, SIM_KEYS, "after refusals")
    same(ctx.evaluate_masked(valid, binary, continuous), egood, EV_KEYS, "after refusals")
    assert sim(3, 3) == 0 and ev(3, 3) == 0            # an empty range
    assert sim(0, rows) == 0 and (bmu == good["bmu"]).all()       # a single output pointer
    assert ev(0, rows) == 0 and (ebmu == egood["bmu"]).all()
    assert sim(0, rows, o=capi.SimilarityMaskedOut()) == 0 and ev(0, rows, o=capi.EvaluateMaskedOut()) == 0     # none at all
    o = po.OracleSom(W, H, J)
    o.set_state(map=init)
    lbo = np.zeros(rows, np.uint64)
    assert f32(ctx.batch_epoch(1.5, True)) == f32(o.batch_epoch(X, lbo, 1.5, True))
    st = ctx.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want), ("after refusals", k)
    ctx.close()

    # CLR contexts
    Xc = (np.abs(gen.blobs(rows, 5, 3, 1, 2)) + f32(0.5)).astype(f32)
    clr = vsom_amd.Context(4, 4, 5, po.CLR)
    oc = po.OracleSom(4, 4, 5, po.CLR)
    initc = gen.random_map(16, oc.depth, seed=2)
    clr.set_state(map=initc)
    oc.set_state(map=initc)
    clr.upload_chunk(Xc)
    with pytest.raises(capi.VsomError, match="vsom_similarity_masked_batch: CLR"):
        clr.similarity_masked(np.ones((rows, 5), np.uint8), 0, 3)
    with pytest.raises(capi.VsomError, match="vsom_evaluate_masked_batch: CLR"):
        clr.evaluate_masked(np.ones((rows, 5), np.uint8), np.ones(5, f32), np.ones(5, f32))
    assert f32(clr.batch_epoch(1.5, True)) == f32(oc.batch_epoch(Xc, lbo, 1.5, True))
    stc = clr.get_state()
    for k, want in (("map", oc.map), ("sigma", oc.sigma), ("weight", oc.weight), ("hits", oc.hits)):
        assert beq(stc[k], want), ("CLR after the refusals", k)
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_similarity_masked_batch"):
        cu.similarity_masked(np.ones((10, 5), np.uint8), 0, 3)
    with pytest.raises(capi.VsomError, match="vsom_evaluate_masked_batch"):
        cu.evaluate_masked(np.ones((10, 5), np.uint8), np.ones(5, f32), np.ones(5, f32))
    cu.bmu_batch()
    cu.close()

    # a chunk staged ahead (as tests/test_gpu_masked.py): refused until it is committed
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * f32(100) + f32(100)).astype(f32)
    big = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    big.set_state(map=init)
    big.upload_chunk(xs[0])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.similarity_masked(np.ones(J, np.uint8), 0, 3)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.evaluate_masked(np.ones(J, np.uint8), np.zeros(J, f32), np.ones(J, f32))
    big.commit_chunk()
    got = big.similarity_masked(np.ones(J, np.uint8), 0, 3, r0=0, r1=4)
    egot = big.evaluate_masked(np.ones(J, np.uint8), np.zeros(J, f32), np.ones(J, f32), r0=0, r1=4)
    bi, bd = big.bmu_batch()
    assert (got["bmu"] == bi[:4]).all() and beq(got["dist"], bd[:4])
    assert (egot["bmu"] == bi[:4]).all() and beq(egot["dist"], bd[:4])
    big.close()
    pb.free()


# ---- 10. mirrors ----------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with validity flags"""

    def __init__(self, X, validity):
        super().__init__(X)
        self.validity = validity


def test_som_mirrors():
    tr, W, H, J, rows = po.STANDARD, 9, 15, 37, 70
    M, S, hits = unit_state(W, H, J, 21)
    X = unit_rows(rows, J, 22)
    valid = np.random.default_rng(4).random((rows, J)) < 0.7
    valid[0, :] = False                                # the first row reports nothing: the finish starts at the next one
    X = np.where(valid, X, f32(np.nan)).astype(f32)
    binary, continuous = column_factors(J, 6)
    s = vs.Som(W, H, J)
    s.setState(map=M, sigma=S, hits=hits)
    ds = ValidDataSet(X, valid)
    ds.loadNextDataFromStream()
    for min_hits in (0, 3):
        bmu, dist = ref.checker(tr, X, M, valid, hits, min_hits)
        b = bmu.astype(np.int64)
        for ns in (1, 3, 1000000):
            # measureSimilarityMasked: the reference's select as written, finished as the literal loop over the masked delta
            delta, lo, hi = sr.columns(X, M[b], S[b], ns, False)
            want_row, want_ok = sr.literal_loop(ref.masked_delta(delta, valid), X, lo, hi, valid)
            rep = s.similarityRowsMasked(ds, ns, min_hits, floor=False, delta=True)
            exp = ref.similarity(X, M[b], S[b], ns, False, valid)
            exp.update(bmu=bmu, dist=dist, nvalid=valid.sum(axis=1).astype(np.uint32))
            same(rep, exp, SIM_KEYS, (min_hits, ns))
            row, ok = vs.measure_similarity_from_rows(rep["first"], rep["dmax"], rep["outside"])
            assert (row, ok) == (want_row, want_ok) and row != 0
            assert want_ok == (ns == 1000000)
            assert s.measureSimilarityMasked(ds, ns, min_hits) == want_ok
        rows_rep = s.evaluateRowsMasked(ds, binary, continuous, min_hits)
        assert (rows_rep["bmu"] == bmu).all() and beq(rows_rep["dist"], dist)
        check_evaluate(rows_rep, X, M[b], binary, continuous, valid, ("Som", min_hits))
        e = s.evaluateMasked(ds, binary, continuous, min_hits)
        assert ref.same_double(e, ref.running_mean(rows_rep["dist"], rows_rep["bsum"]))
    # no validity attribute: every column counts, and the calls are the unmasked ones
    Xc = unit_rows(rows, J, 23)
    plain = s.similarityRowsMasked(Xc, 3, 3, delta=True)
    same(plain, s.similarityRows(Xc, 3, 3, delta=True), ("bmu", "dist") + ref.ROW_KEYS + ("delta",), "no validity")
    assert (plain["nvalid"] == J).all()
    assert s.measureSimilarityMasked(Xc, 3, 1) == s.measureSimilarity(Xc, 3, 1)
    assert ref.same_double(s.evaluateMasked(Xc, binary, continuous), s.evaluate(Xc, binary, continuous))
    # empty data
    none = Xc[:0]
    assert s.measureSimilarityMasked(none, 3, 1) is True and s.evaluateMasked(none) == 0.0
    assert s.similarityRowsMasked(none, 3, 1, delta=True)["delta"].shape == (0, J)
    assert s.evaluateRowsMasked(none)["nvalid"].shape == (0,)
    s.close()


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_masked_score_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "state_downloads=0" in res.stdout
    assert "host_masked_score_test ok" in res.stdout
