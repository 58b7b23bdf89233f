"""GPU: vsom_generate_masked_batch -- K records per chunk row, each around a unit drawn from the row's distribution over its
VALID columns, with the observed columns kept.  Units are vsom_bmd_masked_batch's draws bit for bit; kept columns are the row's
own values bit for bit (with NaN as their L); sampled columns are held against the float64 decode of tests/generate_ref.py
within the bound include/vsom_hip.h derives (assumptions Ld = Lh = 1), the exact cases exactly.  Shapes as
tests/test_gpu_bmd_masked.py, with 1, 3 and 7 draws per row."""
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
import bmd_masked_ref as ref  # noqa: E402
import custom_hooks as hooks  # noqa: E402
import gen  # noqa: E402
import generate_ref as gr  # noqa: E402
from similarity_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
f32 = np.float32
B = ref.B
NO_UNIT = ref.NO_UNIT


def context(c, X=None):
    ctx = vsom_amd.Context(c["W"], c["H"], c["J"], c["tr"])
    ctx.set_state(map=c["M"], sigma=c["S"], hits=c["hits"])
    ctx.upload_chunk(c["X"] if X is None else X)
    return ctx


def logits(n, K, J, seed):
    """L in (0, 1) away from the ends"""
    return np.random.default_rng(seed).integers(1, 1000, (n, K, J)).astype(np.float64) / 1000.0


def same(a, b, what=None):
    assert (a["unit"] == b["unit"]).all(), (what, "unit")
    assert gr.beq(a["record"], b["record"]), (what, "record")


# ---- 1. nothing kept, one draw, an all-valid mask: generate(PER_ROW) ------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_all_valid_equals_generate_per_row(tr, W, H, J):
    c = ref.case(tr, W, H, J)
    ctx = context(c, ref.unit_rows(B, J, 77))
    u = c["U"][:, 0]
    L = logits(B, 1, J, 5)
    L[3, 0, 0], L[4, 0, J - 1], L[6, 0, 0] = 0.0, 1.0, np.nan           # -inf, +inf, NaN: propagated alike
    for min_hits in ref.MIN_HITS:
        want = ctx.generate(min_hits, u, L[:, 0, :], capi.GENERATE_PER_ROW)
        for valid in (np.ones((B, J), np.uint8), np.ones(J, np.uint8)):
            got = ctx.generate_masked(valid, min_hits, u, L, keep_observed=False)
            assert got["unit"].shape == (B, 1) and got["record"].shape == (B, 1, J)
            assert (got["unit"][:, 0] == want["unit"]).all() and gr.beq(got["record"][:, 0, :], want["record"]), min_hits
    ctx.close()


# ---- 5. units, kept columns, sampled columns ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", ref.DRAWS)
@pytest.mark.parametrize("tr,W,H,J", ref.SHAPES)
def test_random_masks(tr, W, H, J, K):
    c = ref.case(tr, W, H, J)
    ctx = context(c)
    U = c["U"][:, :K]
    valid = c["valid"]
    st = ctx.get_state()
    L = logits(B, K, J, 9 + K)
    L[np.broadcast_to(valid[:, None, :], L.shape)] = np.nan             # NaN at every column that is kept
    for min_hits in ref.MIN_HITS:
        got = ctx.generate_masked(valid, min_hits, U, L, draws=K)
        assert got["unit"].shape == (B, K) and got["record"].shape == (B, K, J)
        for k in range(K):                                              # the units: restricted_bmd_masked's draws, bit for bit
            d = ctx.restricted_bmd_masked(valid, min_hits, u=np.ascontiguousarray(U[:, k]))["draw"]
            assert (got["unit"][:, k] == d).all(), (min_hits, k)
        assert (got["unit"] != NO_UNIT).all()
        rec, zs, kept = ref.records(st["map"], st["sigma"], got["unit"], L, c["X"], valid, True)
        assert kept.sum() == K * valid.sum()
        x64 = np.broadcast_to(c["X"].astype(np.float64)[:, None, :], rec.shape)
        assert (got["record"][kept].view(np.uint64) == x64[kept].view(np.uint64)).all()     # kept: the row's value
        ok, worst = gr.within(got["record"], rec, zs)
        print(f"[generate_masked] {tr}/{W}x{H}x{J}/K={K}/min_hits={min_hits}: worst error {worst:.3f} of its bound")
        assert ok, worst
        assert np.isfinite(got["record"]).all()
        # a call with K draws is K calls with one
        for k in range(K):
            one = ctx.generate_masked(valid, min_hits, np.ascontiguousarray(U[:, k]), np.ascontiguousarray(L[:, k, :]))
            assert (one["unit"][:, 0] == got["unit"][:, k]).all() and gr.beq(one["record"][:, 0], got["record"][:, k]), k
    # nothing kept: every column sampled, the NaN of L propagated
    free = ctx.generate_masked(valid, 0, U, L, draws=K, keep_observed=False)
    rec, zs, kept = ref.records(st["map"], st["sigma"], free["unit"], L, c["X"], valid, False)
    assert not kept.any() and gr.within(free["record"], rec, zs)[0]
    assert np.isnan(free["record"][np.broadcast_to(valid[:, None, :], L.shape)]).all()
    ctx.close()


def test_exact_cases_and_draws_without_mass():
    tr, W, H, J, K = po.STANDARD, 9, 15, 9, 3
    c = ref.case(tr, W, H, J)
    S = c["S"].copy()
    S[:, 4] = 0                                                         # s = 0: rec = m for every finite g
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=c["M"], sigma=S, hits=c["hits"])
    ctx.upload_chunk(c["X"])
    valid = c["valid"].copy()
    valid[:, :6] = False                                                # columns 0..5 are sampled in every row
    U = c["U"][:, :K]
    L = logits(B, K, J, 3)
    L[:, :, 0] = 0.5                                                    # q = 1, g = +0: rec = m
    L[:, :, 1] = 0.0                                                    # g = -inf
    L[:, :, 2] = 1.0                                                    # q = inf
    L[:, :, 3] = np.nan
    L[:, 1, 5] = 1.5                                                    # q < 0: log gives NaN
    got = ctx.generate_masked(valid, 0, U, L, draws=K)
    unit = got["unit"].astype(np.int64)
    m64 = c["M"].astype(np.float64)
    assert (got["unit"] != NO_UNIT).all()
    assert (got["record"][:, :, 0].view(np.uint64) == m64[unit, 0].view(np.uint64)).all()
    assert (got["record"][:, :, 4].view(np.uint64) == m64[unit, 4].view(np.uint64)).all()
    s1, s2 = S[unit, 1], S[unit, 2]
    assert (got["record"][:, :, 1][s1 > 0] == -np.inf).all() and (got["record"][:, :, 2][s2 > 0] == np.inf).all()
    assert np.isnan(got["record"][:, :, 3]).all() and np.isnan(got["record"][:, 1, 5]).all()
    rec, zs, kept = ref.records(c["M"], S, got["unit"], L, c["X"], valid, True)
    assert gr.within(got["record"], rec, zs)[0]
    # no node has the hits: no mass, no unit, the quiet NaN in every column, the observed ones included
    none = ctx.generate_masked(c["valid"], 6, U, L, draws=K)
    assert (none["unit"] == NO_UNIT).all() and (none["record"].view(np.uint64) == ref.QNAN_BITS).all()
    # a NaN at a valid column of one row: that row alone has no mass
    Xn = np.where(c["valid"], c["X"], f32(0.5)).astype(f32)
    Xn[11, 7] = np.nan
    ctx.upload_chunk(Xn)
    part = ctx.generate_masked(np.ones(J, np.uint8), 0, U, L, draws=K)
    assert (part["unit"][11] == NO_UNIT).all() and (part["record"][11].view(np.uint64) == ref.QNAN_BITS).all()
    assert (np.delete(part["unit"], 11, axis=0) != NO_UNIT).all()
    ctx.close()


# ---- 6. column mask and sub-ranges --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J,K", [(po.STANDARD, 9, 15, 37, 3), (po.MEDIAN, 17, 16, 9, 7)])
def test_one_mask_and_sub_ranges(tr, W, H, J, K):
    c = ref.case(tr, W, H, J)
    ctx = context(c, np.where(c["valid"], c["X"], f32(0.5)).astype(f32))
    U = c["U"][:, :K]
    L = logits(B, K, J, 21)
    col = c["valid"][1]
    full = ctx.generate_masked(c["valid"], 3, U, L, draws=K)
    one = ctx.generate_masked(col, 3, U, L, draws=K)
    same(ctx.generate_masked(np.repeat(col[None], B, axis=0), 3, U, L, draws=K), one, "1-D mask against its rows")
    assert not gr.beq(one["record"], full["record"])
    for want, v in ((full, c["valid"]), (one, col)):
        pieces = []
        for r0, r1 in ((0, 1), (1, 5), (5, 5), (5, 63), (63, 70)):
            vv = v if v.ndim == 1 else v[r0:r1]
            pieces.append(ctx.generate_masked(vv, 3, U[r0:r1], L[r0:r1], draws=K, r0=r0, r1=r1))
            assert pieces[-1]["unit"].shape == (r1 - r0, K) and pieces[-1]["record"].shape == (r1 - r0, K, J)
        same({k: np.concatenate([p[k] for p in pieces]) for k in ("unit", "record")}, want, "pieces")
    ctx.close()


# ---- 7. slices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr,W,H,J,K", [(po.STANDARD, 17, 16, 37, 3)])
def test_row_slices(monkeypatch, tr, W, H, J, K):
    c = ref.case(tr, W, H, J)
    ctx = context(c, np.where(c["valid"], c["X"], f32(0.5)).astype(f32))
    U = c["U"][:, :K]
    L = logits(B, K, J, 22)
    col = c["valid"][1]
    want = ctx.generate_masked(c["valid"], 3, U, L, draws=K)
    want1 = ctx.generate_masked(col, 3, U, L, draws=K)
    # each override alone, then both at once (20: a pitch of 24 for 20 rows; 64: the tile, then 6 rows)
    for env in ({"VSOM_MASKED_SLICE_ROWS": "20"}, {"VSOM_GENERATE_SLICE_ROWS": "20"}, {"VSOM_GENERATE_SLICE_ROWS": "1"},
                {"VSOM_MASKED_SLICE_ROWS": "64"}, {"VSOM_MASKED_SLICE_ROWS": "20", "VSOM_GENERATE_SLICE_ROWS": "20"}):
        monkeypatch.delenv("VSOM_MASKED_SLICE_ROWS", raising=False)
        monkeypatch.delenv("VSOM_GENERATE_SLICE_ROWS", raising=False)
        for name, rows in env.items():
            monkeypatch.setenv(name, rows)
        same(ctx.generate_masked(c["valid"], 3, U, L, draws=K), want, env)
        same(ctx.generate_masked(col, 3, U, L, draws=K), want1, (env, "column mask"))
        part = ctx.generate_masked(c["valid"][7:66], 3, U[7:66], L[7:66], draws=K, r0=7, r1=66)
        same(part, {k: want[k][7:66] for k in want}, (env, "sub-range"))
    ctx.close()


# ---- 8. read-only; a pending sigmaMap is materialised -------------------------------------------------------------------------
def test_read_only():
    tr, W, H, J, K = po.STANDARD, 9, 15, 37, 3
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
    U = np.random.default_rng(4).random((B, K))
    L = logits(B, K, J, 23)
    a = ctx.generate_masked(valid, 1, U, L, draws=K)
    ctx.generate_masked(valid[0], 0, U[10:50], L[10:50], draws=K, r0=10, r1=50)
    same(ctx.generate_masked(valid, 1, U, L, draws=K), a, "repeated")
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]), k
    assert (ctx.get_last_bmu() == lb).all() and (lb == lbo).all() and beq(ctx.get_sqres(), sq)
    assert beq(ctx.bmu_masked(np.ones(J, np.uint8), fill=True)["fill"], X)      # the chunk, read back
    assert f32(ctx.batch_epoch(2.0, False)) == f32(o.batch_epoch(X, lbo, 2.0, False))
    st = ctx.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want), ("the epoch after generate_masked", k)
    assert (ctx.get_last_bmu() == lbo).all()
    ctx.close()


def test_lazy_sigma_is_materialised():
    W = H = 40
    J, rows, K = 300, 77, 2
    init = gen.random_map(W * H, J, 42) * f32(100)
    X = gen.mnist_like(rows, 3, J)
    valid = np.random.default_rng(8).random((rows, J)) < 0.7
    U = np.random.default_rng(9).random((rows, K))
    L = logits(rows, K, J, 24)
    res = {}
    for mode in (capi.SIGMA_LAZY, capi.SIGMA_EAGER):
        ctx = vsom_amd.Context(W, H, J, capi.STANDARD)
        ctx.set_sigma_mode(mode)
        ctx.set_column_compaction(1)
        ctx.set_state(map=init)
        ctx.upload_chunk(X)
        ctx.batch_epoch(6.0, True)
        s = ctx.sigma_stats()
        assert s["pending"] == (mode == capi.SIGMA_LAZY), (mode, s)
        out = ctx.generate_masked(valid, 0, U, L, draws=K)
        s = ctx.sigma_stats()
        assert not s["pending"] and s["materialised"] == (1 if mode == capi.SIGMA_LAZY else 0), (mode, s)
        res[mode] = (out, ctx.get_state(S=False))
        ctx.close()
    same(res[capi.SIGMA_LAZY][0], res[capi.SIGMA_EAGER][0], "lazy against eager")
    for k in ("map", "sigma", "weight", "hits"):
        assert beq(res[capi.SIGMA_LAZY][1][k], res[capi.SIGMA_EAGER][1][k]), k


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, rows, K = 6, 5, 7, 20, 2
    init = gen.random_map(W * H, J, seed=1)
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=init)
    lib = capi.lib()
    u8, dp = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_double)
    valid = np.ones((rows, J), np.uint8)
    U = np.full((rows, K), 0.5)
    L = logits(rows, K, J, 25)
    unit = np.zeros((rows, K), np.uint64)
    out = capi.GenerateOut()
    out.unit = capi._u(unit)

    def call(r0, r1, h=ctx._h, v=valid, uu=U, ll=L, o=out, draws=K):
        return lib.vsom_generate_masked_batch(h, 0, r0, r1, None if v is None else v.ctypes.data_as(u8), 0, draws, 1,
                                              None if uu is None else uu.ctypes.data_as(dp),
                                              None if ll is None else ll.ctypes.data_as(dp), None if o is None else ctypes.byref(o))

    def refused(code, word):
        assert code == -1, word
        assert word in lib.vsom_last_error().decode(), (word, lib.vsom_last_error().decode())

    refused(call(0, 0), "no chunk")
    refused(call(0, 1, h=None), "null context")
    X = gen.blobs(rows, J, 3, 1, 2)
    ctx.upload_chunk(X)
    good = ctx.generate_masked(valid, 0, U, L, draws=K)
    refused(call(0, rows, v=None), "valid_host")
    refused(call(0, rows, o=None), "out is null")
    refused(call(0, rows, uu=None), "u_host or l_host")
    refused(call(0, rows, ll=None), "u_host or l_host")
    refused(call(0, rows, draws=0), "draws")
    refused(call(0, rows, draws=65536), "draws")
    for r0, r1 in ((5, 4), (0, rows + 1), (rows + 1, rows + 2)):
        refused(call(r0, r1), "row range")
    for bad in (1.0, -0.125, np.nan):
        ub = U.copy()
        ub[rows - 1, K - 1] = bad
        refused(call(0, rows, uu=ub), "uniform " + str(rows * K - 1))
        assert call(0, rows - 1, uu=ub) == 0                # (outside the range: not read)
    same(ctx.generate_masked(valid, 0, U, L, draws=K), good, "after refusals")
    assert call(3, 3) == 0                                  # an empty range
    assert call(0, rows) == 0 and (unit == good["unit"]).all()          # a single output pointer
    assert call(0, rows, o=capi.GenerateOut()) == 0         # none at all
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
    clr.set_state(map=gen.random_map(16, clr.depth, seed=2))
    clr.upload_chunk(Xc)
    with pytest.raises(capi.VsomError, match="vsom_generate_masked_batch: CLR"):
        clr.generate_masked(np.ones((rows, 5), np.uint8), 0, np.full(rows, 0.5), np.full((rows, 5), 0.5))
    clr.bmu_batch()
    clr.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_generate_masked_batch"):
        cu.generate_masked(np.ones((10, 5), np.uint8), 0, np.full(10, 0.5), np.full((10, 5), 0.5))
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
        big.generate_masked(np.ones(J, np.uint8), 0, np.full(1100, 0.5), np.full((1100, J), 0.5))
    big.commit_chunk()
    got = big.generate_masked(np.ones(J, np.uint8), 0, np.full(4, 0.5), np.full((4, J), 0.25), keep_observed=False, r0=0, r1=4)
    want = big.generate(0, np.full(4, 0.5), np.full((4, J), 0.25), r0=0, r1=4)
    assert (got["unit"][:, 0] == want["unit"]).all() and gr.beq(got["record"][:, 0], want["record"])
    big.close()
    pb.free()


# ---- 10. mirrors ------------------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with validity flags"""

    def __init__(self, X, validity):
        super().__init__(X)
        self.validity = validity


def test_som_mirrors():
    tr, W, H, J, K = po.STANDARD, 9, 15, 37, 3
    c = ref.case(tr, W, H, J)
    X, valid, U = c["X"], c["valid"], c["U"][:, :K]
    L = logits(B, K, J, 26)
    s = vs.Som(W, H, J)
    s.setState(map=c["M"], sigma=c["S"], hits=c["hits"])
    ds = ValidDataSet(X, valid)
    ds.loadNextDataFromStream()
    for min_hits in ref.MIN_HITS:
        P, norm, prob, unit, near = ref.case_draws(c, min_hits)
        clear = near[:, :K] > ref.NEAR
        d = s.drawModelVectorsMasked(ds, min_hits, np.ascontiguousarray(U[:, 0]))
        assert (d[clear[:, 0]] == unit[:, 0][clear[:, 0]]).all()
        rep = s.generateRowsMasked(ds, min_hits, U, L, draws=K)
        assert (rep["unit"][clear] == unit[:, :K][clear]).all() and (rep["unit"][:, 0] == d).all()
        rec, zs, kept = ref.records(c["M"], c["S"], rep["unit"], L, X, valid, True)
        assert gr.within(rep["record"], rec, zs)[0]
        for r in (0, ref.NO_VALID_ROW, 69):
            p = s.findRestrictedBmdMasked(X[r], valid[r], min_hits)
            assert np.allclose(p, prob[r], rtol=1e-15, atol=0)
    imp = s.imputeSampled(ds, 0, draws=K, seed=5)
    assert imp.shape == (B, K, J) and np.isfinite(imp).all()
    x64 = np.broadcast_to(X.astype(np.float64)[:, None, :], imp.shape)
    vb = np.broadcast_to(valid[:, None, :], imp.shape)
    assert (imp[vb] == x64[vb]).all() and gr.beq(imp, s.imputeSampled(ds, 0, draws=K, seed=5))
    assert not gr.beq(imp, s.imputeSampled(ds, 0, draws=K, seed=6))
    # no validity attribute: every column counts -- the unmasked calls, and every column kept
    Xc = ref.unit_rows(B, J, 23)
    assert (s.drawModelVectorsMasked(Xc, 3, U[:, 0]) == s.drawModelVectors(Xc, 3, U[:, 0])).all()
    plain = s.generateRowsMasked(Xc, 3, U[:, 0], L[:, 0], keepObserved=False)
    want = s.generateRows(Xc, 3, U[:, 0], L[:, 0])
    assert (plain["unit"][:, 0] == want["unit"]).all() and gr.beq(plain["record"][:, 0], want["record"])
    assert gr.beq(s.imputeSampled(Xc, 3, draws=2, seed=1), np.repeat(Xc.astype(np.float64)[:, None, :], 2, axis=1))
    # empty data
    none = Xc[:0]
    assert s.drawModelVectorsMasked(none, 0, np.zeros(0)).shape == (0,)
    e = s.generateRowsMasked(none, 0, np.zeros((0, K)), np.zeros((0, K, J)), draws=K)
    assert e["unit"].shape == (0, K) and e["record"].shape == (0, K, J)
    assert s.imputeSampled(none, 0, draws=K).shape == (0, K, J)
    s.close()


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_bmd_masked_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "state_downloads=0" in res.stdout
    assert "host_bmd_masked_test ok" in res.stdout
