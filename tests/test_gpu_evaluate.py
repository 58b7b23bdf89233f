"""GPU: vsom_evaluate_batch -- Som::evaluate's search, per-row binary error and running mean in one call.
The search outputs are held bit for bit to vsom_bmu_batch, the running mean bit for bit to the recurrence over the returned
values, zero factors and replaced terms bit for bit to an fp32 restatement in Eigen's packet order (tests/evaluate_ref.py).
Only where the device's log decides a last bit is there a tolerance: bsum within (C + 2 L + 4) * 2^-24 relative of the
float64 restatement (include/vsom_hip.h; L = 1 taken as an assumption).  The largest relative distance seen is printed by
test_zz_report."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from vsom_amd import som as vs
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import custom_hooks as hooks  # noqa: E402
import evaluate_ref as ref  # noqa: E402
import gen  # noqa: E402
from evaluate_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROW_KEYS = ("bmu", "dist", "bsum", "nrepl")
TRS = (po.STANDARD, po.MEDIAN, po.CLR)
WORST = {"rel": 0.0, "where": None, "rows": 0}


def depth_of(tr, J):
    return J * (J - 1) if tr == po.CLR else J


def unit_map(N, D, seed):
    return np.random.default_rng(seed).uniform(0.02, 0.98, (N, D)).astype(np.float32)


def unit_rows(B, J, seed):
    """rows in [0,1] with some columns exactly 0 and some exactly 1"""
    rng = np.random.default_rng(seed)
    X = rng.random((B, J)).astype(np.float32)
    X[:, rng.random(J) < 0.2] = np.float32(0)
    X[:, rng.random(J) < 0.2] = np.float32(1)
    X[rng.random((B, J)) < 0.1] = np.float32(1)
    return X


def column_factors(J, seed):
    rng = np.random.default_rng(seed)
    binary = (rng.random(J) < 0.5).astype(np.float32)
    binary[rng.integers(0, J)] = np.float32(1)          # at least one binary column
    continuous = (rng.random(J) < 0.85).astype(np.float32)
    continuous[np.flatnonzero(binary)[0]] = np.float32(1)
    return binary, continuous


def context(tr, W, H, J, B, seed=1):
    D = depth_of(tr, J)
    M = unit_map(W * H, D, seed)
    X = unit_rows(B, J, seed + 1)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M)
    ctx.upload_chunk(X)
    return ctx, M, X


def same(a, b):
    for k in ROW_KEYS:
        assert beq(a[k], b[k]) if a[k].dtype == np.float32 else (a[k] == b[k]).all(), k
    assert ref.same_double(a["error"], b["error"])


def check_tolerance(got, X, M, binary, continuous, valid, what):
    """bsum against the float64 restatement, within the derived bound; records the worst relative distance"""
    C = M.shape[1]
    b64, n64 = ref.restate64(X[:, :C], M, binary[:C], continuous[:C], None if valid is None else valid[:, :C])
    assert (got["nrepl"] == n64).all(), (what, got["nrepl"][:8], n64[:8])
    zero = b64 == 0
    assert (got["bsum"][zero] == 0).all(), what
    rel = np.abs(got["bsum"][~zero].astype(np.float64) - b64[~zero]) / b64[~zero]
    if rel.size:
        i = int(np.argmax(rel))
        print(f"evaluate {what}: C = {C}, worst relative distance {rel[i]:.3e} = {rel[i] * 2 ** 24:.2f} x 2^-24, "
              f"bound {ref.bound(C) * 2 ** 24:.0f} x 2^-24")
        WORST["rows"] += rel.size
        if rel[i] > WORST["rel"]:
            WORST["rel"], WORST["where"] = float(rel[i]), what
        r = np.flatnonzero(~zero)[i]
        assert rel[i] <= ref.bound(C), (what, "row", int(r), "bsum", float(got["bsum"][r]).hex(), "float64", b64[r].hex(),
                                        "x", X[r, :C].tolist(), "m", M[r].tolist())


# ---- 1. parity -------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 4, 3, 7), (4, 4, 7, 20), (6, 5, 9, 50), (7, 3, 12, 33), (4, 4, 15, 20), (9, 8, 37, 130), (16, 12, 100, 300)]


# (the J = 2 shape is there for CLR's two-part model rows: C = D = 2, column 1 lies in the second part)
@pytest.mark.parametrize("tr, W, H, J, B", [(tr,) + s for s in SHAPES for tr in TRS] + [(po.CLR, 3, 3, 2, 11)])
def test_parity(tr, W, H, J, B):
    ctx, M, X = context(tr, W, H, J, B, seed=J)
    C = min(J, M.shape[1])
    binary, continuous = column_factors(J, J + 3)
    valid = np.random.default_rng(J + 5).random((B, J)) < 0.6
    bi, bd = ctx.bmu_batch()
    for v in (None, valid):
        got = ctx.evaluate(binary, continuous, valid=v)
        assert (got["bmu"] == bi).all() and beq(got["dist"], bd)
        check_tolerance(got, X, M[bi.astype(np.int64)][:, :C], binary, continuous, v, (tr, W, H, J, B, v is not None))
        assert ref.same_double(got["error"], ref.running_mean(got["dist"], got["bsum"]))
        assert (got["bsum"] > 0).any()
    ctx.close()


# ---- 2. engineered exact cases ---------------------------------------------------------------------------------------------
def engineered(tr, J, nan_node0, all_binary):
    """model values 0, 1, -0.5, 2 (and NaN, +inf at node 0) in the binary columns against x of 0, 1 and 0.5: every counting
    term is replaced by -99999, every other one has a zero factor"""
    W, H, B = 4, 3, 29
    N, D = W * H, depth_of(tr, J)
    C = min(J, D)
    rng = np.random.default_rng(J * 7 + nan_node0)
    M = unit_map(N, D, J)
    binary = np.zeros(J, np.float32)
    cols = np.arange(C) if all_binary else np.unique(np.r_[0, C - 1, rng.integers(0, C, max(1, C // 2))])
    binary[cols] = rng.choice(np.array([1.0, 0.5, 2.0, 3.0], np.float32), cols.size)
    continuous = np.ones(J, np.float32)
    special = np.array([0.0, 1.0, -0.5, 2.0], np.float32)
    for n in range(N):
        M[n, cols] = np.roll(np.resize(special, cols.size), n)
    if nan_node0:
        M[0, cols] = np.resize(np.array([np.nan, np.inf, 0.0, 1.0], np.float32), cols.size)
        nb = np.setdiff1d(np.arange(C), cols)
        if nb.size:
            M[0, nb[0]] = np.nan                       # a NaN stored at a non-binary column: be -> -99999, t = -0
    X = unit_rows(B, J, J + 2)
    X[:, cols] = np.resize(np.array([0.0, 1.0, 0.5, 1.0, 0.5], np.float32), (B, cols.size))
    nb = np.setdiff1d(np.arange(J), cols)
    if nb.size:
        X[3, nb[-1]] = np.nan                          # a NaN in a row, at a non-binary column (the row's distance is NaN)
    valid = rng.random((B, J)) < 0.7
    valid[5] = True
    valid[6] = False                                   # a row without a valid column
    if nb.size:
        X[7, nb[0]] = np.nan
        valid[7, nb[0]] = False                        # ... at an invalid column
    return W, H, B, M, X, binary, continuous, valid


@pytest.mark.parametrize("J", [3, 7, 9, 12, 15, 37])
@pytest.mark.parametrize("tr", TRS)
def test_engineered_terms_are_exact(tr, J):
    seen = set()
    for nan_node0 in (0, 1):
        for all_binary in (False, True):
            W, H, B, M, X, binary, continuous, valid = engineered(tr, J, nan_node0, all_binary)
            C = min(J, M.shape[1])
            ctx = vsom_amd.Context(W, H, J, tr)
            ctx.set_state(map=M)
            ctx.upload_chunk(X)
            bi, bd = ctx.bmu_batch()
            if nan_node0:
                assert (bi == 0).all() and np.isnan(bd).all()
            for v in (None, valid):
                got = ctx.evaluate(binary, continuous, valid=v)
                assert (got["bmu"] == bi).all() and beq(got["dist"], bd)
                b32, n32, exact, t32 = ref.restate32(X[:, :C], M[bi.astype(np.int64)][:, :C], binary[:C], continuous[:C],
                                                None if v is None else v[:, :C])
                assert exact.all()
                assert beq(got["bsum"], b32), (tr, J, nan_node0, all_binary, v is not None, got["bsum"][:6], b32[:6])
                assert (got["nrepl"] == n32).all()
                assert ref.same_double(got["error"], ref.running_mean(got["dist"], got["bsum"]))
                seen.add(not beq(ref.sequential(t32), b32))
                if v is None:
                    assert (n32 == np.count_nonzero(binary[:C])).all()
                    if all_binary:
                        assert (n32 == C).all()        # every column replaced: C squares of 99999 b summed in Eigen's order
                else:
                    assert got["bsum"][6] == 0 and got["nrepl"][6] == 0
            ctx.close()
    if J >= 9:                                         # (a property of these inputs, node-0 cases: a plain loop gives other bits)
        assert True in seen


def test_non_finite_column_factors_are_restated_not_skipped():
    """t = (be * 0) * inf is NaN in the reference too: a zero factor only vanishes beside a finite one"""
    W, H, J, B = 4, 4, 12, 20
    ctx, M, X = context(po.STANDARD, W, H, J, B, seed=4)
    bi, _ = ctx.bmu_batch()
    Mb = M[bi.astype(np.int64)]
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    for binary, continuous in ((np.r_[np.zeros(11), 0.0], np.r_[np.ones(11), inf]), (np.r_[inf, np.zeros(11)], np.zeros(12)),
                               (np.r_[np.zeros(5), nan, np.zeros(6)], np.ones(12)), (np.zeros(12), np.r_[np.ones(9), nan, 1, 1])):
        got = ctx.evaluate(binary, continuous)
        b32, n32, _, _ = ref.restate32(X, Mb, binary, continuous)
        assert np.isnan(b32).all() and np.isnan(got["bsum"]).all()
        assert (got["nrepl"] == n32).all() and math.isnan(got["error"])
    # an invalid column beside an infinite binary factor: val = 0, t = (be * inf) * 0 = NaN; valid and finite elsewhere
    valid = np.ones((B, J), bool)
    valid[::2, 0] = False
    binary, continuous = np.r_[inf, np.zeros(11)].astype(np.float32), np.ones(12, np.float32)
    got = ctx.evaluate(binary, continuous, valid=valid)
    b32, n32, _, _ = ref.restate32(X, Mb, binary, continuous, valid)
    assert beq(got["bsum"], b32) and (got["nrepl"] == n32).all()
    ctx.close()


# ---- 3. all-continuous -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", TRS)
def test_all_continuous_is_the_running_mean_of_the_distances(tr):
    W, H, J, B = 6, 5, 9, 50
    X = gen.blobs(B, J, 4, 3, 2)
    X = X if tr != po.CLR else (np.abs(X) + np.float32(0.5)).astype(np.float32)
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=gen.random_map(W * H, o.depth, seed=13))      # (values on both sides of 0)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=o.map)
    ctx.upload_chunk(X)
    bi, bd = ctx.bmu_batch()
    valid = np.random.default_rng(2).random((B, J)) < 0.5
    for v in (None, valid):
        got = ctx.evaluate(np.zeros(J), np.ones(J), valid=v)
        assert (got["bsum"].view(np.uint32) == 0).all() and (got["nrepl"] == 0).all()
        assert (got["bmu"] == bi).all() and beq(got["dist"], bd)
        err = 0.0
        for i in range(B):
            err += 1.0 / (i + 1.0) * (float(bd[i]) - err)
        assert got["error"] == err
    err = 0.0
    for i in range(B):                                 # ... and of the oracle's
        err += 1.0 / (i + 1.0) * (o.dist(o.find_bmu(X[i]), X[i]) - err)
    assert got["error"] == err
    ctx.close()


# ---- 4. row ranges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 9, 7, 13, 70), (po.CLR, 5, 4, 5, 41)])
def test_row_ranges_are_slices_of_the_whole_chunk(tr, W, H, J, B):
    ctx, M, X = context(tr, W, H, J, B, seed=5)
    binary, continuous = column_factors(J, 9)
    valid = np.random.default_rng(1).random((B, J)) < 0.6
    whole = ctx.evaluate(binary, continuous, valid=valid)
    for r0, r1 in ((0, 7), (B // 3, B // 3 + 17), (B - 5, B), (4, 4), (0, 0), (B, B), (9, 10), (B - 1, B), (0, B), (1, B - 1),
                   (8, 40), (33, 34)):
        part = ctx.evaluate(binary, continuous, valid=valid[r0:r1], r0=r0, r1=r1)
        for k in ROW_KEYS:
            assert part[k].shape[0] == r1 - r0
            assert beq(part[k], whole[k][r0:r1]) if k in ("dist", "bsum") else (part[k] == whole[k][r0:r1]).all(), (k, r0, r1)
        # error restarts at r0
        assert ref.same_double(part["error"], ref.running_mean(whole["dist"][r0:r1], whole["bsum"][r0:r1])), (r0, r1)
        if r0 == r1:
            assert part["error"] == 0.0
    ctx.close()


# ---- 5. search modes, state ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tr", TRS)
def test_every_search_mode_and_the_state_the_search_leaves(tr):
    W, H, J, B = (24, 20, 40, 600) if tr != po.CLR else (16, 12, 8, 300)
    ctx, M, X = context(tr, W, H, J, B, seed=5)
    binary, continuous = column_factors(J, 2)
    base = None
    for mode in (capi.BMU_AUTO, capi.BMU_EXACT, capi.BMU_SHORTLIST):
        ctx.set_bmu_mode(mode)
        bi, bd = ctx.bmu_batch()
        ctx.set_last_bmu(np.zeros(B, np.uint64))
        got = ctx.evaluate(binary, continuous)
        assert (got["bmu"] == bi).all() and beq(got["dist"], bd), mode
        assert (ctx.get_last_bmu() == bi).all() and beq(ctx.get_sqres(), bd), mode
        base = got if base is None else base
        same(got, base)
        ctx.set_last_bmu(np.zeros(B, np.uint64))
        part = ctx.evaluate(binary, continuous, r0=5, r1=9)         # the search covers the whole chunk whatever the range
        assert (part["bmu"] == bi[5:9]).all() and beq(part["dist"], bd[5:9])
        assert (ctx.get_last_bmu() == bi).all() and beq(ctx.get_sqres(), bd), mode
    ctx.close()


@pytest.mark.parametrize("tr", [po.STANDARD, po.CLR])
def test_read_only_and_an_epoch_afterwards(tr):
    W, H, J, B = 9, 8, 10, 120
    X = gen.blobs(B, J, 4, 3, 2)
    X = X if tr != po.CLR else (np.abs(X) + np.float32(0.5)).astype(np.float32)
    o = po.OracleSom(W, H, J, tr)
    o.set_state(map=gen.random_map(W * H, o.depth, seed=13))
    o.train_batch(X, [0, B], 2, 4.0, 0.3)
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=o.map, sigma=o.sigma, S=o.S, weight=o.weight, hits=o.hits)
    ctx.upload_chunk(X)
    before = ctx.get_state()
    chunk = ctx.device_ptr(capi.BUF_CHUNK)
    binary, continuous = column_factors(J, 2)
    for v in (None, np.ones((B, J))):
        ctx.evaluate(binary, continuous, valid=v)
    after = ctx.get_state()
    for k in before:
        assert beq(before[k], after[k]) if before[k].dtype == np.float32 else (before[k] == after[k]).all(), k
    assert ctx.device_ptr(capi.BUF_CHUNK) == chunk and ctx.chunk_size == B
    mse = ctx.batch_epoch(2.5, True)
    lbo = np.zeros(B, np.uint64)
    mse_o = o.batch_epoch(X, lbo, 2.5, True)
    st = ctx.get_state()
    assert (ctx.get_last_bmu() == lbo).all()
    for k, r in (("map", o.map), ("sigma", o.sigma), ("weight", o.weight)):
        assert beq(st[k], r), k
    assert (st["hits"] == o.hits).all()
    assert np.float32(mse) == np.float32(mse_o)
    ctx.close()


@pytest.mark.parametrize("tr", [po.STANDARD, po.CLR])
def test_nan_node_zero_pins_the_bmu(tr):
    ctx, M, X = context(tr, 6, 5, 7, 30)
    M[0, 1] = np.nan
    ctx.set_state(map=M)
    bi, bd = ctx.bmu_batch()
    assert (bi == 0).all()
    binary, continuous = column_factors(7, 2)
    got = ctx.evaluate(binary, continuous)
    assert (got["bmu"] == 0).all()
    assert (got["dist"].view(np.uint32) == ref.QNAN).all() and beq(got["dist"], bd)
    assert math.isnan(got["error"])
    assert np.isfinite(got["bsum"]).all()
    ctx.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    W, H, J, B = 6, 5, 7, 20
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=unit_map(W * H, J, 1))
    L = capi.lib()
    out = capi.EvaluateOut()
    bsum = np.full(B, -1, np.float32)
    error = np.full(1, -1.0, np.float64)
    out.bsum = bsum.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    out.error = error.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    binary, continuous = column_factors(J, 2)
    fp = ctypes.POINTER(ctypes.c_float)
    pb, pc = binary.ctypes.data_as(fp), continuous.ctypes.data_as(fp)

    def rc(r0, r1, b=pb, c=pc, o=out):
        return L.vsom_evaluate_batch(ctx._h, r0, r1, b, c, None, None if o is None else ctypes.byref(o))

    assert rc(0, 0) == -1                              # no chunk loaded
    assert "no chunk" in L.vsom_last_error().decode()
    ctx.upload_chunk(unit_rows(B, J, 3))
    good = ctx.evaluate(binary, continuous)
    for args in ((5, 4), (0, B + 1), (B + 1, B + 2), (0, B, None), (0, B, pb, None), (0, B, pb, pc, None)):
        assert rc(*args) == -1, args
        same(ctx.evaluate(binary, continuous), good)
    assert rc(3, 3) == 0 and error[0] == 0.0           # an empty range
    assert rc(0, B) == 0 and beq(bsum, good["bsum"]) and ref.same_double(float(error[0]), good["error"])
    assert L.vsom_evaluate_batch(ctx._h, 0, B, pb, pc, None, ctypes.byref(capi.EvaluateOut())) == 0     # no output at all
    for _ in range(3):                                 # repeated calls are deterministic
        same(ctx.evaluate(binary, continuous), good)
    ctx.close()

    # custom contexts
    depth, rlen = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=depth, residual_len=rlen)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    with pytest.raises(capi.VsomError, match="vsom_evaluate_batch"):
        cu.evaluate(np.zeros(5), np.ones(5))
    cu.bmu_batch()
    cu.close()

    # a chunk staged ahead (as tests/test_gpu_bmd_batch.py): refused until it is committed
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big = vsom_amd.Context(W, H, J)
    pin = capi.PinnedBuffer(xs[1].shape)
    pin.array[...] = xs[1]
    big.set_state(map=init)
    big.upload_chunk(xs[0])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pin.array)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.evaluate(np.zeros(J), np.ones(J))
    big.commit_chunk()
    got = big.evaluate(np.zeros(J), np.ones(J), r0=0, r1=4)
    bi, bd = big.bmu_batch()
    assert (got["bmu"] == bi[:4]).all() and beq(got["dist"], bd[:4])
    big.close()
    pin.free()


# ---- 7. Som mirror ---------------------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet with validity flags"""

    def __init__(self, X, validity):
        super().__init__(X)
        self.validity = validity


@pytest.mark.parametrize("tr, W, H, J, B", [(po.STANDARD, 6, 5, 9, 50), (po.MEDIAN, 7, 3, 12, 33), (po.CLR, 4, 4, 7, 20)])
def test_som_evaluate(tr, W, H, J, B):
    ctx, M, X = context(tr, W, H, J, B, seed=8)
    binary, continuous = column_factors(J, 4)
    valid = np.random.default_rng(5).random((B, J)) < 0.6
    plain = ctx.evaluate(binary, continuous)
    masked = ctx.evaluate(binary, continuous, valid=valid)
    dflt = ctx.evaluate(np.zeros(J), np.ones(J))
    ctx.close()
    assert not ref.same_double(plain["error"], masked["error"])
    t = {po.STANDARD: vs.Transformation.Standard(), po.MEDIAN: vs.Transformation.StandardMedianEstimator(),
         po.CLR: vs.Transformation.CombinatorialLinearRegression()}[tr]
    s = vs.Som(W, H, M.shape[1], t)
    s.setState(map=M)
    assert ref.same_double(s.evaluate(X, binary, continuous), plain["error"])
    same(s.evaluateRows(X, binary, continuous), plain)
    assert ref.same_double(s.evaluate(X, binary, continuous, valid=valid), masked["error"])
    ds = ValidDataSet(X, valid)
    ds.loadNextDataFromStream()
    assert ref.same_double(s.evaluate(ds, binary, continuous), masked["error"])      # the data set's validity
    same(s.evaluateRows(ds, binary, continuous), masked)
    assert ref.same_double(s.evaluate(X), dflt["error"])                              # binary all 0, continuous all 1
    assert s.evaluate(X[:0]) == 0.0
    s.close()


def test_zz_report():
    """the largest relative distance of bsum to its float64 restatement over every tolerance check of this run"""
    print(f"vsom_evaluate_batch: worst relative distance of bsum {WORST['rel']:.3e} = {WORST['rel'] * 2 ** 24:.2f} x 2^-24 "
          f"over {WORST['rows']} rows, at {WORST['where']}")
    if WORST["rows"]:
        assert WORST["rel"] > 0                        # (the tolerance checks compared something)
