"""GPU: the one-launch masked online chunk of tiny maps -- vsom_train_online_chunk_masked where
vsom_online_masked_tiny_applies holds, and vsom_ensemble_train_online_chunk_masked.  Every comparison is on the bits (NaN
equals NaN; the untouched-column test compares the NaN payloads too).  Two yardsticks for every case: the Python reference
tests/online_masked_ref.py on rows poisoned at the invalid positions, and the per-sample loop of the same library, forced
with set_bmu_mode(BMU_EXACT) (the same bits by contract; the mode keeps the one-launch kernel off).

Shapes (W, H, J, B): (10,10,9,20) the fixture; (5,4,1,70) D = 1; (12,9,12,7) two values per thread; (12,9,20,7) four, a
packet tail of 4; (16,16,16,5) 4096 values, the limit; (11,11,33,70) 62 samples a block of staged rows, so the chunk crosses
a block border with the validity restaged, and a scalar tail; (32,32,3,9) 1024 nodes: thread 1023 owns a node and the post
step.  The fixture runs Standard / Median x the two decays x sigma 3.0, 1.5, 1.0, 0.3; the other shapes run the four sigmas
with kind and decay alternating, as SMALL / BIG thin the cases of tests/test_gpu_online_masked.py."""
import ctypes as C
import json
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
import gen  # noqa: E402
import online_masked_cases as oc  # noqa: E402
from online_masked_cases import ETA, beq, same  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
EXP, INV = po.EXPONENTIAL, po.INVERSE_PROPORTIONAL
FIXTURE = (10, 10, 9, 20)
OTHERS = ((5, 4, 1, 70), (12, 9, 12, 7), (12, 9, 20, 7), (16, 16, 16, 5), (11, 11, 33, 70), (32, 32, 3, 9))
CASES = [(FIXTURE, tr, fn, sigma) for tr in oc.KINDS for fn in oc.DECAYS for sigma in oc.SIGMAS] + \
        [(shape, oc.KINDS[(si + gi) % 2], oc.DECAYS[(si + gi // 2) % 2], sigma)
         for si, shape in enumerate(OTHERS) for gi, sigma in enumerate(oc.SIGMAS)]


def snapshot(ctx, mse, lb):
    st = ctx.get_state()
    return {"map": st["map"], "S": st["S"], "sigma": st["sigma"], "weight": st["weight"], "hits": st["hits"],
            "lastbmu": np.array(lb, np.uint64), "mse": np.array([mse], f32)}


def new_ctx(tr, W, H, J, M, S, exact=False, **more):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.set_state(map=M, S=S, **more)
    if exact:
        ctx.set_bmu_mode(capi.BMU_EXACT)
    return ctx


def load(ctx, X, sigma, start):
    ctx.upload_chunk(np.ascontiguousarray(X, dtype=f32))
    if sigma <= 1:
        ctx.set_last_bmu(start)


def gpu_chunk(tr, W, H, J, M, S, X, valid, start, sigma, fn, state=None, exact=False, tiny=True):
    """one masked chunk on a fresh context (valid None: vsom_train_online_chunk_fetch); exact: the per-sample loop.  tiny:
    what vsom_online_masked_tiny_applies must say of the call"""
    ctx = new_ctx(tr, W, H, J, M, S, exact, **(state or {}))
    load(ctx, X, sigma, start)
    if valid is None:
        mse, lb = ctx.train_online_chunk_fetch(ETA, sigma, fn)
    else:
        assert ctx.online_masked_tiny_applies(sigma, np.ndim(valid) == 1) == (tiny and not exact)
        mse, lb = ctx.train_online_chunk_masked(ETA, sigma, fn, valid)
        assert ctx.online_search_stats()["samples"] == 0
    assert (lb == ctx.get_last_bmu()).all() and beq(np.array([ctx.get_mse()], f32), np.array([mse], f32))
    snap = snapshot(ctx, mse, lb)
    ctx.close()
    return snap


def both(tr, W, H, J, M, S, X, valid, start, sigma, fn, want, what, state=None):
    """the one-launch chunk and the loop of the same library against `want`"""
    same(gpu_chunk(tr, W, H, J, M, S, X, valid, start, sigma, fn, state), want, (what, "one launch"))
    same(gpu_chunk(tr, W, H, J, M, S, X, valid, start, sigma, fn, state, exact=True), want, (what, "the loop"))


def ref_chunk(tr, W, H, J, M, S, X, valid, start, sigma, fn, state=None):
    r = oc.ref_new(tr, W, H, J, M, S)
    r.set_state(**(state or {}))
    lb = oc.start_of(sigma, start, X.shape[0])
    mse = r.train_chunk(X, valid, lb, ETA, sigma, fn)
    return r.snapshot(lb, mse)


# ---- 1. the predicate ------------------------------------------------------------------------------------------------------
def applies(W, H, J, B, tr=po.STANDARD, sigma=3.0, one=False, mode=None):
    ctx = vsom_amd.Context(W, H, J, tr)
    ctx.upload_chunk(gen.correlated(B, J, 1) if tr == po.CLR else gen.blobs(B, J, 2, 1, 2))
    if mode is not None:
        ctx.set_bmu_mode(mode)
    got = ctx.online_masked_tiny_applies(sigma, one)
    ctx.close()
    return got


def test_path_predicate(monkeypatch):
    for one in (False, True):
        for sigma in (3.0, 1.0):
            assert applies(10, 10, 9, 20, sigma=sigma, one=one)
            assert applies(16, 16, 16, 64, sigma=sigma, one=one)
            assert applies(10, 10, 9, 20, po.MEDIAN, sigma=sigma, one=one)
        assert not applies(16, 16, 17, 20, one=one)            # N D = 4352
        assert not applies(10, 10, 9, 4097, one=one)
        assert not applies(7, 7, 6, 20, po.CLR, one=one)
        assert not applies(10, 10, 9, 20, mode=capi.BMU_EXACT, one=one)
        assert not applies(10, 10, 9, 20, sigma=float("nan"), one=one)
    d, r = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    assert not cu.online_masked_tiny_applies(3.0)
    cu.close()
    no_chunk = vsom_amd.Context(10, 10, 9)
    assert not no_chunk.online_masked_tiny_applies(3.0)
    no_chunk.close()
    assert capi.lib().vsom_online_masked_tiny_applies(None, 3.0, 0) == 0
    monkeypatch.setenv("VSOM_NO_TINY", "1")                    # (read when a context is created)
    assert not applies(10, 10, 9, 20)


# ---- 2. random masks, NaN / inf at the invalid positions -------------------------------------------------------------------
@pytest.mark.parametrize("shape, tr, fn, sigma", CASES)
def test_random_mask(shape, tr, fn, sigma):
    W, H, J, B = shape
    X, M, valid, S, start = oc.data(W, H, J, B)
    want = oc.reference(tr, W, H, J, B, fn, sigma)
    both(tr, W, H, J, M, S, oc.poisoned(X, valid), valid, start, sigma, fn, want, "poisoned rows")


@pytest.mark.parametrize("sigma", (3.0, 1.0))
@pytest.mark.parametrize("tr", oc.KINDS)
@pytest.mark.parametrize("B", (1, 2, 3))
def test_chunk_sizes_across_the_sample_parity(B, tr, sigma):
    W, H, J = 10, 10, 9
    X, M, valid, S, start = oc.data(W, H, J, B, seed=20 + B)
    Xp = oc.poisoned(X, valid)
    want = ref_chunk(tr, W, H, J, M, S, Xp, valid, start, sigma, EXP)
    both(tr, W, H, J, M, S, Xp, valid, start, sigma, EXP, want, f"B = {B}")


# ---- 3. all-valid masks, column masks, empty rows, NaN ---------------------------------------------------------------------
@pytest.mark.parametrize("sigma", oc.SIGMAS)
@pytest.mark.parametrize("tr", oc.KINDS)
@pytest.mark.parametrize("shape", (FIXTURE, (12, 9, 20, 7)))
def test_all_valid_is_the_unmasked_chunk(shape, tr, sigma):
    W, H, J, B = shape
    X, M, valid, S, start = oc.data(W, H, J, B)
    for fn in oc.DECAYS:
        want = gpu_chunk(tr, W, H, J, M, S, X, None, start, sigma, fn)           # the unmasked one-launch chunk
        same(gpu_chunk(tr, W, H, J, M, S, X, np.ones((B, J), np.uint8), start, sigma, fn), want, "per-row mask")
        same(gpu_chunk(tr, W, H, J, M, S, X, np.ones(J, np.uint8), start, sigma, fn), want, "one_mask")


@pytest.mark.parametrize("sigma", (3.0, 1.0))
@pytest.mark.parametrize("tr", oc.KINDS)
def test_column_mask(tr, sigma):
    W, H, J, B = 12, 9, 20, 7
    X, M, _, S, start = oc.data(W, H, J, B)
    cols = np.ones(J, np.uint8)
    cols[[0, 5, 8, 16, J - 1]] = 0       # in the packet blocks, the packet tail's last element
    Xp = oc.poisoned(X, cols != 0)
    for fn in oc.DECAYS:
        want = ref_chunk(tr, W, H, J, M, S, Xp, cols, start, sigma, fn)
        both(tr, W, H, J, M, S, Xp, cols, start, sigma, fn, want, "one_mask")
        same(gpu_chunk(tr, W, H, J, M, S, Xp, np.tile(cols, (B, 1)), start, sigma, fn), want, "the same mask per row")


@pytest.mark.parametrize("sigma", (3.0, 1.0))
def test_a_row_without_a_valid_column(sigma):
    W, H, J, B = FIXTURE
    X, M, valid, S, start = oc.data(W, H, J, B)
    valid = np.array(valid)
    empty = (0, 4, B - 1)
    valid[list(empty)] = False
    Xp = oc.poisoned(X, valid)
    for fn in oc.DECAYS:
        want = ref_chunk(po.STANDARD, W, H, J, M, S, Xp, valid, start, sigma, fn)
        both(po.STANDARD, W, H, J, M, S, Xp, valid, start, sigma, fn, want, "empty rows")
        for j in empty:                  # every distance is +0: node 0, or the walk stays where it starts
            assert want["lastbmu"][j] == (0 if sigma > 1 else start[j])
    # a chunk of empty rows only: map, SMap and sigmaMap keep their bits, the MSE is 0; only weightMap and bmuHits move
    none = np.zeros((B, J), np.uint8)
    got = gpu_chunk(po.STANDARD, W, H, J, M, S, Xp, none, start, sigma, EXP)
    assert beq(got["map"], M) and beq(got["S"], S) and not got["sigma"].any() and got["mse"][0] == 0
    assert got["hits"].sum() == B and (got["weight"] != 0).any()
    same(got, gpu_chunk(po.STANDARD, W, H, J, M, S, Xp, none, start, sigma, EXP, exact=True), "empty rows only")


def test_nan_in_node_0():
    W, H, J, B = FIXTURE
    X, M, valid, S, start = oc.data(W, H, J, B)
    valid = np.array(valid)
    valid[:, 3] = True
    valid[:, 6] = False
    Xp = oc.poisoned(X, valid)
    # at a valid column: d_0 is NaN and keeps node 0 for every sample
    M1 = np.array(M)
    M1[0, 3] = np.nan
    want = ref_chunk(po.STANDARD, W, H, J, M1, S, Xp, valid, start, 3.0, EXP)
    assert not want["lastbmu"].any() and want["hits"][0] == B
    both(po.STANDARD, W, H, J, M1, S, Xp, valid, start, 3.0, EXP, want, "NaN at a valid column of node 0")
    # at an invalid column: no effect on anything but that entry, which keeps its bits
    M2 = np.array(M)
    M2[0, 6] = np.nan
    want = ref_chunk(po.STANDARD, W, H, J, M2, S, Xp, valid, start, 3.0, EXP)
    assert want["lastbmu"].any() and np.isnan(want["map"][0, 6])
    both(po.STANDARD, W, H, J, M2, S, Xp, valid, start, 3.0, EXP, want, "NaN at an invalid column of node 0")


# ---- 4. sigmaMap takes the weight of the value's last VALID step -----------------------------------------------------------
@pytest.mark.parametrize("fn", oc.DECAYS)
@pytest.mark.parametrize("tr", oc.KINDS)
def test_sigma_map_takes_the_weight_of_the_last_valid_step(tr, fn):
    """sample 0 steps column d of the nodes of its window; sample 1, with d invalid, visits most of them again: their weight
    moves, sigmaMap[., d] does not.  sqrt(|S / final weight|), the plain chunk's write-back, differs there in the bits."""
    W, H, J, B, d = 10, 10, 9, 2, 4
    X, M, _, S, start = oc.data(W, H, J, B, seed=77)
    valid = np.ones((B, J), bool)
    valid[1, d] = False
    Xp = oc.poisoned(X, valid)
    want = ref_chunk(tr, W, H, J, M, S, Xp, valid, start, 3.0, fn)
    after0 = ref_chunk(tr, W, H, J, M, S, Xp[:1], valid[:1], start[:1], 3.0, fn)
    twice = (after0["weight"].reshape(-1) != 0) & (want["weight"].reshape(-1) != after0["weight"].reshape(-1))
    assert twice.sum() >= 4                                    # nodes of both windows
    with np.errstate(all="ignore"):
        final = np.sqrt(np.abs(want["S"][:, d] / want["weight"].reshape(-1).astype(f32))).astype(f32)
    wrong = twice & (final.view(np.uint32) != want["sigma"][:, d].view(np.uint32))
    assert wrong.any()                                         # the final-weight rule fails this case
    assert beq(want["sigma"][twice, d], after0["sigma"][twice, d])
    got = gpu_chunk(tr, W, H, J, M, S, Xp, valid, start, 3.0, fn)
    assert beq(got["sigma"][wrong, d], want["sigma"][wrong, d])
    same(got, want, "one launch")
    same(gpu_chunk(tr, W, H, J, M, S, Xp, valid, start, 3.0, fn, exact=True), want, "the loop")


# ---- 5. a column valid in no row keeps its bits ----------------------------------------------------------------------------
def nan_payloads(shape, base):
    """distinct quiet-NaN payloads, one per element"""
    n = int(np.prod(shape))
    return (np.uint32(0x7FC00000) + np.uint32(base) + np.arange(n, dtype=np.uint32)).view(f32).reshape(shape)


@pytest.mark.parametrize("sigma", (3.0, 1.0))
@pytest.mark.parametrize("tr", oc.KINDS)
def test_a_column_valid_in_no_row_keeps_its_bits(tr, sigma):
    W, H, J, B = FIXTURE
    X, M, valid, S, start = oc.data(W, H, J, B)
    valid = np.array(valid)
    dead = (2, J - 1)                    # a packet-block column and the scalar tail
    valid[:, dead] = False
    M2, S2, G2 = np.array(M), np.array(S), np.zeros_like(M)
    for i, d in enumerate(dead):
        M2[:, d] = nan_payloads(W * H, 0x1000 * (3 * i + 1))
        S2[:, d] = nan_payloads(W * H, 0x1000 * (3 * i + 2))
        G2[:, d] = nan_payloads(W * H, 0x1000 * (3 * i + 3))
    Xp = oc.poisoned(X, valid)
    for fn in oc.DECAYS:
        got = gpu_chunk(tr, W, H, J, M2, S2, Xp, valid, start, sigma, fn, state={"sigma": G2})
        for k, before in (("map", M2), ("S", S2), ("sigma", G2)):
            for d in dead:
                assert (got[k][:, d].view(np.uint32) == before[:, d].view(np.uint32)).all(), (k, d)
        same(got, ref_chunk(tr, W, H, J, M2, S2, Xp, valid, start, sigma, fn, state={"sigma": G2}), "beside the dead columns")


# ---- 6. chunks in sequence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", (3.0, 1.0))
def test_two_chunks_continue_the_running_mse(sigma):
    W, H, J, B = 12, 9, 20, 7
    X, M, valid, S, start = oc.data(W, H, J, B)
    X2, _, valid2, _, start2 = oc.data(W, H, J, 5, seed=31)
    ctx = new_ctx(po.MEDIAN, W, H, J, M, S)
    r = oc.ref_new(po.MEDIAN, W, H, J, M, S)
    mse_r = f32(0)
    for first, (Xc, vc, sc) in zip((True, False), ((X, valid, start), (X2, valid2, start2))):
        Xp = oc.poisoned(Xc, vc)
        load(ctx, Xp, sigma, sc)
        assert ctx.online_masked_tiny_applies(sigma)
        mse, lb = ctx.train_online_chunk_masked(ETA, sigma, INV, vc, first_chunk=first)
        lbr = oc.start_of(sigma, sc, Xc.shape[0])
        mse_r = r.train_chunk(Xp, vc, lbr, ETA, sigma, INV, mse_start=mse_r)
        same(snapshot(ctx, mse, lb), r.snapshot(lbr, mse_r), f"chunk first={first}")
        assert ctx.get_mse() == mse
    ctx.close()


@pytest.mark.parametrize("B", (11, 4))           # odd and even: the chunk ends on either key parity
def test_masked_unmasked_masked(B):
    """a masked one-launch chunk, an unmasked one-launch chunk, a masked one: the same sequence on the loop"""
    W, H, J = 10, 10, 9
    X, M, valid, S, start = oc.data(W, H, J, B, seed=40 + B)
    Xp = oc.poisoned(X, valid)
    Xz = np.where(valid, X, f32(0))
    tiny, loop = new_ctx(po.STANDARD, W, H, J, M, S), new_ctx(po.STANDARD, W, H, J, M, S, exact=True)
    for step, (rows, mask, sigma) in enumerate(((Xp, valid, 3.0), (Xz, None, 1.5), (Xp, valid, 1.0))):
        snaps = []
        for ctx in (tiny, loop):
            ctx.upload_chunk(rows)
            if mask is None:
                mse, lb = ctx.train_online_chunk_fetch(ETA, sigma, EXP, first_chunk=step == 0)
            else:
                mse, lb = ctx.train_online_chunk_masked(ETA, sigma, EXP, mask, first_chunk=step == 0)
            snaps.append(snapshot(ctx, mse, lb))
        same(snaps[0], snaps[1], f"step {step}")
    tiny.close()
    loop.close()


# ---- 7. Som.trainBasicSomMasked --------------------------------------------------------------------------------------------
class ValidDataSet(vs.ArrayDataSet):
    """an ArrayDataSet whose loaded rows carry validity flags"""

    def __init__(self, X, validity, maxLoadCount):
        super().__init__(X, maxLoadCount)
        self._validity = validity
        self.validity = validity[0:0]

    def loadNextDataFromStream(self):
        start = self._pos
        super().loadNextDataFromStream()
        self.validity = self._validity[start:start + self.data.shape[0]]


@pytest.mark.parametrize("fn", oc.DECAYS)
def test_train_basic_som_masked_equals_the_schedule_on_the_loop(fn):
    W, H, J = 10, 10, 9
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    X = np.array(fx["rows"], f32)
    rows = X.shape[0]
    chunk = (rows + 1) // 2                      # two chunks per epoch
    rng = np.random.default_rng(8)
    valid = rng.random(X.shape) < 0.7
    Xp = oc.poisoned(X, valid)
    M = rng.random((W * H, J), dtype=f32)
    epochs, eta0, eta_decay, sigma0, sigma_decay = 5, 0.5, 0.1, 3.0, 0.4      # sigma 3, 2.01, 1.35, then the clamp at 1.0
    s = vs.Som(W, H, J)
    s._verbose = False
    s.setState(map=M)
    ds = ValidDataSet(Xp, valid, chunk)
    s.trainBasicSomMasked(ds, epochs, eta0, eta_decay, sigma0, sigma_decay, fn)
    got = s.state()
    metrics = np.array(s.metrics.MeanSquaredError[:epochs], f32)
    s.close()

    loop = new_ctx(po.STANDARD, W, H, J, M, np.zeros_like(M), exact=True)
    want_metrics = []
    for e in range(epochs):
        eta = eta0 * math.exp(-eta_decay * float(e))
        sigma = max(sigma0 * math.exp(-sigma_decay * float(e)), 1.0)
        for r0 in range(0, rows, chunk):
            loop.upload_chunk(Xp[r0:r0 + chunk])
            assert not loop.online_masked_tiny_applies(sigma)
            mse, lb = loop.train_online_chunk_masked(eta, sigma, fn, valid[r0:r0 + chunk], first_chunk=r0 == 0)
        want_metrics.append(f32(mse / f32(2)))
    st = loop.get_state()
    loop.close()
    for k in ("map", "sigma", "weight", "hits"):
        assert beq(got[k], st[k]), k
    assert beq(metrics, np.array(want_metrics, f32))
    assert (ds.lastBMU == lb).all()


# ---- 8. ensembles ----------------------------------------------------------------------------------------------------------
class Member:
    """a member context m and its twin t, which is no member"""

    def __init__(self, W, H, J, tr, B, seed, masked, one=False):
        self.W, self.H, self.J, self.tr, self.B = W, H, J, tr, B
        self.X = gen.correlated(B, J, seed) if tr == po.CLR else gen.blobs(B, J, 4, seed, seed + 1)
        init = gen.random_map(W * H, po.length(tr, J), seed=seed + 3)
        self.m, self.t = vsom_amd.Context(W, H, J, tr), vsom_amd.Context(W, H, J, tr)
        for c in (self.m, self.t):
            c.set_state(map=init)
        self.valid = None
        rng = np.random.default_rng(seed + 50)
        self.start = rng.integers(0, W * H, B).astype(np.uint64)
        if masked:
            self.valid = (rng.random(J if one else (B, J)) < 0.7).astype(np.uint8)
            self.Xp = oc.poisoned(self.X, np.broadcast_to(self.valid, self.X.shape) != 0)
        else:
            self.Xp = self.X

    def load(self):
        for c in (self.m, self.t):
            c.upload_chunk(self.Xp)
            c.set_last_bmu(self.start)

    def single(self, eta, sigma, fn, first):
        if self.valid is None:
            return self.t.train_online_chunk_fetch(eta, sigma, fn, first_chunk=first)
        return self.t.train_online_chunk_masked(eta, sigma, fn, self.valid, first_chunk=first)

    def state(self, ctx):
        st = ctx.get_state()
        st["lastbmu"] = ctx.get_last_bmu()
        st["mse"] = np.array([ctx.get_mse()], f32)
        return st

    def check(self, what):
        a, b = self.state(self.m), self.state(self.t)
        for k in b:
            assert beq(a[k], b[k]), (what, k)

    def close(self):
        self.m.close()
        self.t.close()


def six_members():
    return [Member(10, 10, 9, po.STANDARD, 20, 61, True),               # masked, one launch, sigma > 1
            Member(12, 9, 12, po.MEDIAN, 7, 62, True),                  # masked, one launch, sigma <= 1, two values per thread
            Member(10, 10, 9, po.STANDARD, 20, 63, True, one=True),     # one_mask
            Member(16, 16, 33, po.STANDARD, 9, 64, True),               # masked, off the fast path
            Member(6, 5, 7, po.STANDARD, 30, 65, False),                # plain, one launch
            Member(7, 7, 6, po.CLR, 30, 66, False)]                     # plain CLR
SIGMA6 = [3.0, 1.0, 2.5, 3.0, 1.5, 3.0]
FN6 = [EXP, INV, INV, EXP, EXP, INV]
ETA6 = [0.3, 0.25, 0.2, 0.3, 0.35, 0.3]

_STREAM = []


def shared_stream():
    """one stream for the members of an ensemble, alive for the whole module (contexts keep the handle)"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream(device=torch.device("cuda", 0)))
    return _STREAM[0]


@pytest.mark.parametrize("shared", [False, True])
def test_ensemble_of_masked_and_plain_members(shared):
    members = six_members()
    n = len(members)
    stream = shared_stream() if shared else None
    if shared:
        for mb in members:
            mb.m.set_stream(stream.cuda_stream)
    ens = vsom_amd.Ensemble([mb.m for mb in members])
    valids = [mb.valid for mb in members]
    for mb in members:
        mb.load()
    assert [mb.m.online_masked_tiny_applies(SIGMA6[k], mb.valid is not None and mb.valid.ndim == 1)
            for k, mb in enumerate(members)] == [True, True, True, False, True, False]
    # two successive chunks of one epoch, results through lastbmu_out / mse_out
    for first in (True, False):
        mse, lbs = ens.train_online_chunk_masked(ETA6, SIGMA6, FN6, valids, first_chunk=first)
        assert mse.shape == (n,) and mse.dtype == np.float32
        for k, mb in enumerate(members):
            mse_t, lb_t = mb.single(ETA6[k], SIGMA6[k], FN6[k], first)
            assert beq(mse[k], mse_t) and (lbs[k] == lb_t).all(), ("results", first, k)
            mb.check(("chunk", first, k))
    # NULL lastbmu_out entries and a NULL mse_out: the members' own words hold the results
    keep, vptrs, ones = ens._validities(valids)
    lb0 = np.zeros(members[0].B, np.uint64)
    u64p = C.POINTER(C.c_uint64)
    ptrs = (u64p * n)(*([lb0.ctypes.data_as(u64p)] + [u64p()] * (n - 1)))
    capi.check(capi.lib().vsom_ensemble_train_online_chunk_masked(
        ens._h, (C.c_double * n)(*ETA6), (C.c_double * n)(*SIGMA6), (C.c_int * n)(*FN6), 1, vptrs, ones, ptrs, None))
    for k, mb in enumerate(members):
        mb.single(ETA6[k], SIGMA6[k], FN6[k], True)
        mb.check(("NULL entries", k))
    assert (lb0 == members[0].t.get_last_bmu()).all()
    capi.check(capi.lib().vsom_ensemble_train_online_chunk_masked(
        ens._h, (C.c_double * n)(*ETA6), (C.c_double * n)(*SIGMA6), (C.c_int * n)(*FN6), 0, vptrs, ones, None, None))
    for k, mb in enumerate(members):
        mb.single(ETA6[k], SIGMA6[k], FN6[k], False)
        mb.check(("no lastbmu_out", k))
    del keep
    ens.close()
    if stream is not None:
        stream.synchronize()
    for mb in members:
        mb.close()


def test_ensemble_refusals_leave_every_member_untouched():
    L = capi.lib()
    a = Member(10, 10, 9, po.STANDARD, 20, 71, True)
    b = Member(6, 5, 7, po.STANDARD, 30, 72, False)
    clr = Member(7, 7, 6, po.CLR, 30, 73, False)
    for mb in (a, b, clr):
        mb.load()
    d, r = hooks.shape("standard", 5)
    cu = capi.Context(4, 4, 5, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    cu.upload_chunk(gen.blobs(10, 5, 2, 1, 2))
    empty = vsom_amd.Context(10, 10, 9)
    vc, vu = np.ones((30, 6), np.uint8), np.ones((10, 5), np.uint8)

    def untouched(before, what):
        for k, (mb, snap) in enumerate(zip((a, b, clr), before)):
            now = mb.state(mb.m)
            for key in snap:
                assert beq(now[key], snap[key]), (what, k, key)

    before = [mb.state(mb.m) for mb in (a, b, clr)]
    for third, v3, fn3, word in ((clr.m, vc, EXP, "member 2: .*CLR"), (cu, vu, EXP, "member 2: .*custom"),
                                 (empty, a.valid[:0], EXP, "member 2: no chunk loaded"),
                                 (clr.m, None, po.BATCHMAP, "member 2: .*Exponential or InverseProportional")):
        ens = vsom_amd.Ensemble([a.m, b.m, third])
        with pytest.raises(capi.VsomError, match=word):
            ens.train_online_chunk_masked(0.3, 3.0, [EXP, EXP, fn3], [a.valid, None, v3])
        untouched(before, word)
        ens.close()
    ens = vsom_amd.Ensemble([a.m, b.m, clr.m])
    one = (C.c_double * 3)(3.0, 3.0, 3.0)
    fns = (C.c_int * 3)(EXP, EXP, EXP)
    assert L.vsom_ensemble_train_online_chunk_masked(ens._h, one, one, fns, 1, None, None, None, None) == -1
    assert "valid_host" in L.vsom_last_error().decode()
    keep, vptrs, ones = ens._validities([a.valid, None, None])
    assert L.vsom_ensemble_train_online_chunk_masked(None, one, one, fns, 1, vptrs, ones, None, None) == -1
    assert "null ensemble" in L.vsom_last_error().decode()
    assert L.vsom_ensemble_train_online_chunk_masked(ens._h, None, one, fns, 1, vptrs, ones, None, None) == -1
    assert "null parameter array" in L.vsom_last_error().decode()
    untouched(before, "after the refusals")
    # the next legal call gives the single calls' results
    mse, lbs = ens.train_online_chunk_masked(0.3, 3.0, EXP, [a.valid, None, None])
    for k, mb in enumerate((a, b, clr)):
        mse_t, lb_t = mb.single(0.3, 3.0, EXP, True)
        assert beq(mse[k], mse_t) and (lbs[k] == lb_t).all(), k
        mb.check(("after the refusals", k))
    del keep
    ens.close()
    cu.bmu_batch()
    cu.close()
    empty.close()
    for mb in (a, b, clr):
        mb.close()
