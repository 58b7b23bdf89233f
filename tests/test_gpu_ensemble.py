"""GPU: ensembles (include/vsom_hip.h, vsom_ensemble_*) -- many contexts trained by one call, one workgroup per tiny map.
Every comparison is bitwise against twin contexts trained one by one with the single-context calls, and against the
oracle for a subset: online chunks of mixed maps (U = 1/2/4, local and full search, the LDS limits), batch epochs of the
three kinds, members that take their ordinary path in the same call, both stream layouts, the ingest sequences, more
members than the chip has CUs, and the refusals."""
import numpy as np
import pytest

import custom_hooks as hooks
import gen
import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

EXP, INV = capi.EXPONENTIAL, capi.INVERSE_PROPORTIONAL
KEYS = ("map", "S", "sigma", "weight", "hits")


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()
    return (a == b).all()


def rows(B, J, seed, nan=True):
    """blobs with a NaN row and repeated rows (duplicates of the model below)"""
    X = gen.blobs(B, J, 4, seed, seed + 1, sigma=0.3)
    if B >= 4:
        X[B // 3] = X[0]
        X[B - 1] = X[1]
        if nan:
            X[B // 2, J // 2] = np.nan
    return np.ascontiguousarray(X, dtype=np.float32)


class Pair:
    """a member and its twin: the same map, the same chunks, the same calls (the twin's one by one)"""

    def __init__(self, W, H, J, tr, B, seed, custom=None, mode=None, chunks=1):
        self.W, self.H, self.J, self.tr, self.B = W, H, J, tr, B
        D = po.length(tr, J) if custom is None else hooks.shape(custom, J)[0]
        init = gen.random_map(W * H, D, seed=seed)
        # a model row equal to a sample: a zero distance at the BMU
        self.X = []
        for c in range(chunks):
            X = gen.correlated(B, J, seed + c) if tr == po.CLR else rows(B, J, seed + 7 * c)
            self.X.append(X)
        if custom is None and tr != po.CLR:
            init[min(3, W * H - 1)] = self.X[0][2]

        def make():
            if custom is not None:
                d, r = hooks.shape(custom, J)
                ctx = capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES[custom], depth=d, residual_len=r)
            else:
                ctx = vsom_amd.Context(W, H, J, tr)
            if mode is not None:
                ctx.set_bmu_mode(mode)
            ctx.set_state(map=init)
            return ctx

        self.m, self.t = make(), make()
        self.init = init
        self.lb = [np.zeros(B, np.uint64) for _ in range(chunks)]   # lastBMU of each chunk from the previous epoch

    def load(self, c):
        for ctx in (self.m, self.t):
            ctx.upload_chunk(self.X[c])
            ctx.set_last_bmu(self.lb[c])

    def same_state(self, what):
        a, b = self.m.get_state(), self.t.get_state()
        for k in KEYS:
            assert beq(a[k], b[k]), (what, k)

    def close(self):
        self.m.close()
        self.t.close()


def online_round(ens, pairs, eta, sigma, fn, first, c, what):
    for p in pairs:
        p.load(c)
    mse, lbs = ens.train_online_chunk_fetch(eta, sigma, fn, first_chunk=first)
    for k, p in enumerate(pairs):
        mse_t, lb_t = p.t.train_online_chunk_fetch(eta[k], sigma[k], fn[k], first_chunk=first)
        assert beq(lbs[k], lb_t), (what, k, "lastBMU")
        assert beq(np.float32(mse[k]), np.float32(mse_t)), (what, k, mse[k], mse_t)
        assert beq(p.m.get_last_bmu(), lb_t) and beq(np.float32(p.m.get_mse()), np.float32(mse_t)), (what, k)
        p.same_state((what, k))
        p.lb[c] = lb_t.copy()
    return mse, lbs


def test_online_mixed_members():
    """10x10x9, 12x9x20 Median, 1x1x7, 2x1x1, 32x32x4 (B 4096), 4x2x512 Median, 32x16x8 Median (B 4095): U = 1/2/4,
    local and full search, the largest LDS; own eta / sigma / decay per member, sigma above, at and below 1; three
    chunks per epoch with the running MSE carried, two epochs; member 0 against the oracle as well"""
    specs = [(10, 10, 9, po.STANDARD, 20), (12, 9, 20, po.MEDIAN, 37), (1, 1, 7, po.STANDARD, 30), (2, 1, 1, po.STANDARD, 9),
             (32, 32, 4, po.STANDARD, 4096), (4, 2, 512, po.MEDIAN, 131), (32, 16, 8, po.MEDIAN, 4095)]
    pairs = [Pair(W, H, J, tr, B, seed=11 + i, chunks=3) for i, (W, H, J, tr, B) in enumerate(specs)]
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    n = len(pairs)
    eta = [0.02 + 0.01 * k for k in range(n)]
    fn = [EXP if k % 2 == 0 else INV for k in range(n)]
    p0 = pairs[0]
    o = po.OracleSom(p0.W, p0.H, p0.J, p0.tr)
    o.set_state(map=p0.init)
    olb = [np.zeros(p0.B, np.uint64) for _ in range(3)]
    for ep, base in enumerate((3.0, 1.0)):
        run_o = np.float32(0)
        for c in range(3):
            # sigma per member: above 1 in epoch 0; at 1 and below 1 in epoch 1
            sigma = [base + (0.5 * k if ep == 0 else -0.15 * (k % 3)) for k in range(n)]
            first = c == 0
            mse, lbs = online_round(ens, pairs, eta, sigma, fn, first, c, (ep, c))
            lb = olb[c] if sigma[0] <= 1 else np.zeros(p0.B, np.uint64)
            run_o = o.train_online_chunk(p0.X[c], lb, eta[0], sigma[0], fn[0], mse_start=0.0 if first else float(run_o))
            olb[c] = lb
            assert beq(lbs[0], lb) and beq(np.float32(mse[0]), np.float32(run_o)), (ep, c)
            st = p0.m.get_state()
            for k in KEYS:
                assert beq(st[k], getattr(o, k)), (ep, c, k)
    ens.close()
    for p in pairs:
        p.close()


def test_batch_epochs_of_the_three_kinds():
    """Standard, Median and CLR tiny maps, own sigma per member, is_first both ways; the CLR member against the oracle"""
    specs = [(10, 10, 9, po.STANDARD, 20), (8, 8, 12, po.MEDIAN, 50), (6, 6, 5, po.CLR, 40), (5, 7, 3, po.STANDARD, 256),
             (16, 16, 16, po.MEDIAN, 60)]
    pairs = [Pair(W, H, J, tr, B, seed=31 + i) for i, (W, H, J, tr, B) in enumerate(specs)]
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    pc = pairs[2]
    o = po.OracleSom(pc.W, pc.H, pc.J, pc.tr)
    o.set_state(map=pc.init)
    lbo = np.zeros(pc.B, np.uint64)
    for p in pairs:
        p.load(0)
    for ep, first in enumerate((True, False, True, False)):
        sigma = [4.0 - 0.7 * ep + 0.3 * k for k in range(len(pairs))]
        mse = ens.batch_epoch(sigma, first)
        for k, p in enumerate(pairs):
            mse_t = p.t.batch_epoch(sigma[k], first)
            assert beq(np.float32(mse[k]), np.float32(mse_t)), (ep, k)
            assert beq(p.m.get_last_bmu(), p.t.get_last_bmu()), (ep, k)
            p.same_state((ep, k))
        mse_o = o.batch_epoch(pc.X[0], lbo, sigma[2], first)
        assert beq(np.float32(mse[2]), np.float32(mse_o)) and beq(pc.m.get_last_bmu(), lbo), ep
        st = pc.m.get_state()
        for k in ("map", "sigma", "weight"):
            assert beq(st[k], getattr(o, k)), (ep, k)
    ens.close()
    for p in pairs:
        p.close()


def _fallback_pairs():
    return [Pair(10, 10, 9, po.STANDARD, 20, seed=51),
            Pair(64, 64, 64, po.STANDARD, 64, seed=52),                      # above the tiny limits
            Pair(7, 7, 6, po.CLR, 40, seed=53),                              # CLR: no one-launch online chunk
            Pair(10, 10, 9, po.STANDARD, 20, seed=54, custom="standard"),   # custom transformation
            Pair(10, 10, 9, po.STANDARD, 20, seed=55, mode=capi.BMU_EXACT),  # a non-AUTO search mode
            Pair(12, 9, 20, po.MEDIAN, 37, seed=56)]


def test_members_on_their_ordinary_path_in_the_same_call():
    pairs = _fallback_pairs()
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    n = len(pairs)
    fn = [EXP, INV, EXP, INV, EXP, INV]
    for ep, (sigma0, first) in enumerate(((2.5, True), (1.0, True), (float("nan"), False))):
        sigma = [sigma0 + 0.25 * k for k in range(n)]
        if ep == 2:
            sigma = [float("nan") if k == 0 else 2.0 for k in range(n)]    # sigma = NaN: the ordinary path
        online_round(ens, pairs, [0.05] * n, sigma, fn, first, 0, ep)
    for ep, first in enumerate((True, False)):
        sigma = [3.0 + 0.5 * k for k in range(n)]
        mse = ens.batch_epoch(sigma, first)
        for k, p in enumerate(pairs):
            assert beq(np.float32(mse[k]), np.float32(p.t.batch_epoch(sigma[k], first))), ("batch", ep, k)
            p.same_state(("batch", ep, k))
    ens.close()
    for p in pairs:
        p.close()


def _layout_run(shared, ingest):
    """the same ensemble, members on one stream or each on its own; ingest: the chunk arrives through prefetch / commit,
    and a batch epoch + online chunk are followed by a stage-ahead of the next chunk (the ADVICE.md sequence)"""
    import torch
    specs = [(10, 10, 9, po.STANDARD, 20), (12, 9, 20, po.MEDIAN, 37), (8, 8, 12, po.STANDARD, 50), (32, 32, 4, po.STANDARD, 500)]
    pairs = [Pair(W, H, J, tr, B, seed=71 + i, chunks=2) for i, (W, H, J, tr, B) in enumerate(specs)]
    stream = torch.cuda.Stream(device=torch.device("cuda", 0)) if shared else None
    if shared:
        for p in pairs:
            p.m.set_stream(stream.cuda_stream)
    ens = vsom_amd.Ensemble([p.m for p in pairs])
    n = len(pairs)
    out = []
    for c in (0, 1):
        if ingest:
            for p in pairs:
                p.m.prefetch_chunk(p.X[c])
                p.m.commit_chunk()
                p.m.set_last_bmu(p.lb[c])
                p.t.prefetch_chunk(p.X[c])
                p.t.commit_chunk()
                p.t.set_last_bmu(p.lb[c])
        else:
            for p in pairs:
                p.load(c)
        sigma = [2.0 + 0.3 * k for k in range(n)]
        mse = ens.batch_epoch(sigma, True)
        for k, p in enumerate(pairs):
            assert beq(np.float32(mse[k]), np.float32(p.t.batch_epoch(sigma[k], True))), (c, k)
            p.same_state((c, k, "batch"))
        for p in pairs:
            p.lb[c] = p.t.get_last_bmu().copy()
            p.m.set_last_bmu(p.lb[c])
        mse, lbs = ens.train_online_chunk_fetch([0.03] * n, [1.5] * n, [EXP] * n, first_chunk=True)
        for k, p in enumerate(pairs):
            p.t.set_last_bmu(p.lb[c])
            mse_t, lb_t = p.t.train_online_chunk_fetch(0.03, 1.5, EXP, first_chunk=True)
            assert beq(lbs[k], lb_t) and beq(np.float32(mse[k]), np.float32(mse_t)), (c, k)
            p.same_state((c, k, "online"))
        if ingest and c == 0:        # the next chunk staged ahead right behind the launch, then adopted
            for p in pairs:
                p.m.prefetch_chunk(p.X[1])
                p.t.prefetch_chunk(p.X[1])
        out.append([p.m.get_state() for p in pairs])
    ens.close()
    for p in pairs:
        p.close()
    if stream is not None:
        stream.synchronize()
    return out


def test_stream_layouts_and_ingest_give_identical_results():
    runs = [_layout_run(shared, ingest) for shared in (True, False) for ingest in (False, True)]
    for r in runs[1:]:
        for c in range(2):
            for k in range(len(r[c])):
                for key in KEYS:
                    assert beq(r[c][k][key], runs[0][c][k][key]), (c, k, key)


def test_more_members_than_compute_units():
    """600 members of 10x10x9, each with its own seed and eta; one twin replays each member's calls"""
    K, W, H, J, B = 600, 10, 10, 9, 20
    rng = np.random.default_rng(5)
    inits = [gen.random_map(W * H, J, seed=1000 + k) for k in range(K)]
    Xs = [rows(B, J, 2000 + 3 * k, nan=(k % 7 == 0)) for k in range(K)]
    eta = [float(e) for e in rng.uniform(0.01, 0.2, K)]
    members = []
    for k in range(K):
        c = vsom_amd.Context(W, H, J)
        c.set_state(map=inits[k])
        c.upload_chunk(Xs[k])
        members.append(c)
    start = [c.get_state() for c in members]
    ens = vsom_amd.Ensemble(members)
    calls = [("online", 3.0, EXP, True), ("online", 2.0, INV, False), ("batch", 2.5, True), ("online", 1.0, EXP, True)]
    res = []
    for call in calls:
        if call[0] == "online":
            res.append(ens.train_online_chunk_fetch(eta, call[1], call[2], first_chunk=call[3]))
        else:
            res.append((ens.batch_epoch(call[1], call[2]), None))
    twin = vsom_amd.Context(W, H, J)
    for k in range(K):
        twin.set_state(**start[k])
        twin.upload_chunk(Xs[k])
        twin.set_last_bmu(np.zeros(B, np.uint64))
        for call, (mse, lbs) in zip(calls, res):
            if call[0] == "online":
                mse_t, lb_t = twin.train_online_chunk_fetch(eta[k], call[1], call[2], first_chunk=call[3])
                assert beq(lbs[k], lb_t), (k, call)
            else:
                mse_t = twin.batch_epoch(call[1], call[2])
            assert beq(np.float32(mse[k]), np.float32(mse_t)), (k, call)
        a, b = members[k].get_state(), twin.get_state()
        for key in KEYS:
            assert beq(a[key], b[key]), (k, key)
    twin.close()
    ens.close()
    for c in members:
        c.close()


def test_refusals_name_the_member_and_change_nothing():
    a, c = Pair(10, 10, 9, po.STANDARD, 20, seed=91), Pair(12, 9, 20, po.MEDIAN, 37, seed=92)
    with pytest.raises(capi.VsomError, match="member 2: the same context"):
        vsom_amd.Ensemble([a.m, c.m, a.m])
    g = vsom_amd.Group(10, 10, 9, po.STANDARD, ndev=1)
    with pytest.raises(capi.VsomError, match="member 1: a member of a vsom_group"):
        vsom_amd.Ensemble([a.m, g.member(0)])
    g.close()

    # member 1: a map whose batch epoch frees the staged rows early, so that a prefetch stages the next chunk ahead over
    # them (as tests/test_gpu_ingest.py); its twin runs the same calls
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big, big_t = vsom_amd.Context(W, H, J), vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    for ctx in (big, big_t):
        ctx.set_state(map=init)
        ctx.upload_chunk(xs[0])
    a.load(0)                            # c has no chunk
    ens = vsom_amd.Ensemble([a.m, big, c.m])
    before = [p.m.get_state() for p in (a, c)]
    with pytest.raises(capi.VsomError, match="member 2: no chunk loaded"):
        ens.train_online_chunk_fetch(0.05, 2.0, EXP)
    with pytest.raises(capi.VsomError, match="member 2: no chunk loaded"):
        ens.batch_epoch(2.0, True)
    c.load(0)
    with pytest.raises(capi.VsomError, match="member 1: online training needs"):
        ens.train_online_chunk_fetch(0.05, 2.0, [EXP, capi.BATCHMAP, EXP])
    for ctx in (big, big_t):
        ctx.batch_epoch_async(10.0, True)
        ctx.prefetch_chunk(pb.array)     # staged beside the chains of chunk 0
    with pytest.raises(capi.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.train_online_chunk_fetch(0.05, 2.0, EXP)
    with pytest.raises(capi.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.batch_epoch(2.0, True)
    for p, st in zip((a, c), before):
        now = p.m.get_state()
        for k in KEYS:
            assert beq(now[k], st[k]), k
    # the next call on the same ensemble trains every member
    for ctx in (big, big_t):
        ctx.commit_chunk()
    a.load(0)
    c.load(0)
    mse, lbs = ens.train_online_chunk_fetch([0.05, 0.1, 0.05], [2.0, 3.0, 2.0], EXP, first_chunk=True)
    mse_t, lb_t = big_t.train_online_chunk_fetch(0.1, 3.0, EXP, first_chunk=True)
    assert beq(lbs[1], lb_t) and beq(np.float32(mse[1]), np.float32(mse_t))
    sa, sb = big.get_state(), big_t.get_state()
    for k in KEYS:
        assert beq(sa[k], sb[k]), k
    for k, p in ((0, a), (2, c)):
        m_t, l_t = p.t.train_online_chunk_fetch(0.05, 2.0, EXP, first_chunk=True)
        assert beq(lbs[k], l_t) and beq(np.float32(mse[k]), np.float32(m_t)), k
        p.same_state(k)
    ens.close()
    for ctx in (big, big_t, a, c):
        ctx.close()
    pb.free()


def test_two_ensembles_do_not_undo_each_others_lds_limit():
    """the dynamic LDS limit of a *_many kernel is the function's, process-wide: an ensemble whose members need less
    (32x32x4, B 500) must not lower it below what an earlier ensemble's member needs (32x32x4, B 4096) -- E1, E2, E1"""
    p1 = Pair(32, 32, 4, po.STANDARD, 4096, seed=121)
    p2 = Pair(32, 32, 4, po.STANDARD, 500, seed=122)
    e1, e2 = vsom_amd.Ensemble([p1.m]), vsom_amd.Ensemble([p2.m])
    for what, ens, p in (("E1", e1, p1), ("E2", e2, p2), ("E1 again", e1, p1)):
        online_round(ens, [p], [0.05], [3.0], [EXP], True, 0, what)
    e1.close()
    e2.close()
    p1.close()
    p2.close()
