"""GPU: vsom_batch_schedule / vsom_ensemble_batch_schedule -- a whole batch schedule in one call.
Every comparison is on the bits (NaN equals NaN) against a twin context driven by the sequence the call stands for
(tests/schedule_ref.py: lastBMU := 0 between epochs when reset_bmu, one vsom_batch_epoch per sigma); with reset_bmu = 1
also against the CPU oracle (OracleSom.train_batch for schedules given as sigma0 / decay, the restated loop for explicit
sigma arrays).  Compared: map, sigmaMap, SMap, weightMap, bmuHits, lastBMU, sqres, every epoch's MSE, vsom_get_mse.

Shapes are the smallest that reach each branch of the one-launch kernels and of the call around them: the reference's
10x10x9 fixture (33 of 40 epochs), W != H both ways, Median, CLR; B = 1, 3 and 256; the three bounds of the one-launch
path (B * N = 16384, chains = 4096 with chains * B = 262144, rows that do not fit LDS); NaN / inf values; sigma at and
below 1; a 0/0 neighbourhood; the launch split above VSOM_SCHEDULE_MAX_EPOCHS; every fallback; the calls that follow;
ensembles of mixed kinds, lengths, paths and stream layouts; the refusals."""
import json
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
import schedule_ref as sref  # noqa: E402
from schedule_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("map", "sigma", "S", "weight", "hits")
MAXE = capi.SCHEDULE_MAX_EPOCHS


def fixture_rows():
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "ican_fixture.json")))
    return np.array(fx["rows"], np.float32)


def rows_for(tr, B, J, seed):
    return gen.correlated(B, J, seed) if tr == po.CLR else gen.blobs(B, J, 4, seed, seed + 1, sigma=0.3)


def make_pair(W, H, J, tr, init, custom=None):
    def make():
        if custom is not None:
            d, r = hooks.shape(custom, J)
            ctx = capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES[custom], depth=d, residual_len=r)
        else:
            ctx = vsom_amd.Context(W, H, J, tr)
        ctx.set_state(map=init)
        return ctx
    return make(), make()


def same(m, t, mse, mse_t, what):
    """the scheduled context m against its twin t, and the per-epoch MSEs"""
    print(what, "mse[:3]", mse[:3], "twin", mse_t[:3], "epochs", len(mse))
    assert beq(mse, mse_t), (what, "per-epoch MSE")
    a, b = m.get_state(), t.get_state()
    for k in KEYS:
        assert beq(a[k], b[k]), (what, k)
    assert beq(m.get_last_bmu(), t.get_last_bmu()), (what, "lastBMU")
    assert beq(m.get_sqres(), t.get_sqres()), (what, "sqres")
    assert beq(np.float32(m.get_mse()), np.float32(t.get_mse())), (what, "vsom_get_mse")
    if len(mse):
        assert beq(np.float32(m.get_mse()), mse[-1]), (what, "vsom_get_mse is the last epoch's")


def run(W, H, J, tr, X, init, sigmas, reset, what, sched=None, custom=None, oracle=True, keep=False):
    """one schedule call against the twin loop (and the oracle when reset); sched = (epochs, sigma0, decay) when the
    sigmas come from batch_sigma_schedule"""
    m, t = make_pair(W, H, J, tr, init, custom)
    m.upload_chunk(X)
    t.upload_chunk(X)
    mse = m.batch_schedule(sigmas, reset_bmu=reset)
    mse_t = sref.twin_loop(t, sigmas, reset_bmu=reset)
    assert mse.dtype == np.float32 and mse.shape == (len(sigmas),)
    same(m, t, mse, mse_t, what)
    if reset and oracle and custom is None:
        o = po.OracleSom(W, H, J, tr)
        o.set_state(map=init)
        if sched is not None:
            done, mse_o = o.train_batch(X, [0, X.shape[0]], *sched)
            assert done == len(sigmas)
            mse_o = mse_o[:done]
        else:
            mse_o, lb_o = sref.oracle_loop(o, X, sigmas, reset_bmu=True)
            assert beq(m.get_last_bmu(), lb_o), (what, "lastBMU against the oracle")
        assert beq(mse, mse_o), (what, "MSE against the oracle")
        st = m.get_state()
        for k in ("map", "sigma", "weight", "hits"):
            assert beq(st[k], getattr(o, k)), (what, k, "against the oracle")
    if keep:
        return m, t
    m.close()
    t.close()


def sched(epochs, sigma0, decay):
    return vs.batch_sigma_schedule(epochs, sigma0, decay), (epochs, sigma0, decay)


# ---- fixture and kinds -----------------------------------------------------------------------------------------------
KIND_CASES = {
    "fixture_10x10x9": (10, 10, 9, po.STANDARD, 20, (40, 5.0, 0.05)),
    "std_9x7": (9, 7, 13, po.STANDARD, 70, (8, 4.0, 0.2)),
    "std_7x11": (7, 11, 9, po.STANDARD, 36, (8, 4.0, 0.2)),
    "median_5x11": (5, 11, 10, po.MEDIAN, 60, (10, 3.0, 0.15)),
    "clr_5x4_J6": (5, 4, 6, po.CLR, 40, (8, 2.5, 0.2)),
}


@pytest.mark.parametrize("reset", [1, 0])
@pytest.mark.parametrize("name", sorted(KIND_CASES))
def test_fixture_and_kinds(name, reset):
    W, H, J, tr, B, sc = KIND_CASES[name]
    X = fixture_rows() if name.startswith("fixture") else rows_for(tr, B, J, 5)
    init = gen.random_map(W * H, po.length(tr, J), seed=42)
    sigmas, sc = sched(*sc)
    if name.startswith("fixture"):
        assert len(sigmas) == 33
    assert len(sigmas) >= 5
    run(W, H, J, tr, X, init, sigmas, reset, (name, reset), sched=sc)


# ---- chunk sizes and the bounds of the one-launch path ---------------------------------------------------------------
SIZE_CASES = {
    "B1": (6, 5, 7, po.STANDARD, 1),
    "B3": (6, 5, 7, po.MEDIAN, 3),
    "B256_the_tiny_bound": (5, 7, 3, po.STANDARD, 256),
    "BN_16384": (8, 8, 16, po.STANDARD, 256),              # B * N = 16384
    "chains_4096": (16, 16, 16, po.STANDARD, 64),          # chains = 4096, chains * B = 262144
    "rows_beyond_lds": (4, 4, 64, po.STANDARD, 256),       # 16384 staged values > 10240: stage_x = 0
    "clr_B256": (4, 3, 5, po.CLR, 256),
}


@pytest.mark.parametrize("reset", [1, 0])
@pytest.mark.parametrize("name", sorted(SIZE_CASES))
def test_chunk_sizes_and_bounds(name, reset):
    W, H, J, tr, B = SIZE_CASES[name]
    X = rows_for(tr, B, J, 9)
    init = gen.random_map(W * H, po.length(tr, J), seed=7)
    sigmas, sc = sched(5, 3.0, 0.25)
    assert len(sigmas) == 5
    run(W, H, J, tr, X, init, sigmas, reset, (name, reset), sched=sc)


# ---- values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [1, 0])
@pytest.mark.parametrize("name", ["nan_row", "nan_at_node0", "inf_values", "sigma_1_and_below", "zero_over_zero_16x16"])
def test_values(name, reset):
    W, H, J, tr, B = 8, 6, 7, po.STANDARD, 30
    sigmas = [3.0, 2.2, 1.6, 1.2]
    if name == "zero_over_zero_16x16":
        # (float)exp(-d^2 / (2 sigma^2)) is 0 once d^2 > 207.9 sigma^2 (below 2^-150); row 0 is node 0's model vector, so
        # its BMU is the corner and the far corner lies d^2 = 450 away: at sigma 1.2 every node past d^2 = 299 starts its
        # chain with W = 0 and c = 0/0
        W, H, J, B = 16, 16, 4, 12
        sigmas = [1.2, 1.1, 1.2]
    X = rows_for(tr, B, J, 3)
    init = gen.random_map(W * H, J, seed=13)
    if name == "zero_over_zero_16x16":
        X[0] = init[0]
    elif name == "nan_row":
        X[B // 2, J // 2] = np.nan
    elif name == "nan_at_node0":
        init[0, 1] = np.nan
    elif name == "inf_values":
        X[1, 0] = np.inf
        X[2, 3] = -np.inf
        init[5, 2] = np.inf
    elif name == "sigma_1_and_below":
        sigmas = [2.0, 1.0, 0.7, 1.5, 0.7]
    run(W, H, J, tr, X, init, sigmas, reset, (name, reset))
    if name == "zero_over_zero_16x16":
        # the case does what it is for: some node saw 0/0
        o = po.OracleSom(W, H, J, tr)
        o.set_state(map=init)
        sref.oracle_loop(o, X, sigmas[:1])
        assert np.isnan(o.map[W * H - 1]).all() and not np.isnan(o.map[0]).any()


# ---- the launch split ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [1, 0])
def test_more_epochs_than_one_launch_holds(reset):
    """3x3x2, B = 4, VSOM_SCHEDULE_MAX_EPOCHS + 3 epochs of one sigma: two launches, the exact search only in the first"""
    W, H, J, B = 3, 3, 2, 4
    X = rows_for(po.STANDARD, B, J, 2)
    init = gen.random_map(W * H, J, seed=3)
    run(W, H, J, po.STANDARD, X, init, [1.5] * (MAXE + 3), reset, ("split", reset), oracle=False)


def update_launches(ctx):
    """the launches the context's "update" timer has seen since the last look (the one-workgroup kernels are in that
    group: the single epoch counts one per call, a schedule one per launch)"""
    return ctx.get_timing()["update"][1]


def test_the_schedule_runs_as_one_launch_per_1024_epochs():
    """what tells the one-launch kernels from the loop they replace: with the "update" group timed, a schedule counts
    one launch per VSOM_SCHEDULE_MAX_EPOCHS epochs, the loop (here forced by a NaN sigma) one per epoch"""
    W, H, J, B = 3, 3, 2, 4
    m, t = make_pair(W, H, J, po.STANDARD, gen.random_map(W * H, J, seed=3))
    X = rows_for(po.STANDARD, B, J, 2)
    for ctx in (m, t):
        ctx.upload_chunk(X)
        ctx.enable_timing(True, groups=["update"])
        update_launches(ctx)
    m.batch_schedule([1.5] * (MAXE + 3))
    assert update_launches(m) == 2
    m.batch_schedule([3.0, 2.0, 1.5])
    assert update_launches(m) == 1
    m.batch_schedule([1.5] * MAXE)
    assert update_launches(m) == 1
    m.batch_schedule([3.0, np.nan, 1.5])
    assert update_launches(m) == 3
    sref.twin_loop(t, [3.0, 2.0, 1.5])
    assert update_launches(t) == 3
    m.close()
    t.close()


def test_python_resident_training_equals_train_batch_som():
    """Som.trainBatchSomResident against Som.trainBatchSom on the device: the fixture (33 of 40 epochs) and a map above
    the one-launch bound; state, metrics, lastBMU, and the stream left at its start"""
    for W, H, X, args in ((10, 10, fixture_rows(), (40, 5.0, 0.05)), (24, 20, rows_for(po.STANDARD, 60, 11, 4), (4, 3.0, 0.15))):
        got = []
        for resident in (False, True):
            data = vs.ArrayDataSet(X)
            som = vs.Som(W, H, data)
            som.randomInitialize(7, 1.0)
            (som.trainBatchSomResident if resident else som.trainBatchSom)(data, *args)
            assert data.isAtStartOfDataStream() and not data.hasReadWholeDataStream()
            got.append((som.state(), np.array(som.metrics.MeanSquaredError, np.float32), data.lastBMU.copy()))
            som.close()
        (sa, ma, la), (sb, mb, lb) = got
        for k in KEYS:
            assert beq(sa[k], sb[k]), (W, H, k)
        assert beq(ma, mb) and beq(la, lb), (W, H)
        ran = len(vs.batch_sigma_schedule(*args))
        assert (mb[:ran] > 0).all() and (mb[ran:] == 0).all()


# ---- fallbacks -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [1, 0])
def test_map_above_the_tiny_bound(reset):
    W, H, J, B = 20, 20, 16, 50
    sigmas, sc = sched(4, 4.0, 0.3)
    run(W, H, J, po.STANDARD, rows_for(po.STANDARD, B, J, 4), gen.random_map(W * H, J, seed=5), sigmas, reset,
        ("20x20x16", reset), sched=sc)


@pytest.mark.parametrize("reset", [1, 0])
def test_custom_context(reset):
    W, H, J, B = 6, 5, 7, 30
    run(W, H, J, po.STANDARD, rows_for(po.STANDARD, B, J, 4), gen.random_map(W * H, J, seed=5), [3.0, 2.0, 1.4], reset,
        ("custom", reset), custom="standard")


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("reset", [1, 0])
def test_non_finite_sigma_in_the_middle(reset, bad):
    W, H, J, B = 6, 5, 7, 30
    run(W, H, J, po.STANDARD, rows_for(po.STANDARD, B, J, 4), gen.random_map(W * H, J, seed=5), [3.0, bad, 2.0, 1.4], reset,
        ("bad sigma", reset), oracle=False)


def test_without_the_one_launch_kernels():
    """VSOM_NO_TINY=1 is read when a context is created: a child interpreter runs the kinds and chunk-size cases with it"""
    env = dict(os.environ)
    env["VSOM_NO_TINY"] = "1"
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", os.path.abspath(__file__),
           "-k", "test_fixture_and_kinds or B3 or B256_the_tiny_bound"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-2000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, tail


# ---- after the call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [1, 0])
def test_calls_that_follow_a_schedule(reset):
    """the single-epoch call caches its neighbourhood table by sigma: a schedule must not leave it stale.  Before the
    schedule both contexts tabulate sigma 2.5; afterwards one epoch at 2.5 (the cached value), one at a fresh sigma, an
    online chunk and a search must equal the twin's"""
    W, H, J, B = 10, 10, 9, 20
    X, init = fixture_rows(), gen.random_map(W * H, J, seed=42)
    m, t = make_pair(W, H, J, po.STANDARD, init)
    for ctx in (m, t):
        ctx.upload_chunk(X)
        ctx.batch_epoch(2.5, True)
    sigmas = [4.0, 3.0, 2.0]
    same(m, t, m.batch_schedule(sigmas, reset_bmu=reset), sref.twin_loop(t, sigmas, reset_bmu=reset), "schedule")
    # (the twin's own cache now holds 2.0: give it the same history by value, not by cache state)
    for sigma in (2.5, 1.7):
        a, b = m.batch_epoch(sigma, False), t.batch_epoch(sigma, False)
        same(m, t, np.array([a], np.float32), np.array([b], np.float32), ("epoch after", sigma))
    # the cached value once more after a second schedule that ends on another sigma
    same(m, t, m.batch_schedule([3.5, 1.7], reset_bmu=reset), sref.twin_loop(t, [3.5, 1.7], reset_bmu=reset), "second")
    a, b = m.batch_epoch(1.7, False), t.batch_epoch(1.7, False)
    same(m, t, np.array([a], np.float32), np.array([b], np.float32), "epoch at the sigma cached before the second schedule")
    ma, la = m.train_online_chunk_fetch(0.05, 2.0, capi.EXPONENTIAL, first_chunk=True)
    mb, lb = t.train_online_chunk_fetch(0.05, 2.0, capi.EXPONENTIAL, first_chunk=True)
    assert beq(np.float32(ma), np.float32(mb)) and beq(la, lb)
    ia, da = m.bmu_batch()
    ib, db = t.bmu_batch()
    assert beq(ia, ib) and beq(da, db)
    sa, sb = m.get_state(), t.get_state()
    for k in KEYS:
        assert beq(sa[k], sb[k]), k
    m.close()
    t.close()


def test_no_epochs_is_a_no_op():
    W, H, J = 6, 5, 7
    m, t = make_pair(W, H, J, po.STANDARD, gen.random_map(W * H, J, seed=5))
    assert m.batch_schedule([]).shape == (0,)          # no chunk loaded: still nothing to do
    X = rows_for(po.STANDARD, 10, J, 1)
    m.upload_chunk(X)
    t.upload_chunk(X)
    assert m.batch_schedule([], reset_bmu=False).shape == (0,)
    a, b = m.get_state(), t.get_state()
    for k in KEYS:
        assert beq(a[k], b[k]), k
    m.close()
    t.close()


# ---- ensembles -------------------------------------------------------------------------------------------------------
class Member:
    def __init__(self, W, H, J, tr, B, seed, sigmas, custom=None):
        self.W, self.H, self.J, self.tr = W, H, J, tr
        self.X = rows_for(tr, B, J, seed)
        D = po.length(tr, J) if custom is None else hooks.shape(custom, J)[0]
        self.init = gen.random_map(W * H, D, seed=seed + 3)
        self.m, self.t = make_pair(W, H, J, tr, self.init, custom)
        self.sigmas = list(sigmas)
        for ctx in (self.m, self.t):
            ctx.upload_chunk(self.X)

    def close(self):
        self.m.close()
        self.t.close()


_STREAM = []


def shared_stream():
    """one stream for the members of an ensemble, alive for the whole module (contexts keep the handle)"""
    import torch
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream(device=torch.device("cuda", 0)))
    return _STREAM[0]


def ensemble_round(members, reset, what, shared=False, sigmas=None):
    stream = shared_stream() if shared else None
    if shared:
        for mb in members:
            mb.m.set_stream(stream.cuda_stream)
    ens = vsom_amd.Ensemble([mb.m for mb in members])
    mses = ens.batch_schedule([mb.sigmas for mb in members] if sigmas is None else sigmas, reset_bmu=reset)
    assert len(mses) == len(members)
    for k, mb in enumerate(members):
        mse_t = sref.twin_loop(mb.t, mb.sigmas, reset_bmu=reset)
        same(mb.m, mb.t, mses[k], mse_t, (what, k))
    ens.close()
    if stream is not None:
        stream.synchronize()


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("reset", [1, 0])
def test_ensemble_of_kinds_lengths_and_paths(reset, shared):
    """the three kinds with different schedule lengths (0 and 1 among them), equal shapes on different schedules, and
    members on their ordinary path (a map above the bound, a custom context, a NaN sigma) in the same call; members on
    one stream and each on its own"""
    members = [
        Member(10, 10, 9, po.STANDARD, 20, 11, [4.0, 3.0, 2.2, 1.6, 1.2]),
        Member(5, 11, 10, po.MEDIAN, 60, 12, [3.0]),
        Member(5, 4, 6, po.CLR, 40, 13, [2.5, 2.0, 1.6]),
        Member(9, 7, 13, po.STANDARD, 70, 14, []),
        Member(10, 10, 9, po.STANDARD, 20, 15, [3.0, 2.2, 1.0, 0.7]),      # the shape of member 0, another schedule
        Member(20, 20, 16, po.STANDARD, 50, 16, [4.0, 3.0]),               # above the tiny bound
        Member(6, 5, 7, po.STANDARD, 30, 17, [3.0, 2.0], custom="standard"),
        Member(6, 5, 7, po.MEDIAN, 30, 18, [3.0, np.nan, 2.0]),
        Member(10, 10, 9, po.STANDARD, 20, 11, [4.0, 3.0, 2.2, 1.6, 1.2]),  # member 0 again: every table shared
    ]
    before = members[3].m.get_state()
    ensemble_round(members, reset, ("mixed", reset, shared), shared=shared)
    after = members[3].m.get_state()
    for k in KEYS:
        assert beq(before[k], after[k]), ("the member without epochs", k)
    # a second call on the same members: the schedules continue from the state the first left
    ens_members = [mb for k, mb in enumerate(members) if k != 3]
    ensemble_round(ens_members, reset, ("again", reset, shared), shared=shared)
    for mb in members:
        mb.close()


def test_more_members_than_compute_units_share_one_schedule():
    """300 members (an MI355X has 256 CUs) of 6x5x4 on one sigma schedule given once; three different seeds of rows"""
    sigmas = vs.batch_sigma_schedule(6, 3.0, 0.2)
    members = [Member(6, 5, 4, po.STANDARD, 12, 20 + k % 3, sigmas) for k in range(300)]
    stream = shared_stream()
    for mb in members:
        mb.m.set_stream(stream.cuda_stream)
    ens = vsom_amd.Ensemble([mb.m for mb in members])
    for mb in members[:3]:
        mb.m.enable_timing(True, groups=["update"])
        update_launches(mb.m)
    mses = ens.batch_schedule(sigmas, reset_bmu=True)
    # the launches of an ensemble are not timed; a member on the loop would count one launch per epoch
    assert [update_launches(mb.m) for mb in members[:3]] == [0, 0, 0]
    # the twins of the three distinct members, every member against its kind's twin
    twins = {}
    for k in range(3):
        mb = members[k]
        twins[k] = (sref.twin_loop(mb.t, sigmas, reset_bmu=True), mb.t.get_state(), mb.t.get_last_bmu(), mb.t.get_sqres())
    for k, mb in enumerate(members):
        mse_t, st, lb, sq = twins[k % 3]
        assert beq(mses[k], mse_t), k
        a = mb.m.get_state()
        for key in KEYS:
            assert beq(a[key], st[key]), (k, key)
        assert beq(mb.m.get_last_bmu(), lb) and beq(mb.m.get_sqres(), sq), k
        assert beq(np.float32(mb.m.get_mse()), mse_t[-1]), k
    ens.close()
    stream.synchronize()
    for mb in members:
        mb.close()


def test_ensemble_launch_split_with_unequal_lengths():
    """members past VSOM_SCHEDULE_MAX_EPOCHS beside short ones, each on its own stream: the second round's launch holds
    the short members with no epochs left"""
    members = [Member(3, 3, 2, po.STANDARD, 4, 31, [1.5] * (MAXE + 2)), Member(3, 3, 2, po.MEDIAN, 4, 32, [1.5, 1.2]),
               Member(3, 2, 2, po.STANDARD, 5, 33, [2.0] * 3)]
    ensemble_round(members, 1, "ensemble split")
    for mb in members:
        mb.close()


# ---- refusals --------------------------------------------------------------------------------------------------------
def snapshot(ctx, rows=True):
    st = ctx.get_state()
    out = [st[k].copy() for k in KEYS]
    if rows:
        out += [ctx.get_last_bmu().copy(), ctx.get_sqres().copy(), np.float32(ctx.get_mse())]
    return out


def unchanged(a, b):
    return len(a) == len(b) and all(beq(x, y) for x, y in zip(a, b))


def test_refusals_leave_the_state_untouched():
    import ctypes as C
    L = capi.lib()
    W, H, J, B = 10, 10, 9, 20
    X, init = fixture_rows(), gen.random_map(W * H, J, seed=42)
    sig = (C.c_double * 3)(3.0, 2.0, 1.5)
    out = (C.c_float * 3)()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    assert L.vsom_batch_schedule(None, sig, 3, 1, out) != 0
    a, b = make_pair(W, H, J, po.STANDARD, init)
    before = snapshot(a, rows=False)
    with pytest.raises(capi.VsomError, match="no chunk loaded"):
        a.batch_schedule([3.0, 2.0])
    assert unchanged(before, snapshot(a, rows=False))
    a.upload_chunk(X)
    a.batch_epoch(3.0, True)
    before = snapshot(a)
    assert L.vsom_batch_schedule(a._h, None, 3, 1, out) != 0
    assert L.vsom_batch_schedule(a._h, sig, 3, 1, None) != 0
    assert L.vsom_batch_schedule(a._h, None, 0, 1, None) == 0          # nothing to do: no array is read
    assert unchanged(before, snapshot(a))

    # ensembles: every member is checked before anything runs, and the message names the member
    b.upload_chunk(X)
    c, c_t = make_pair(W, H, J, po.STANDARD, init)                     # no chunk
    ens = vsom_amd.Ensemble([a, b, c])
    with pytest.raises(capi.VsomError, match="member 2: no chunk loaded"):
        ens.batch_schedule([3.0, 2.0])
    assert ens.batch_schedule([[3.0], [2.0], []])[2].shape == (0,)      # ... unless that member has no epochs
    # a custom member without a chunk behind members that would be launched: refused before anything runs
    d, r = hooks.shape("standard", J)
    cu = capi.Context(W, H, J, capi.CUSTOM, source=hooks.SOURCES["standard"], depth=d, residual_len=r)
    cu.set_state(map=init)
    with pytest.raises(capi.VsomError, match="no chunk loaded"):
        cu.batch_schedule([3.0, 2.0])
    ens_cu = vsom_amd.Ensemble([a, b, cu])
    ab = [snapshot(a), snapshot(b)]
    with pytest.raises(capi.VsomError, match="member 2: no chunk loaded"):
        ens_cu.batch_schedule([3.0, 2.0])
    assert unchanged(ab[0], snapshot(a)) and unchanged(ab[1], snapshot(b))
    ens_cu.close()
    cu.close()
    a2, b2 = make_pair(W, H, J, po.STANDARD, init)
    for ctx in (a2, b2):
        ctx.upload_chunk(X)
    ens2 = vsom_amd.Ensemble([a2, b2])
    befores = [snapshot(a2), snapshot(b2)]
    sigs = (dp * 2)(C.cast(sig, dp), None)
    outs = (fp * 2)(C.cast(out, fp), C.cast(out, fp))
    cnt = (C.c_size_t * 2)(3, 3)
    assert L.vsom_ensemble_batch_schedule(ens2._h, sigs, cnt, 1, outs) != 0
    assert b"member 1" in L.vsom_last_error()
    sigs = (dp * 2)(C.cast(sig, dp), C.cast(sig, dp))
    outs = (fp * 2)(None, C.cast(out, fp))
    assert L.vsom_ensemble_batch_schedule(ens2._h, sigs, cnt, 1, outs) != 0
    assert b"member 0" in L.vsom_last_error()
    assert L.vsom_ensemble_batch_schedule(ens2._h, sigs, None, 1, outs) != 0
    assert L.vsom_ensemble_batch_schedule(None, sigs, cnt, 1, outs) != 0
    assert L.vsom_ensemble_batch_schedule(ens2._h, None, cnt, 1, outs) != 0
    assert unchanged(befores[0], snapshot(a2)) and unchanged(befores[1], snapshot(b2))
    for e in (ens, ens2):
        e.close()
    for ctx in (a, b, c, c_t, a2, b2):
        ctx.close()


def test_a_chunk_staged_ahead_is_refused():
    """a map whose batch epoch frees the staged rows early, so that a prefetch stages the next chunk over them (as
    tests/test_gpu_ensemble.py): the schedule must not read those rows"""
    W = H = 48
    J = 196
    xs = [gen.mnist_like(1100, seed=70 + i, dim=J) for i in range(2)]
    init = (gen.random_map(W * H, J, seed=42) * np.float32(100) + np.float32(100)).astype(np.float32)
    big = vsom_amd.Context(W, H, J)
    pb = capi.PinnedBuffer(xs[1].shape)
    pb.array[...] = xs[1]
    big.set_state(map=init)
    big.upload_chunk(xs[0])
    small, small_t = make_pair(10, 10, 9, po.STANDARD, gen.random_map(100, 9, seed=42))
    small.upload_chunk(fixture_rows())
    ens = vsom_amd.Ensemble([small, big])
    big.batch_epoch_async(10.0, True)
    big.prefetch_chunk(pb.array)         # staged beside the chains of chunk 0
    before = snapshot(small)
    with pytest.raises(capi.VsomError, match="staged ahead"):
        big.batch_schedule([3.0, 2.0])
    with pytest.raises(capi.VsomError, match="member 1: the next chunk is staged ahead"):
        ens.batch_schedule([3.0, 2.0])
    assert unchanged(before, snapshot(small))
    big.commit_chunk()
    mses = ens.batch_schedule([[3.0, 2.0], [12.0]])
    assert len(mses[0]) == 2 and len(mses[1]) == 1
    ens.close()
    for ctx in (big, small, small_t):
        ctx.close()
    pb.free()
