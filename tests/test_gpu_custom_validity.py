"""GPU: a custom context hands its hooks the value_weight row the reference would build -- the loaded chunk's validity
(vsom_set_chunk_validity) times the column weights (vsom_set_column_weights); include/vsom_hip.h, "value_weight".

Everything is bit-exact (NaN == NaN) against tests/custom_validity_ref.py, the numpy restatement of the host path for
custom hooks that tests/test_custom_validity_ref.py pins against that host path itself.  The reference of a case is
computed once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import gen
import custom_hooks
import custom_validity_hooks as vhooks
import custom_validity_ref as ref
from vsom_amd import capi
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
f32 = np.float32

# W, H, J, B: below one packet; a packet and a scalar tail; many packets with a packet tail
SHAPES = {"j3": (7, 5, 3, 61), "j17": (9, 6, 17, 77), "j794": (12, 9, 794, 64)}
# how validity and weights are set: a B x J mask with weights, the one_mask form with weights, weights alone
CONFIGS = ("rows", "one", "weights")


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


@functools.lru_cache(maxsize=None)
def case(shape):
    """inputs of a shape: rows, a B x J mask (about 20 % invalid, row 2 without a valid column, column J - 2 invalid in
    every row), a column mask, weights with a 0, a 2.5 and a 0.5, and an initial state whose sigmaMap has zeros"""
    W, H, J, B = SHAPES[shape]
    rng = np.random.default_rng(100 + J)
    X = gen.blobs(B, J, 4, 1, 2 + J)
    rows = rng.random((B, J)) >= 0.2
    rows[2, :] = False
    rows[:, J - 2] = False
    one = rng.random(J) >= 0.3
    one[J - 1] = True
    w = np.ones(J, f32)
    w[0], w[J // 2], w[J - 1] = 0.0, 2.5, 0.5
    init = gen.random_map(W * H, J, 5 + J)
    sig = (np.abs(gen.random_map(W * H, J, 6 + J)) * f32(0.5)).astype(f32)
    sig[:, ::3] = 0.0
    for a in (X, rows, one, w, init, sig):
        a.setflags(write=False)
    return dict(W=W, H=H, J=J, B=B, X=X, rows=rows, one=one, w=w, init=init, sig=sig)


def settings(c, config):
    """(valid, one_mask, weights) of a configuration"""
    return {"rows": (c["rows"], False, c["w"]), "one": (c["one"], True, c["w"]), "weights": (None, False, c["w"]),
            "rows_unit": (c["rows"], False, None), "unset": (None, False, None)}[config]


def make_ctx(c, hook="select", source=None, state=True):
    ctx = capi.Context(c["W"], c["H"], c["J"], capi.CUSTOM, source=source or vhooks.SOURCES[hook], depth=c["J"],
                       residual_len=c["J"])
    if state:
        ctx.set_state(map=c["init"], sigma=c["sig"])
    return ctx


def apply(ctx, c, config, X=None):
    valid, one, w = settings(c, config)
    ctx.upload_chunk(c["X"] if X is None else X)
    if w is not None:
        ctx.set_column_weights(w)
    if valid is not None:
        ctx.set_chunk_validity(valid, one_mask=one)


def ref_som(c, hook="select"):
    s = ref.ValiditySom(c["W"], c["H"], c["J"], hook)
    s.set_state(map=c["init"], sigma=c["sig"])
    return s


def ref_vw(c, config):
    valid, _, w = settings(c, config)
    return ref.value_weights(valid, w, c["B"], c["J"])


def snapshot(s, last, mse):
    return dict(map=s.map.copy(), sigma=s.sigma.copy(), S=s.S.copy(), weight=s.weight.copy(), hits=s.hits.copy(),
                last=np.array(last, np.uint64), mse=f32(mse))


def assert_snapshot(ctx, want, mse, what):
    st = ctx.get_state()
    for k in ("map", "sigma", "S", "weight", "hits"):
        assert beq(st[k], want[k]), f"{what}: {k} differs from the reference"
    assert beq(ctx.get_last_bmu(), want["last"]), f"{what}: lastBMU"
    assert beq(f32(mse), want["mse"]), (what, mse, want["mse"])


# ---- searches and distances ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_searches(shape, config, hook):
    c = case(shape)
    s = ref_som(c, hook)
    _, vw = ref_vw(c, config)
    full = s.bmu_rows(c["X"], vw)
    start = (np.arange(c["B"]) * 7 % (c["W"] * c["H"])).astype(np.uint64)
    local = s.bmu_rows(c["X"], vw, start)
    nodes = np.array([0, 5, c["W"] * c["H"] - 1, 13, 1], np.uint64)
    rows = np.array([0, c["B"] - 1, 2, 2, 7], np.uint64)
    return full, start, local, nodes, rows, s.dist_pairs(c["X"], vw, nodes, rows)


# (SCALED, the hook that reads the dispersion and with it the 1e-5 floor, at one shape)
SEARCHES = [("select", shape, config) for shape in SHAPES for config in CONFIGS] + [("scaled", "j17", cfg) for cfg in CONFIGS]


@pytest.mark.parametrize("hook,shape,config", SEARCHES)
def test_searches_and_distances(hook, shape, config):
    c = case(shape)
    full, start, local, nodes, rows, dists = ref_searches(shape, config, hook)
    ctx = make_ctx(c, hook)
    apply(ctx, c, config)
    idx, dist = ctx.bmu_batch()
    assert beq(idx, full[0]) and beq(dist, full[1]), "bmu_batch"
    ctx.set_last_bmu(start)
    idx, dist = ctx.bmu_local_batch()
    assert beq(idx, local[0]) and beq(dist, local[1]), "bmu_local_batch"
    assert beq(ctx.distances(nodes, rows), dists), "distances"
    ctx.close()


# ---- batch epochs: validity set once holds over both epochs of the chunk ------------------------------------------------
@functools.lru_cache(maxsize=None)
def ref_batch(shape, config):
    c = case(shape)
    s = ref_som(c)
    valid, vw = ref_vw(c, config)
    last = np.zeros(c["B"], np.uint64)
    out = []
    for e, sigma in enumerate((2.5, 1.3)):
        mse = s.batch_epoch(c["X"], valid, vw, last, sigma, e == 0)
        out.append(snapshot(s, last, mse))
    return out


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_two_batch_epochs_first_and_local(shape, config):
    c = case(shape)
    want = ref_batch(shape, config)
    ctx = make_ctx(c)
    apply(ctx, c, config)
    for e, sigma in enumerate((2.5, 1.3)):
        mse = ctx.batch_epoch(sigma, e == 0)
        assert_snapshot(ctx, want[e], mse, f"epoch {e}")
    ctx.close()


# ---- online chunks ---------------------------------------------------------------------------------------------------
ONLINE = [(shape, "rows", fn, sigma) for shape in SHAPES for fn in (po.EXPONENTIAL, po.INVERSE_PROPORTIONAL)
          for sigma in (2.2, 0.9)]
ONLINE += [("j17", "one", po.EXPONENTIAL, 2.2), ("j17", "weights", po.INVERSE_PROPORTIONAL, 0.9)]


@functools.lru_cache(maxsize=None)
def ref_online(shape, config, fn, sigma):
    c = case(shape)
    s = ref_som(c)
    _, vw = ref_vw(c, config)
    last = np.zeros(c["B"], np.uint64)
    mse = s.train_chunk(c["X"], vw, last, 0.3, sigma, fn)
    return snapshot(s, last, mse)


@pytest.mark.parametrize("shape,config,fn,sigma", ONLINE)
def test_online_chunk(shape, config, fn, sigma):
    c = case(shape)
    want = ref_online(shape, config, fn, sigma)
    ctx = make_ctx(c)
    apply(ctx, c, config)
    mse = ctx.train_online_chunk(0.3, sigma, fn)
    assert_snapshot(ctx, want, mse, "online chunk")
    ctx.close()


# ---- the four _valid calls -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_single_vector_valid_calls(shape):
    c = case(shape)
    s = ref_som(c)
    _, vw = ref_vw(c, "rows")
    ctx = make_ctx(c)
    ctx.set_column_weights(c["w"])
    last_r = last_g = 0
    for i in (0, 2, 5, 9):                      # (row 2 has no valid column)
        v, valid = c["X"][i], c["rows"][i]
        s.vw = vw[i]
        assert ctx.find_bmu(v, valid=valid) == (s.find_bmu(v), s.dist(s.find_bmu(v), v))
        lb = s.find_local_bmu(v, 3)
        assert ctx.find_local_bmu(v, 3, valid=valid) == (lb, s.dist(lb, v))
        assert beq(ctx.dist_single(v, 4, valid=valid), s.dist(4, v))
        fn, sigma = (po.EXPONENTIAL, 1.8) if i % 2 else (po.INVERSE_PROPORTIONAL, 0.8)
        br, rr, dr, last_r = s.train_single(v, vw[i], 0.2, sigma, last_r, fn)
        bg, rg, dg, last_g = ctx.train_single(v, 0.2, sigma, last_g, fn, valid=valid)
        assert (br, last_r) == (bg, last_g) and beq(rg, rr) and beq(dg, dr), f"train_single_valid of row {i}"
    st = ctx.get_state()
    for k in ("map", "sigma", "S", "weight"):
        assert beq(st[k], getattr(s, k)), k
    # without valid= the vector is all valid and the column weights still apply
    v = c["X"][1]
    s.vw = c["w"]
    assert ctx.find_bmu(v) == (s.find_bmu(v), s.dist(s.find_bmu(v), v))
    assert beq(ctx.dist_single(v, 4), s.dist(4, v))
    assert ctx.find_bmu(v, valid=np.ones(c["J"])) == ctx.find_bmu(v)
    ctx.close()


# ---- poison: what stands at an invalid position reaches nothing -------------------------------------------------------
def test_nan_and_inf_at_invalid_positions_change_no_bit():
    c = case("j17")
    clean = np.where(c["rows"], c["X"], f32(0)).astype(f32)
    poison = clean.copy()
    bad = np.array([np.nan, np.inf, -np.inf], f32)
    holes = np.argwhere(~c["rows"])
    poison[holes[:, 0], holes[:, 1]] = bad[np.arange(len(holes)) % 3]
    got = []
    for X in (clean, poison):
        ctx = make_ctx(c)
        apply(ctx, c, "rows", X)
        out = [*ctx.bmu_batch()]
        out.append(ctx.batch_epoch(2.0, True))
        out.append(ctx.batch_epoch(1.2, False))
        out.append(ctx.train_online_chunk(0.3, 1.6, po.EXPONENTIAL))
        out.append(ctx.train_online_chunk(0.3, 0.9, po.INVERSE_PROPORTIONAL))
        st = ctx.get_state()
        got.append(out + [st[k] for k in ("map", "sigma", "S", "weight", "hits")] + [ctx.get_last_bmu()])
        ctx.close()
    assert not any(np.isnan(np.asarray(a, np.float64)).any() for a in got[0][:6])
    for a, b in zip(*got):
        assert beq(np.asarray(a), np.asarray(b))


# ---- nothing changed --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["never_set", "all_valid_unit_weights", "hook_ignores_value_weight"])
def test_standard_source_keeps_the_oracles_bits(how):
    """the restated Standard source: a run that never calls the setters, one that sets all-valid bytes and unit weights,
    and -- the hook never reads value_weight -- one with a mask and weights all give the oracle's bits"""
    c = case("j17")
    W, H, J, B = c["W"], c["H"], c["J"], c["B"]
    o = po.OracleSom(W, H, J, po.STANDARD)
    o.set_state(map=c["init"], sigma=c["sig"])
    ctx = make_ctx(c, source=custom_hooks.SOURCES["standard"])
    ctx.upload_chunk(c["X"])
    if how == "all_valid_unit_weights":
        ctx.set_column_weights(np.ones(J, f32))
        ctx.set_chunk_validity(np.ones((B, J), np.uint8))
    elif how == "hook_ignores_value_weight":
        ctx.set_column_weights(c["w"])
        ctx.set_chunk_validity(c["rows"])
    lbo = np.zeros(B, np.uint64)
    for e, sigma in enumerate((2.0, 1.2)):
        mse_o = o.batch_epoch(c["X"], lbo, sigma, e == 0)
        mse = ctx.batch_epoch(sigma, e == 0)
        assert beq(ctx.get_last_bmu(), lbo) and beq(f32(mse), f32(mse_o))
    run_o = o.train_online_chunk(c["X"], lbo, 0.3, 1.5, po.EXPONENTIAL, mse_start=0.0)
    run = ctx.train_online_chunk(0.3, 1.5, po.EXPONENTIAL)
    assert beq(ctx.get_last_bmu(), lbo) and beq(f32(run), f32(run_o))
    st = ctx.get_state()
    for k, want in (("map", o.map), ("sigma", o.sigma), ("S", o.S), ("weight", o.weight), ("hits", o.hits)):
        assert beq(st[k], want), f"{how}: {k} differs from the oracle"
    ctx.close()


def test_all_valid_rows_and_unit_weights_change_no_bit_of_a_hook_that_reads_them():
    """SELECT reads value_weight in every hook call: with a B x J mask of ones and unit weights set, the launches read the
    expanded [B][J] arrays (stride J) and must give the bits of a run that never calls the setters (the ones vector)"""
    c = case("j17")
    got = []
    for set_them in (False, True):
        ctx = make_ctx(c)
        ctx.upload_chunk(c["X"])
        if set_them:
            ctx.set_column_weights(np.ones(c["J"], f32))
            ctx.set_chunk_validity(np.ones((c["B"], c["J"]), np.uint8))
        out = [*ctx.bmu_batch(), ctx.distances(np.array([3, 8], np.uint64), np.array([1, 5], np.uint64))]
        out.append(ctx.batch_epoch(2.0, True))
        out.append(ctx.batch_epoch(1.2, False))
        out.append(ctx.train_online_chunk(0.3, 1.6, po.EXPONENTIAL))
        out.append(ctx.train_online_chunk(0.3, 0.9, po.INVERSE_PROPORTIONAL))
        st = ctx.get_state()
        got.append(out + [st[k] for k in ("map", "sigma", "S", "weight", "hits")] + [ctx.get_last_bmu()])
        ctx.close()
    for a, b in zip(*got):
        assert beq(np.asarray(a), np.asarray(b))
    want = ref_searches("j17", "unset", "select")[0]
    assert beq(got[1][0], want[0]) and beq(got[1][1], want[1])


# ---- lifecycle --------------------------------------------------------------------------------------------------------
def test_validity_belongs_to_the_chunk_and_weights_to_the_context():
    c = case("j17")
    masked, _, _, _, _, _ = ref_searches("j17", "rows", "select")
    weighted, _, _, _, _, _ = ref_searches("j17", "weights", "select")
    ctx = make_ctx(c)
    apply(ctx, c, "rows")
    ctx.set_last_bmu(np.zeros(c["B"], np.uint64))            # survives set_last_bmu and set_state
    ctx.set_state(map=c["init"], sigma=c["sig"])
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), masked)), "validity after set_last_bmu / set_state"
    ctx.upload_chunk(c["X"])                                 # a new chunk is all valid; the weights stay
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), weighted)), "after upload_chunk"
    ctx.set_chunk_validity(c["rows"])
    ctx.prefetch_chunk(c["X"])
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), masked)), "a prefetch alone changes nothing"
    ctx.prefetch_wait()
    ctx.commit_chunk()
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), weighted)), "after prefetch / commit"
    ctx.set_chunk_validity(c["rows"])
    ctx.set_chunk_validity(None)
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), weighted)), "validity set back to all valid"
    ctx.set_chunk_validity(c["rows"])
    ctx.set_column_weights(None)                             # the mask stays when the weights go
    plain, _, _, _, _, _ = ref_searches("j17", "rows_unit", "select")
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), plain)), "weights unset under a mask"
    ctx.close()


def test_ensemble_upload_resets_a_custom_members_validity():
    c = case("j17")
    masked, _, _, _, _, _ = ref_searches("j17", "rows", "select")
    weighted, _, _, _, _, _ = ref_searches("j17", "weights", "select")
    ctx = make_ctx(c)
    ens = capi.Ensemble([ctx])
    apply(ctx, c, "rows")
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), masked))
    ens.upload_chunks([c["X"]])
    assert all(beq(a, b) for a, b in zip(ctx.bmu_batch(), weighted)), "after vsom_ensemble_upload_chunks"
    ens.close()
    ctx.close()


# ---- the masked family computes the same distance ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_plain_select_equals_bmu_masked_batch(shape):
    """select(valid, m - x, +0) summed in the packet order: bmu_batch of a PLAIN_SELECT custom context with unit weights
    and vsom_bmu_masked_batch(min_hits = 0) of a Standard context give the same (index, distance) bits"""
    c = case(shape)
    ctx = make_ctx(c, "plain_select")
    apply(ctx, c, "rows_unit")
    idx, dist = ctx.bmu_batch()
    ctx.close()
    std = capi.Context(c["W"], c["H"], c["J"], capi.STANDARD)
    std.set_state(map=c["init"], sigma=c["sig"])
    std.upload_chunk(c["X"])
    m = std.bmu_masked(c["rows"], min_hits=0)
    std.close()
    assert beq(idx, m["bmu"]) and beq(dist, m["dist"])


# ---- the Python Som takes validity and weights from the data set ---------------------------------------------------------
def test_python_som_takes_validity_and_weights_from_the_data_set():
    from vsom_amd import som

    class ValidDataSet(som.ArrayDataSet):
        """an ArrayDataSet whose loaded rows carry validity flags"""

        def __init__(self, X, V, chunk, weights):
            super().__init__(X, chunk, weights=weights)
            self.V = V

        def loadNextDataFromStream(self):
            pos = self._pos
            super().loadNextDataFromStream()
            self.validity = self.V[pos:pos + self.data.shape[0]]

    c = case("j17")
    W, H, J, B = c["W"], c["H"], c["J"], c["B"]
    chunk = 40                                              # two chunks: each brings its own validity
    vf, vw = ref_vw(c, "rows")
    for online in (False, True):
        s = som.Som(W, H, ValidDataSet(c["X"], c["rows"], chunk, c["w"]), som.Transformation.Custom(vhooks.SELECT, J, J))
        s.setState(map=c["init"], sigma=c["sig"])
        r = ref_som(c)
        data = ValidDataSet(c["X"], c["rows"], chunk, c["w"])
        mses = []
        for e in range(2):
            mse = f32(0)
            for a in range(0, B, chunk):
                b, last = min(B, a + chunk), np.zeros(min(B, a + chunk) - a, np.uint64)
                if online:
                    mse = r.train_chunk(c["X"][a:b], vw[a:b], last, 0.4 * np.exp(-0.2 * e), 1.7, po.EXPONENTIAL, mse_start=mse)
                else:
                    mse = f32(mse + r.batch_epoch(c["X"][a:b], vf[a:b], vw[a:b], last, 2.0 * np.exp(-0.3 * e), e == 0))
            mses.append(f32(mse / f32(2)))
        if online:
            s.trainBasicSom(data, 2, 0.4, 0.2, 1.7, 0.0, som.WeigthDecayFunction.Exponential)
        else:
            s.trainBatchSom(data, 2, 2.0, 0.3)
        st = s.state()
        for k in ("map", "sigma", "weight"):
            assert beq(st[k], getattr(r, k)), (online, k)
        assert beq(np.asarray(s.metrics.MeanSquaredError, f32), np.array(mses, f32)), online
        v, valid = c["X"][5], c["rows"][5]
        r.vw = vw[5]
        assert s.findBmu(v, valid, c["w"]) == som.SomIndex(r.find_bmu(v) % W, r.find_bmu(v) // W)
        assert beq(f32(s.euclidianWeightedDist(3, v, valid, c["w"])), r.dist(3, v))
        s.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_context_usable():
    c = case("j3")
    J, B = c["J"], c["B"]
    L = capi.lib()
    v = c["X"][0].copy()
    vb = (C.c_uint8 * J)(*([1] * J))
    rows = (C.c_uint8 * (B * J))(*([1] * (B * J)))
    u, d, lb = C.c_uint64(), C.c_float(), C.c_uint64(0)

    def six(h):
        return [L.vsom_set_column_weights(h, capi._f(v)), L.vsom_set_chunk_validity(h, rows, 0),
                L.vsom_find_bmu_valid(h, capi._f(v), vb, C.byref(u), C.byref(d)),
                L.vsom_find_local_bmu_valid(h, capi._f(v), vb, 0, C.byref(u), C.byref(d)),
                L.vsom_dist_single_valid(h, capi._f(v), vb, 0, C.byref(d)),
                L.vsom_train_single_valid(h, capi._f(v), vb, 0.1, 1.5, C.byref(lb), capi.EXPONENTIAL, None, None, None)]

    # a built-in context: all six, with a message that names the masked calls
    std = capi.Context(c["W"], c["H"], J, capi.STANDARD)
    std.set_state(map=c["init"])
    std.upload_chunk(c["X"])
    assert six(std._h) == [-1] * 6
    msg = L.vsom_last_error().decode()
    assert "valueWeight" in msg and "vsom_bmu_masked_batch" in msg
    o = po.OracleSom(c["W"], c["H"], J, po.STANDARD)
    o.set_state(map=c["init"])
    lbo = np.zeros(B, np.uint64)
    assert beq(f32(std.batch_epoch(1.5, True)), f32(o.batch_epoch(c["X"], lbo, 1.5, True)))
    assert beq(std.get_state()["map"], o.map)
    std.close()
    # a custom context with no chunk
    ctx = make_ctx(c)
    assert L.vsom_set_chunk_validity(ctx._h, rows, 0) == -1
    assert "no chunk" in L.vsom_last_error().decode()
    want = ref_batch("j3", "rows")[0]
    apply(ctx, c, "rows")
    mse = ctx.batch_epoch(2.5, True)
    assert_snapshot(ctx, want, mse, "after the refusal")
    ctx.close()
