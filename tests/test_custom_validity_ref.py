"""No GPU: the numpy restatement of the host path for hooks that use valueWeight (tests/custom_validity_ref.py) against the
bits of that host path itself -- host_custom_validity_test runs the same hooks as C++ lambdas through a Som over an
in-test IDataLoader with NULLs and column weights (the state stays on the host) and prints its inputs and results as
hexfloat.  Also what the device-side feature shows without a device: the hook sources compile, the six calls refuse a
null context.  (Their refusal of a built-in context needs a context, hence a device: tests/test_gpu_custom_validity.py.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import custom_validity_hooks as vhooks
import custom_validity_ref as ref
from vsom_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "host_custom_validity_test")
f32 = np.float32


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool((a == b).all())


@pytest.fixture(scope="module")
def host():
    """name -> values of every line the driver's host mode prints"""
    if not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([EXE, "host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        if name.endswith((".hits", ".last")):
            out[name] = np.array([int(v) for v in vals], np.uint64)
        else:
            out[name] = np.array([float.fromhex(v) for v in vals], np.float64).astype(f32)
    return out


def inputs(host, k):
    W, H, J, rows, chunk = (int(v) for v in host[f"in{k}.shape"])
    X = host[f"in{k}.x"].reshape(rows, J)
    valid = host[f"in{k}.valid"].reshape(rows, J)
    w = host[f"in{k}.weights"]
    som_state = host[f"in{k}.init"].reshape(W * H, J), host[f"in{k}.sig"].reshape(W * H, J)
    return W, H, J, rows, chunk, X, valid, w, som_state


def replay(host, k, hook, mode):
    """the driver's run `mode` of input k, restated: what Som::train / the single-vector members do on the host path"""
    W, H, J, rows, chunk, X, valid, w, (init, sig) = inputs(host, k)
    s = ref.ValiditySom(W, H, J, hook)
    s.set_state(map=init, sigma=sig)
    vf, vw = ref.value_weights(valid, w, rows, J)
    chunks = [(a, min(rows, a + chunk)) for a in range(0, rows, chunk)]
    mses, singles, last = [], [], np.zeros(0, np.uint64)
    if mode == "batch":
        for e in range(2):
            sigma = 2.0 * np.exp(-0.3 * e)
            mse = f32(0)
            for a, b in chunks:
                last = np.zeros(b - a, np.uint64)          # a load zeroes lastBMU
                mse = f32(mse + s.batch_epoch(X[a:b], vf[a:b], vw[a:b], last, sigma, e == 0))
            mses.append(f32(mse / f32(len(chunks))))
    elif mode in ("exp", "inv"):
        fn = ref.EXPONENTIAL if mode == "exp" else ref.INVERSE_PROPORTIONAL
        for e in range(2):
            eta, sigma = 0.5 * np.exp(-0.3 * e), max(1.6 * np.exp(-0.6 * e), 1.0)
            mse = f32(0)
            for a, b in chunks:
                last = np.zeros(b - a, np.uint64)
                mse = s.train_chunk(X[a:b], vw[a:b], last, eta, sigma, fn, mse_start=mse)
            mses.append(f32(mse / f32(len(chunks))))
    else:
        lb = 0
        for i in range(6):
            s.vw = vw[i]
            singles += [f32(s.find_bmu(X[i])), f32(s.find_local_bmu(X[i], 2)), s.dist(i + 1, X[i])]
            bmu, res, dist, lb = s.train_single(X[i], vw[i], 0.4, 0.9 if i % 2 else 1.7, lb,
                                                ref.EXPONENTIAL if i < 3 else ref.INVERSE_PROPORTIONAL)
            singles += [f32(bmu), dist, *res]
        last = np.array([lb], np.uint64)
    return s, np.array(mses, f32), np.array(singles, f32), last


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("hook", ["select", "scaled"])
@pytest.mark.parametrize("mode", ["batch", "exp", "inv", "singles"])
def test_numpy_restatement_matches_host_lambdas(host, k, hook, mode):
    s, mses, singles, last = replay(host, k, hook, mode)
    c = f"in{k}.{hook}.{mode}"
    for name, mine in (("map", s.map), ("sigma", s.sigma), ("S", s.S), ("weight", s.weight), ("hits", s.hits),
                       ("mse", mses), ("singles", singles), ("last", last)):
        assert beq(np.asarray(mine).ravel(), host[f"{c}.{name}"]), f"{c}.{name} differs from the host-lambda path"


def test_inputs_have_nulls_and_weights(host):
    for k in (0, 1):
        W, H, J, rows, chunk, X, valid, w, _ = inputs(host, k)
        assert not valid[3].any() and not valid[:, J - 2].any() and 0.1 < 1 - valid.mean() < 0.6
        assert {0.0, 2.5, 0.5} <= set(float(v) for v in w)


@pytest.mark.parametrize("name", sorted(vhooks.SOURCES))
def test_hook_sources_compile(name):
    capi.custom_compile_check(vhooks.SOURCES[name], 17, 17)


def test_the_six_calls_refuse_a_null_context():
    L = capi.lib()
    v = np.zeros(3, f32)
    vb = (C.c_uint8 * 3)(1, 1, 1)
    u, d = C.c_uint64(), C.c_float()
    refused = [
        L.vsom_set_column_weights(None, capi._f(v)),
        L.vsom_set_chunk_validity(None, vb, 0),
        L.vsom_find_bmu_valid(None, capi._f(v), vb, C.byref(u), C.byref(d)),
        L.vsom_find_local_bmu_valid(None, capi._f(v), vb, 0, C.byref(u), C.byref(d)),
        L.vsom_dist_single_valid(None, capi._f(v), vb, 0, C.byref(d)),
        L.vsom_train_single_valid(None, capi._f(v), vb, 0.1, 1.0, C.byref(u), capi.EXPONENTIAL, None, None, None),
    ]
    assert refused == [-1] * 6
    assert "null context" in L.vsom_last_error().decode()
