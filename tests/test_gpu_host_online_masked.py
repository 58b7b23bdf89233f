"""GPU: Som::trainBasicSomMasked of the C++ mirror (host/tests/host_online_masked_test.cpp) on a 9x7x11 map over 50 rows in
two chunks with validity zeros and NaN / inf at the invalid positions.  The driver itself asserts that the all-valid schedule
is trainBasicSom, that the flags matter, that garbage at invalid positions changes nothing and that training downloads no
model state; here its final state, metrics and BMUs must equal, bit for bit, the Python binding's on the same inputs."""
import math
import os
import subprocess

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
f32 = np.float32


def parse(stdout):
    out = {}
    for ln in stdout.splitlines():
        tok = ln.split()
        if len(tok) >= 2 and tok[0] in ("shape", "schedule", "rows", "valid", "map0", "sigma0", "S0", "weight0", "map", "sigma",
                                        "S", "weight", "hits", "mse", "lastbmu"):
            out[tok[0]] = tok[1:]
    return out


def floats(tok, dtype=f32):
    return np.array([float.fromhex(t) for t in tok], dtype)


def beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def test_cpp_train_basic_som_masked_equals_the_python_binding():
    exe = os.path.join(HOST, "host_online_masked_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr
    assert "host_online_masked_test ok" in res.stdout
    f = parse(res.stdout)
    W, H, J, rows, chunk, epochs = (int(t) for t in f["shape"])
    eta0, eta_decay, sigma0, sigma_decay = (float.fromhex(t) for t in f["schedule"])
    X = floats(f["rows"]).reshape(rows, J)
    valid = np.array([int(t) for t in f["valid"]], np.uint8).reshape(rows, J)
    assert 0 < np.count_nonzero(valid == 0) < valid.size and not valid[:, 4].any()
    X = np.where(valid != 0, X, f32(np.nan))          # (the driver's loader put NaN / inf / 1e30 there)

    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=floats(f["map0"]).reshape(W * H, J), sigma=floats(f["sigma0"]).reshape(W * H, J),
                  S=floats(f["S0"]).reshape(W * H, J), weight=floats(f["weight0"]))
    metrics, clamped = [], 0
    for e in range(epochs):
        eta = eta0 * math.exp(-eta_decay * float(e))
        sigma = sigma0 * math.exp(-sigma_decay * float(e))
        if sigma < 1.0:
            sigma, clamped = 1.0, clamped + 1
        count = 0
        for r0 in range(0, rows, chunk):
            ctx.upload_chunk(np.ascontiguousarray(X[r0:r0 + chunk]))
            mse, lb = ctx.train_online_chunk_masked(eta, sigma, capi.INVERSE_PROPORTIONAL, valid[r0:r0 + chunk],
                                                    first_chunk=(count == 0))
            count += 1
        metrics.append(f32(mse / f32(count)))
    assert clamped >= 1 and count == 2
    st = ctx.get_state()
    ctx.close()
    for k in ("map", "sigma", "S"):
        assert beq(st[k], floats(f[k]).reshape(W * H, J)), k
    assert beq(st["weight"], floats(f["weight"]))
    assert (st["hits"] == np.array([int(t) for t in f["hits"]], np.uint64)).all() and st["hits"].sum() == rows * epochs
    assert beq(np.array(metrics, f32), floats(f["mse"]))
    assert (lb == np.array([int(t) for t in f["lastbmu"]], np.uint64)).all()
