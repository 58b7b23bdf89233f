"""GPU: Som::evaluate and Som::evaluateRows of the C++ mirror (host/tests/host_evaluate_test.cpp) on a 10x10x9 map over 50
rows with 3 binary columns and validity zeros.  The mirror's per-row report must equal the Python binding's on the same state
bit for bit, its scalar the recurrence over those rows, the all-continuous value the running mean of the oracle's distances,
and the driver itself asserts that the call downloads no model state."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vsom_amd
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import evaluate_ref as ref  # noqa: E402
from evaluate_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
W, H, J, B = 10, 10, 9, 50


def parse(stdout):
    out = {}
    for ln in stdout.splitlines():
        tok = ln.split()
        if len(tok) >= 2 and "=" not in tok[0]:
            out[tok[0]] = tok[1:]
    return out


def floats(tok, dtype=np.float32):
    return np.array([float.fromhex(t) for t in tok], dtype)


def test_cpp_evaluate_and_evaluate_rows():
    exe = os.path.join(HOST, "host_evaluate_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_evaluate_test ok" in res.stdout and "state_downloads_by_evaluate=0" in res.stdout
    f = parse(res.stdout)
    # a Transformation::Device Som keeps the host loop (the driver compares it with its rows' own searches and exits non-zero)
    assert float.fromhex(f["evaluate_device_source"][0]) > 0
    M = floats(f["map"]).reshape(W * H, J)
    X = floats(f["rows"]).reshape(B, J)
    valid = np.array([int(t) for t in f["valid"]], np.uint8).reshape(B, J)
    binary = np.array([int(t) for t in f["binary"]], np.float32)
    continuous = np.array([int(t) for t in f["continuous"]], np.float32)
    assert np.count_nonzero(binary) == 3 and (continuous == 1).all()
    assert 0 < np.count_nonzero(valid == 0) < valid.size and set(np.unique(valid)) == {0, 1}
    rep = {"bmu": np.array([int(t) for t in f["bmu"]], np.uint64), "dist": floats(f["dist"]), "bsum": floats(f["bsum"]),
           "nrepl": np.array([int(t) for t in f["nrepl"]], np.uint32)}

    # the rows against the C-ABI call on the same state
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=M)
    ctx.upload_chunk(X)
    got = ctx.evaluate(binary, continuous, valid=valid)
    assert (got["bmu"] == rep["bmu"]).all() and (got["nrepl"] == rep["nrepl"]).all()
    assert beq(got["dist"], rep["dist"]) and beq(got["bsum"], rep["bsum"])
    # ... and against the float64 restatement, within the stated tolerance
    b64, n64 = ref.restate64(X, M[rep["bmu"].astype(np.int64)], binary, continuous, valid)
    assert (rep["nrepl"] == n64).all()
    nz = b64 != 0
    assert nz.any() and (np.abs(rep["bsum"][nz].astype(np.float64) - b64[nz]) <= ref.bound(J) * b64[nz]).all()
    assert (rep["bsum"][~nz] == 0).all()
    # the scalar against the recurrence
    want = ref.running_mean(rep["dist"], rep["bsum"])
    assert ref.same_double(float.fromhex(f["evaluate"][0]), want)
    assert ref.same_double(float.fromhex(f["rows_error"][0]), want)
    assert ref.same_double(got["error"], want)
    ctx.close()

    # all-continuous, all-valid: bit-identical to the running mean of the oracle's distances
    o = po.OracleSom(W, H, J)
    o.set_state(map=M)
    err = 0.0
    for i in range(B):
        err += 1.0 / (i + 1.0) * (o.dist(o.find_bmu(X[i]), X[i]) - err)
    assert float.fromhex(f["evaluate_plain"][0]) == err
