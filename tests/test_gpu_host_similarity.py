"""GPU: Som::similarityRows and Som::measureSimilarity of the C++ mirror (host/tests/host_similarity_test.cpp), on one GPU
and through a three-member group on one device (VSOM_DEVICES=0,0,0).  The mirror's per-row report must equal the Python
binding's bit for bit, measureSimilarity the restated reference loop, and the driver itself asserts that the call downloads
no model state."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import vsom_amd
from vsom_amd import capi
from oracle import pyoracle as po

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import similarity_ref as ref  # noqa: E402
from similarity_ref import beq  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")
FIELDS = (("bmu", np.uint64), ("dist", np.float32), ("dmax", np.float32), ("dmax_col", np.uint32), ("first", np.float32),
          ("amax", np.float32), ("amax_col", np.uint32), ("outside", np.uint32))


def read_dump(path):
    raw = open(path, "rb").read()
    W, H, J, n, ns = (int(x) for x in np.frombuffer(raw[:40], np.uint64))
    N, off = W * H, 40
    out = {"W": W, "H": H, "J": J, "n": n, "settings": []}

    def take(dt, cnt):
        nonlocal off
        a = np.frombuffer(raw, dt, cnt, off)
        off += cnt * np.dtype(dt).itemsize
        return a

    out["map"] = take(np.float32, N * J).reshape(N, J)
    out["sigma"] = take(np.float32, N * J).reshape(N, J)
    out["hits"] = take(np.uint64, N)
    out["rows"] = take(np.float32, n * J).reshape(n, J)
    out["valid"] = take(np.uint8, n * J).reshape(n, J)
    for _ in range(ns):
        sigmas, hits, floor, verdict = (int(x) for x in take(np.int64, 4))
        rep = {k: take(dt, n) for k, dt in FIELDS}
        rep["delta"] = take(np.float32, n * J).reshape(n, J)
        out["settings"].append((sigmas, hits, bool(floor), verdict, rep))
    assert off == len(raw)
    return out


@pytest.mark.parametrize("mode", ["single", "group3"])
def test_cpp_similarity_rows_and_measure_similarity(mode):
    exe = os.path.join(HOST, "host_similarity_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    d = tempfile.mkdtemp(prefix="vsom_similarity_")
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    if mode == "group3":
        env["VSOM_DEVICES"] = "0,0,0"
    res = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert ("group_members=3" if mode == "group3" else "group_members=1") in res.stdout
    assert "no state download ok" in res.stdout
    f = read_dump(os.path.join(d, "similarity.bin"))
    W, H, J, n = f["W"], f["H"], f["J"], f["n"]
    assert len(f["settings"]) == 7 and (f["sigma"] > 1e-5).any() and f["hits"].max() > 1
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=f["map"], sigma=f["sigma"], hits=f["hits"])
    ctx.upload_chunk(f["rows"])
    o = po.OracleSom(W, H, J)
    o.set_state(map=f["map"], sigma=f["sigma"], hits=f["hits"])
    verdicts = set()
    for sigmas, hits, floor, verdict, rep in f["settings"]:
        got = ctx.similarity(hits, sigmas, capi.SIGMA_FLOOR if floor else capi.SIGMA_AS_WRITTEN, valid=f["valid"], delta=True)
        for k in got:
            assert beq(got[k], rep[k]), (sigmas, hits, floor, k)
        if not floor:
            b = np.array([o.find_restricted_bmu(x, hits) for x in f["rows"]], np.int64)
            assert (b == rep["bmu"].astype(np.int64)).all()
            delta, lo, hi = ref.columns(f["rows"], o.map[b], o.sigma[b], sigmas, False)
            row, ok = ref.literal_loop(delta, f["rows"], lo, hi, f["valid"])
            assert verdict == int(ok), (sigmas, hits)
            verdicts.add(verdict)
        else:
            assert verdict == -1
    assert verdicts == {0, 1}                          # both outcomes occur among the settings
    ctx.close()
