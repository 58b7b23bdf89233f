"""GPU: Som::drawModelVectors and Som::variationalAutoEncoder of the C++ mirror (host/tests/host_bmd_test.cpp), on one
GPU and through a three-member group on one device (VSOM_DEVICES=0,0,0).  The mirror's draws and norms must equal
the Python binding's bit for bit; variationalAutoEncoder's engineered cases are checked by the program itself."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import vsom_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def read_draws(path):
    raw = open(path, "rb").read()
    W, H, J, n, min_hits = (int(x) for x in np.frombuffer(raw[:40], np.uint64))
    N, off = W * H, 40
    out = {"W": W, "H": H, "J": J, "n": n, "min_hits": min_hits}
    for k, dt, cnt in (("map", np.float32, N * J), ("hits", np.uint64, N), ("rows", np.float32, n * J),
                       ("u", np.float64, n), ("draw", np.uint64, n), ("norm", np.float64, n)):
        out[k] = np.frombuffer(raw, dt, cnt, off)
        off += cnt * np.dtype(dt).itemsize
    assert off == len(raw)
    return out


@pytest.mark.parametrize("mode", ["single", "group3"])
def test_cpp_draws_and_vae(mode):
    exe = os.path.join(HOST, "host_bmd_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    d = tempfile.mkdtemp(prefix="vsom_bmd_")
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    if mode == "group3":
        env["VSOM_DEVICES"] = "0,0,0"
    res = subprocess.run([exe, d], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert ("group_members=3" if mode == "group3" else "group_members=1") in res.stdout
    for tag in ("vae_one ok", "vae_two ok", "vae_none ok"):
        assert tag in res.stdout
    f = read_draws(os.path.join(d, "bmd_draws.bin"))
    W, H, J = f["W"], f["H"], f["J"]
    ctx = vsom_amd.Context(W, H, J)
    ctx.set_state(map=f["map"].reshape(W * H, J), hits=f["hits"])
    ctx.upload_chunk(f["rows"].reshape(f["n"], J))
    got = ctx.restricted_bmd(f["min_hits"], u=f["u"])
    ctx.close()
    assert (got["draw"] == f["draw"]).all()
    assert (got["norm"].view(np.uint64) == f["norm"].view(np.uint64)).all()
    assert (f["draw"] < W * H).all() and (f["hits"][f["draw"]] >= f["min_hits"]).all()
