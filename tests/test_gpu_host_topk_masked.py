"""GPU: Som::findBestMatchingUnitsMasked, Som::topographicErrorMasked and Som::imputeBlend of the C++ mirror
(host/tests/host_topk_masked_test.cpp): on an all-valid data set they are findBestMatchingUnits / topographicError / the rows
themselves, under validity zeros with garbage behind them entry 0 is findMaskedBmus', the padding and the imputed values are
as the header states, and nothing downloads the model state."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def test_cpp_mirror_driver():
    exe = os.path.join(HOST, "host_topk_masked_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "state_downloads=0" in res.stdout
    assert "host_topk_masked_test ok" in res.stdout
