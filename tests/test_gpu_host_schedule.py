"""GPU: Som::trainBatchSomResident of the C++ mirror (host/tests/host_schedule_test.cpp).  The driver trains the same
one-chunk ArrayDataLoader data set with trainBatchSom and with trainBatchSomResident -- the reference fixture's shape on the
one-launch path and a map above its bound -- and exits non-zero unless the state, the metrics and getLastBMU agree bit for
bit; it also checks that a two-chunk data set throws before anything trains and that a multi-device Som throws."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host")


def test_cpp_resident_schedule_equals_train_batch_som():
    exe = os.path.join(HOST, "host_schedule_test")
    if not os.path.exists(exe):
        subprocess.check_call(["bash", os.path.join(HOST, "build.sh")], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    env.pop("VSOM_DEVICES", None)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host_schedule_test ok" in res.stdout
