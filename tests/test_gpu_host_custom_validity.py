"""GPU: the C++ mirror hands a device-hook Som (Transformation::Device) the loader's NULLs and column weights.
host_custom_validity_test, device mode, trains batch and both online decays through Som::train over a loader with NULLs
and weights, and runs the single-vector members with a validity vector, once with the hooks as host lambdas and once as
device source; every result must be bit-identical."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_hooks_match_host_lambdas_over_nulls_and_weights():
    exe = os.path.join(ROOT, "variational-self-organizing-maps_amd", "host", "host_custom_validity_test")
    if not os.path.exists(exe):
        import __graft_entry__
        __graft_entry__.build()
    r = subprocess.run([exe, "device"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "DIFFERENT" not in r.stdout
    assert "custom validity device parity ok" in r.stdout
