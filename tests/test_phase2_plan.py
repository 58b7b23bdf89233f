"""The decision table of phase 2 (csrc/vsom_phase2_plan.hpp), on the host: a C++ driver fills contexts by hand, calls
vsom_phase2_plan and compares the path, geometry, launch shape, kernel, deferral, rows-free offer and what follows the chains
with literals -- at the thresholds between the small-map and the quad kernels, between the one-quad and two-quad mean-only
forms and around the two-round limit of the rows-free offer, so a threshold that moves by one workgroup fails here although
every path computes the same bits.  No device is needed (the HIP headers only; the runtime library is linked but never
called)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "variational-self-organizing-maps_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-result", "-I", CSRC,
           "-I", os.path.join(ROCM, "include"), "-D__HIP_PLATFORM_AMD__", *extra,
           os.path.join(ROOT, "tests", "phase2_plan_driver.cpp"), "-o", out,
           "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_phase2_decision_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not os.path.isdir(os.path.join(ROCM, "include", "hip")):
        pytest.skip("needs a host C++ compiler and the HIP headers")
    exe = str(tmp_path / "phase2_plan_driver")
    r = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:                      # a toolchain without the sanitizers: the plain build
        r = _compile(cxx, exe, [])
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
