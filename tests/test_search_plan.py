"""The decision table of the BMU search (csrc/vsom_search_plan.hpp), on the host: a C++ driver fills contexts by hand, calls
vsom_search_plan, vsom_exact_plan and vsom_sl_backoff_step and compares the path, the form and kernels of the integer
contraction, every buffer size, grid and threshold factor, the duplicate-row passes and the back-off with literals -- on
both sides of every threshold, so a rule that moves by one tile fails here although every path computes the same bits.  No
device is needed (the HIP headers only; the runtime library is linked but never called)."""
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
           os.path.join(ROOT, "tests", "search_plan_driver.cpp"), "-o", out,
           "-L", os.path.join(ROCM, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_search_decision_table(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None or not os.path.isdir(os.path.join(ROCM, "include", "hip")):
        pytest.skip("needs a host C++ compiler and the HIP headers")
    exe = str(tmp_path / "search_plan_driver")
    r = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:                      # a toolchain without the sanitizers: the plain build
        r = _compile(cxx, exe, [])
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
