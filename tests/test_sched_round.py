"""The round image of a resident schedule (csrc/vsom_sched_round.hpp), on the host: what the one-launch schedule kernels of
tiny maps read per round -- the deduplicated neighbourhood tables, every member's table offsets, the members' validity
bytes -- as the single-context and the ensemble schedule calls lay it out.  A C++ driver (tests/sched_round_driver.cpp)
pins the layout: tables shared by (shape, sigma's bits) in the order of first use, -0.0 apart from 0.0, a member whose
schedule has ended, the validity offsets of B x J / one-row / plain members, the refusal of more than 2^32 table values
(from the size computation alone), and the table values themselves.  No device and no library are needed: the header is
plain host C++, and the driver is a program of its own, built with AddressSanitizer and UBSan where the toolchain has
them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "variational-self-organizing-maps_amd", "csrc")


def _compile(cxx, out, extra):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, *extra,
           os.path.join(ROOT, "tests", "sched_round_driver.cpp"), "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_round_image_layout(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("needs a host C++ compiler")
    exe = str(tmp_path / "sched_round_driver")
    r = _compile(cxx, exe, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    if r.returncode != 0:                      # a toolchain without the sanitizers: the plain build
        r = _compile(cxx, exe, [])
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok")
