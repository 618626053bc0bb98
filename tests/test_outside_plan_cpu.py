"""What the chunked outside pass plans on the host (hyphy_amd/csrc/outside_plan.h): the requests of a call grouped by branch, the
tiles of a chunk under the scratch budget and the stride of the per-tile records, through tests/outside_plan_check.cpp.  Compiled
with the host compiler (the header needs nothing of HIP), run as a child process; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_outside_plan_on_the_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++) to build tests/outside_plan_check.cpp with")
    exe = tmp_path / "outside_plan_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "outside_plan_check.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "outside_plan_check: ok"
