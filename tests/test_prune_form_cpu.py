"""Which instantiation of the pruning kernels a launch takes (hyphy_amd/csrc/prune_form.h): the selector against the frozen
transcription of the cascades it replaced, membership in the list of compiled instantiations, no fused-combine target without the build
that serves it, LDS and grid bounds, reachability of every listed instantiation, over the whole key space, through
tests/prune_form_check.cpp.  Compiled with the host compiler (the header needs nothing of HIP), run as a child process; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prune_form_on_the_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++) to build tests/prune_form_check.cpp with")
    exe = tmp_path / "prune_form_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "prune_form_check.cpp"),
                            "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "prune_form_check: ok"
