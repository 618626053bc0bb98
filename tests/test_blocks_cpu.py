"""The owner of a shard's device and pinned blocks (hyphy_amd/csrc/blocks.h), on the host alone: tests/blocks_host_check.cpp links
the header against a malloc-backed pool of its own that aborts on a free of a block it does not hold and can fail the k-th
allocation.  Compiled with the host compiler (of HIP only the hipError_t type is needed), run as a child process; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_block_owner_on_the_host(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++ / clang++) to build tests/blocks_host_check.cpp with")
    exe = tmp_path / "blocks_host_check"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + ROCM_INCLUDE, "-D__HIP_PLATFORM_AMD__",
                            os.path.join(ROOT, "tests", "blocks_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "blocks_host_check: ok"
