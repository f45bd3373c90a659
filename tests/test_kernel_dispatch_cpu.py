"""The dispatch of (kernel kind, padded width) to the covariance kernels' template constants (gumbi_amd/csrc/kernel_dispatch.hpp) with
a recording functor: tools/kernel_dispatch_check.cpp built with the system's C++ compiler and run.  No GPU; the sanitizer build of
the same file is run by hand (the command is in its head)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_kernel_dispatch_check_builds_and_passes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "kernel_dispatch_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", str(ROOT / "tools" / "kernel_dispatch_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
