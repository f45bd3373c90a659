"""The engine's validity marks (gumbi_amd/csrc/factor_state.hpp) against the frozen copy of the loose fields and assignments they
replaced, over every short sequence of ABI calls: tools/factor_state_check.cpp built with the system's C++ compiler and run.  No GPU;
the sanitizer build of the same file is run by hand (the command is in its head)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_factor_state_check_builds_and_passes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "factor_state_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", str(ROOT / "tools" / "factor_state_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
