"""The walk over a SELECTION of an additive model's covariance terms (gumbi_amd/csrc/term_walk.hpp) with recording stubs:
tools/term_select_check.cpp -- every mask of T = 1, 3, 5 terms, with and without failing bodies and preparations -- built with the
system's C++ compiler and run.  No GPU; the sanitizer build of the same file is run by hand (the command is in its head)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_term_select_check_builds_and_passes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "term_select_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", str(ROOT / "tools" / "term_select_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all cases agree" in run.stdout
