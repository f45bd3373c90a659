"""The engine's workspaces and the budgets of its guarded calls (gumbi_amd/csrc/workspaces.hpp, the Budget of device_buffers.hpp) over
a host allocator: tools/workspace_budget_check.cpp built with the system's C++ compiler and run.  No GPU; the sanitizer build of the
same file is run by hand (the command is in its head)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_workspace_budget_check_builds_and_passes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "workspace_budget_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "workspace_budget_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "workspace budgets agree" in run.stdout
