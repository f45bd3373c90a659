"""An evaluation's plan (gumbi_amd/csrc/eval_plan.hpp) against the frozen copy of the two-site logic on loose engine fields that it
replaced, over the full grid of its inputs: tools/eval_plan_check.cpp built with the system's C++ compiler and run.  No GPU; the
sanitizer build of the same file is run by hand (the command is in its head)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def test_eval_plan_check_builds_and_passes(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "eval_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", str(ROOT / "tools" / "eval_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
