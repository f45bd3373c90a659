"""Goldens of the large launch shapes of tests/test_gpu_composite_limits.py: the float64 oracle's NLML and gradient
(``O.nlml_and_grad``, direct distances) of every problem of ``composite_reference.LARGE_CASES``, so that the GPU tests do not
spend the oracle's O(N^3) on the host.  The problems come back from their seeds (``composite_reference.large_problem``);
stored per case: theta, nlml, grad -- nothing else.  Longdouble is not affordable at these sizes.

Wall time: about a minute.

Usage:  python tests/golden/make_composite_limits_goldens.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import composite_reference as CR  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402


def main():
    out = {}
    for name in CR.LARGE_CASES:
        spec, theta, X, y = CR.large_problem(name)
        val, grad = O.nlml_and_grad(spec, theta, X, y, dist_mode="direct")
        out[f"{name}/theta"], out[f"{name}/nlml"], out[f"{name}/grad"] = theta, np.float64(val), grad
        print(f"{name}: N = {len(y)}, nlml {val:.6f}, |grad| {np.min(np.abs(grad)):.2e} .. {np.max(np.abs(grad)):.2e}")
    np.savez(HERE / "composite_limits_goldens.npz", **out)


if __name__ == "__main__":
    main()
