"""The device-byte ledger after each of a fixed sequence of calls: what every call allocates, and in which order it grows.

    python tools/gpu_workspace_ledger.py                       the in-tree library
    GUMBI_HIP_LIB=/path/to/libgumbi_hip.so python tools/...    another build of it

For A/B runs of two builds of the library: a change that moves no allocation prints the same lines.  The problem is the suite's
``fit_4224`` (Matern-5/2, d = 2, N = 4224, 400 grid points), behind ``evaluate(theta, grad=True)`` as after a MAP fit, so the
predictions take the product form.  After each call one line: ``resident_bytes()`` and ``resident_bytes(peak=True)``.  No timing, no
threshold.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gumbi_amd.engine import Engine, KernelSpec  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

N, D = 4224, 2


def main():
    X, y, ls = O.synthetic_table(N, D, seed=4224)
    spec = O.make_spec(D, range(D), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.3)
    Xs = O.synthetic_grid(D, res=20)
    M = Xs.shape[0]
    rows = np.arange(7, 7 + 3 * 150, 3)  # 150 training rows left out together
    offsets = np.concatenate([np.arange(0, 130), [M]])  # 129 singleton groups and the rest in one
    Z = np.random.default_rng(0).standard_normal((3, M))
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(KernelSpec(D=D, idx_cont=list(range(D)), kind=spec["kind"], ard=spec["ard"], jitter=spec["jitter"]))
        eng.set_theta(theta)
        eng.evaluate(theta, grad=True)
        calls = [
            ("evaluate(grad=True)", lambda: None),
            ("predict", lambda: eng.predict(Xs)),
            ("predict_joint", lambda: eng.predict_joint(Xs)),
            ("draw_joint", lambda: eng.draw_joint(Xs, Z)),
            ("leave_out(cov=True)", lambda: eng.leave_out(rows, cov=True)),
            ("loo", lambda: eng.loo()),
            ("predict_groups(cov=True)", lambda: eng.predict_groups(Xs, offsets, cov=True)),
            ("predict_groups", lambda: eng.predict_groups(Xs, offsets)),
            ("predict_decompose", lambda: eng.predict_decompose(Xs)),
            ("predict_slope(cov=True)", lambda: eng.predict_slope(Xs, cov=True)),
            ("predict_with_grad", lambda: eng.predict_with_grad(Xs)),
        ]
        for name, call in calls:
            call()
            print(f"{name:<26s} resident {eng.resident_bytes():>12d}  peak {eng.resident_bytes(peak=True):>12d}", flush=True)


if __name__ == "__main__":
    main()
