"""Golden host posterior for the C3 full-size parity test (tests/test_gpu_configs.py::test_c3_full_size_sampled_parity_against_the_host).

C3 = N = 50k, d = 8, Matern-5/2 ARD at theta = (generator length scales, eta = 1, sigma = 0.2): the oracle's arithmetic at FULL size
(tests/host_reference.py: the 50k x 50k covariance built block-wise with PyMC's distance expansion, one in-place LAPACK dpotrf,
the solves) at 32 points sampled from the 10^4-point grid -> mean, variance, NLML.  It needs ~24 GB of host memory and minutes of
host time, which is why the GPU test reads the stored result instead of recomputing it beside the GPU run.

The dpotrf runs with at most 8 BLAS threads: the threaded dpotrf of the OpenBLAS that scipy bundles (0.3.28) crashes with a
segmentation fault on this 50k matrix with 16 threads.

Usage:  python tests/golden/make_c3_host_goldens.py
"""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from host_reference import host_posterior_blockwise  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

N, D, N_SAMPLED, SAMPLE_SEED = 50_000, 8, 32, 11


def main():
    from threadpoolctl import threadpool_limits

    X, y, ls = O.synthetic_table(N, D)
    spec = O.make_spec(D, range(D), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    Xs = O.synthetic_grid(D, res=100)
    sub = np.sort(np.random.default_rng(SAMPLE_SEED).choice(len(Xs), N_SAMPLED, replace=False))
    with threadpool_limits(limits=8, user_api="blas"):
        mu, var, nlml = host_posterior_blockwise(spec, theta, X, y, Xs[sub])
    out = HERE / "c3_host_goldens.npz"
    np.savez(out, sub=sub, theta=theta, mu=mu, var=var, nlml=np.array(nlml))
    print(f"wrote {out}: nlml {nlml:.10f}, mean[:3] {mu[:3]}, var[:3] {var[:3]}")


if __name__ == "__main__":
    main()
