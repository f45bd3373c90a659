"""Goldens of the ill-conditioned parity tests (tests/test_gpu_conditioning.py): extended-precision results and the float64
host's own error, per case.

Each case is a table whose Sigma = K + sigma^2 I + jitter I is ill-conditioned the way MAP fits on smooth, low-noise data make
it: (a) jitter-limited smooth 1-D tables, (b) near-duplicate and exactly repeated inputs, (c) ARD length scales spanning two
orders of magnitude, (d) one moderately conditioned control; plus a composite model (linear term x coregion x two outputs) and a two-output
table on shared inputs (the Kronecker path).
The sizes reach the launch tree (N ~ 300), the tile Cholesky / fused evaluation / GEMM-form prediction (N ~ 1000 - 1300) and
the tile triangular solve of the prediction (N = 2700 with 4200 test points); most N are not multiples of 128.  Test points:
every fifth training input shifted by 1e-3 (the noiseless variance there is ~0 and k** - |A|^2 cancels) and random points.

Stored per case ``<case>/<key>``: the inputs (X, y, Xs, theta, spec = the make_spec keywords as JSON); the extended-precision
results of tests/precise_reference.py (mean, var, var_noise, nlml, alpha, grad); ``e64_<key>``, the error of the float64 host
path (LAPACK potrf + triangular solves, the oracle's gradient with inverse="trsm") against them -- max |host - ref|, the 2-norm for grad; and ``cond``,
``pivot_margin`` = min diag(L)^2 / (eps max diag Sigma) of the LAPACK factor.  Vectors only, no matrices.

Wall time: ~8 minutes on one CPU core (numpy's longdouble products run single-threaded).

Usage:  python tests/golden/make_conditioning_goldens.py
"""
import json
import sys
import time
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

import precise_reference as P  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402

EPS = np.finfo(float).eps


def _points(X, rng, m_rand, lo, hi):
    near = X[::5].copy()
    near[:, 0] += 1e-3
    return np.vstack([near, rng.uniform(lo, hi, (m_rand, X.shape[1]))])


def cases():
    """(name, make_spec keywords, theta, X, y, Xs)"""
    out = []
    # (a) jitter-limited smooth 1-D tables: sorted uniform inputs, y = sin 3x
    for name, n, kind, eta, ls, sigma, m_rand, seed in (
        ("a_expquad_n300", 300, "ExpQuad", 4.5, 0.5, 1e-9, 240, 1),
        ("a_matern52_n1100", 1100, "Matern52", 3.0, 0.5, 1e-9, 300, 2),
        ("a_matern32_n1100", 1100, "Matern32", 2.0, 1.0, 1e-7, 300, 3),
        ("a_expquad_n2700", 2700, "ExpQuad", 2.5, 0.3, 1e-6, 4200 - 540, 4),
    ):
        rng = np.random.default_rng(seed)
        X = np.sort(rng.uniform(-2, 2, n))[:, None]
        y = np.sin(3 * X[:, 0])
        kw = dict(D=1, idx_cont=[0], kind=kind)
        spec = O.make_spec(**kw)
        out.append((name, kw, O.pack_theta(spec, [ls], eta, sigma), X, y, _points(X, rng, m_rand, -2.2, 2.2)))
    # (b) near-duplicate inputs: the second half repeats the first at scaled distance 1e-5 (Matern-3/2, r^2 expansion on the
    # interior tiles) -- and exact duplicates with Matern-1/2, whose gradient has dk/dr2 ~ 1/r at r = sqrt(1e-12)
    rng = np.random.default_rng(5)
    X0 = rng.standard_normal((512, 2))
    ls = np.array([1.0, 1.5])
    X = np.vstack([X0, X0 + 1e-5 * ls * rng.standard_normal((512, 2))])
    y = np.sin(X[:, 0] / ls[0]) + np.cos(X[:, 1] / ls[1]) + 1e-3 * rng.standard_normal(1024)
    kw = dict(D=2, idx_cont=[0, 1], kind="Matern32")
    out.append(("b_matern32_n1024", kw, O.pack_theta(O.make_spec(**kw), ls, 1.5, 1e-3), X, y, _points(X, rng, 200, -2.5, 2.5)))
    rng = np.random.default_rng(6)
    X0 = rng.standard_normal((150, 2))
    X = np.vstack([X0, X0])
    y = np.sin(X[:, 0]) + np.cos(X[:, 1]) + 1e-4 * rng.standard_normal(300)
    kw = dict(D=2, idx_cont=[0, 1], kind="Matern12")
    out.append(("b_matern12_dup_n300", kw, O.pack_theta(O.make_spec(**kw), [1.2, 0.8], 1.0, 1e-4), X, y,
                _points(X, rng, 150, -2.5, 2.5)))
    # (c) d = 6, ARD length scales over two orders of magnitude
    rng = np.random.default_rng(7)
    ls = np.geomspace(0.3, 30.0, 6)
    X = rng.standard_normal((1200, 6))
    y = np.sum(np.sin(X / ls), axis=1)
    kw = dict(D=6, idx_cont=list(range(6)), kind="ExpQuad")
    out.append(("c_ard_expquad_n1200", kw, O.pack_theta(O.make_spec(**kw), ls, 1.0, 1e-3), X, y, _points(X, rng, 260, -2.5, 2.5)))
    # (d) the control: the parity tests' own regime
    X, y, ls = O.synthetic_table(1000, 3, seed=8)
    kw = dict(D=3, idx_cont=[0, 1, 2], kind="Matern52")
    out.append(("d_control_matern52_n1000", kw, O.pack_theta(O.make_spec(**kw), ls, 1.0, 0.3), X, y,
                _points(X, np.random.default_rng(8), 200, -2.5, 2.5)))
    # composite: 2 continuous (1 linear) x 3-level categorical x 2 outputs, heteroskedastic noise, sigma = 1e-3
    rng = np.random.default_rng(9)
    n = 350
    Xc = np.sort(rng.uniform(-2, 2, (n, 2)), axis=0)
    cat = rng.integers(0, 3, n).astype(float)
    X1 = np.column_stack([Xc, cat])
    X = np.vstack([np.column_stack([X1, np.full(n, p)]) for p in range(2)])
    y = np.sin(2 * X[:, 0]) + X[:, 1] * (1 + X[:, 3]) + 0.3 * X[:, 2]
    kw = dict(D=4, idx_cont=[0, 1], idx_lin=[1], coreg=[(2, 3)], out_col=3, n_out=2, hetero_noise=True)
    spec = O.make_spec(**kw)
    theta = O.pack_theta(spec, [0.9, 1.4], 1.2, 1e-3, c=[0.2], tau=0.5, coreg=[(rng.standard_normal((3, 2)), [0.4, 0.7, 1.1])],
                         W_out=rng.standard_normal((2, 2)), kappa_out=[0.3, 0.6], W_noise=rng.standard_normal((2, 2)),
                         kappa_noise=[0.5, 0.9])
    near = X[::5].copy()
    near[:, 0] += 1e-3
    far = X[rng.integers(0, 2 * n, 120)].copy()
    far[:, :2] = rng.uniform(-2.2, 2.2, (120, 2))
    out.append(("composite_n700", kw, theta, X, y, np.vstack([near, far])))
    # two outputs on the SAME inputs (the Kronecker path, regression/icm.py: one N = 600 system per eigenvalue of the scaled
    # coregion matrix), checked against the reference of the stacked 1200 x 1200 system
    rng = np.random.default_rng(10)
    n = 600
    x = np.sort(rng.uniform(-2, 2, n))
    X = np.column_stack([np.tile(x, 2), np.repeat([0.0, 1.0], n)])
    y = np.concatenate([np.sin(3 * x), np.sin(3 * x) + 0.5 * np.cos(2 * x)])
    kw = dict(D=2, idx_cont=[0], out_col=1, n_out=2, hetero_noise=True)
    spec = O.make_spec(**kw)
    theta = O.pack_theta(spec, [0.5], 1.0, 1e-4, W_out=[[1.0, 0.3], [0.8, -0.2]], kappa_out=[0.1, 0.2],
                         W_noise=[[0.5, 0.1], [0.2, 0.4]], kappa_noise=[0.6, 0.9])
    Xs = np.column_stack([np.tile(np.concatenate([x[::5] + 1e-3, rng.uniform(-2.2, 2.2, 100)]), 2), np.repeat([0.0, 1.0], 220)])
    out.append(("kron_expquad_2x600", kw, theta, X, y, Xs))
    return out


def main():
    from threadpoolctl import threadpool_limits

    with threadpool_limits(limits=1, user_api="blas"):  # (one BLAS thread: the host errors come out the same bits everywhere)
        _main()


def _main():
    t0 = time.time()
    out = {}
    for name, kw, theta, X, y, Xs in cases():
        t = time.time()
        spec = O.make_spec(**kw)
        S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
        Lh = np.linalg.cholesky(S)
        margin = float(np.min(np.diag(Lh)) ** 2 / (EPS * np.max(np.diag(S))))
        assert margin >= 1e3, (name, margin)  # every case factors in LAPACK with margin
        ref = P.posterior(spec, theta, X, y, Xs, grad=True, sigma=S)
        host = P.host_float64(spec, theta, X, y, Xs, grad=True)
        rec = {"X": X, "y": y, "Xs": Xs, "theta": np.asarray(theta, float), "spec": np.array(json.dumps(kw)),
               "cond": np.array(np.linalg.cond(S)), "pivot_margin": np.array(margin)}
        for key in ("mean", "var", "var_noise", "nlml", "alpha", "grad"):
            r = np.asarray(ref[key], dtype=float)
            rec[key] = r
            d = np.asarray(host[key], float) - r
            rec[f"e64_{key}"] = np.array(np.linalg.norm(d) if key == "grad" else np.max(np.abs(d)))
        out.update({f"{name}/{k}": v for k, v in rec.items()})
        print(f"{name}: N={len(y)} M={len(Xs)} cond {float(rec['cond']):.2e} margin {margin:.1e}  "
              + "  ".join(f"e64_{k} {float(rec['e64_' + k]):.1e}" for k in ("mean", "var", "nlml", "alpha", "grad") if "e64_" + k in rec)
              + f"  ({time.time() - t:.1f} s)", flush=True)
    path = HERE / "conditioning_goldens.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes) in {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
