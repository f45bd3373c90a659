"""numpy reference for the gradient of the posterior mean with respect to the test point (``gmb_predict_grad``), built over
``oracle.gp_oracle``.  TEST INFRASTRUCTURE ONLY.

One term of the model is ``k(x*, x) = [eta^2 f(r^2) + tau sum_l (x*_l - c_l)(x_l - c_l)] F(x*, x)`` with F the product of the
coregion table entries, so with ``alpha = Sigma^-1 y``

    d mu / d x*_d = sum_n alpha_n F_mn [ eta^2 f'(r^2_mn) 2 (x*_d - x_nd) / ls_d^2 + tau (x_nd - c_d) 1{d linear} ]

``f' = oracle._stationary_dr2`` (it keeps ``sqrt(r^2 + 1e-12)``).  Additive models sum their terms (``oracle.additive_terms``);
periodic models are the stationary model on the warped features of ``tests/periodic_reference.py`` plus the chain rule through
``(sin, cos)(2 pi x / T)``.  Categorical columns and the output index get 0.

``fd_mean_grad`` is the independent check: Richardson-extrapolated central differences of ``cov_full(...) @ alpha``.
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O

import periodic_reference as PR


def _alpha(spec, theta, X, y):
    L, v = O.factorize(spec, theta, X, y, dist_mode="direct")
    return solve_triangular(L, v, lower=True, trans="T")


def _term_grad(spec, theta, X, Xs, alpha):
    """(M, D) gradient of ``K(Xs, X) @ alpha`` for ONE non-additive term."""
    p = O.unpack_theta(spec, theta)
    ic = spec["idx_cont"]
    ls = np.broadcast_to(np.asarray(p["ls"], float), (len(ic),))
    G = np.zeros(Xs.shape)
    F = O._coreg_factor(spec, p, Xs, X)
    Fa = alpha[None, :] * (1.0 if F is None else F)           # (M, N)
    diff = (Xs[:, None, ic] - X[None, :, ic]) / ls            # (M, N, d): u* - u
    S = p["eta"] ** 2 * O._stationary_dr2(spec["kind"], np.einsum("mnk,mnk->mn", diff, diff)) * Fa
    A = np.einsum("mn,mnk->mk", S, diff)
    for k, col in enumerate(ic):
        G[:, col] += 2.0 / ls[k] * A[:, k]
    if spec["idx_lin"]:
        il = spec["idx_lin"]
        B = Fa @ (X[:, il] - p["c"])
        for l, col in enumerate(il):
            G[:, col] += p["tau"] * B[:, l]
    return G


def _stationary_grad(spec, theta, X, Xs, alpha, block=1024):
    terms = O.additive_terms(spec, theta) if spec.get("additive") else [(spec, theta, None)]
    out = np.zeros(Xs.shape)
    for m0 in range(0, len(Xs), block):
        for sp, th, _ in terms:
            out[m0:m0 + block] += _term_grad(sp, np.asarray(th, float), X, Xs[m0:m0 + block], alpha)
    return out


def mean_grad(spec, theta, X, y, Xs, periodic=0, periods=None):
    """Analytic d mu / d x* at the rows of ``Xs``: (M, D)."""
    X, y, Xs, theta = np.asarray(X, float), np.asarray(y, float), np.asarray(Xs, float), np.asarray(theta, float)
    if not periodic:
        return _stationary_grad(spec, theta, X, Xs, _alpha(spec, theta, X, y))
    w = PR.Warped(spec, periodic, periods)
    wX, wXs, wth = w.X(X), w.X(Xs), w.theta(theta)
    Gw = _stationary_grad(w.spec, wth, wX, wXs, _alpha(w.spec, wth, wX, y))
    s = 2 * len(spec["idx_cont"])
    G = Gw[:, s:].copy()                                       # the model's own columns (linear terms land here)
    for d, col in enumerate(spec["idx_cont"]):                 # features (2d, 2d + 1) = (sin, cos)(2 pi x / T_d)
        om = 2.0 * np.pi / float(periods[d])
        G[:, col] += om * (Gw[:, 2 * d] * wXs[:, 2 * d + 1] - Gw[:, 2 * d + 1] * wXs[:, 2 * d])
    return G


def posterior_mean(spec, theta, X, y, periodic=0, periods=None):
    """``mu(Xs)`` as a closure over a fixed alpha (what the finite differences difference)."""
    X, y, theta = np.asarray(X, float), np.asarray(y, float), np.asarray(theta, float)
    if periodic:
        w = PR.Warped(spec, periodic, periods)
        wX, wth = w.X(X), w.theta(theta)
        alpha = _alpha(w.spec, wth, wX, y)
        return lambda Xs: O.cov_full(w.spec, wth, wX, w.X(Xs), dist_mode="direct").T @ alpha
    alpha = _alpha(spec, theta, X, y)
    return lambda Xs: O.cov_full(spec, theta, X, np.asarray(Xs, float), dist_mode="direct").T @ alpha


def fd_mean_grad(mu, Xs, cols, h=1e-3):
    """Richardson-extrapolated central differences (h and h / 2) of ``mu`` along the columns ``cols`` of ``Xs``: (M, D), zeros
    elsewhere."""
    Xs = np.asarray(Xs, float)
    G = np.zeros(Xs.shape)

    def central(col, step):
        E = np.zeros(Xs.shape)
        E[:, col] = step
        return (mu(Xs + E) - mu(Xs - E)) / (2.0 * step)

    for col in cols:
        G[:, col] = (4.0 * central(col, 0.5 * h) - central(col, h)) / 3.0
    return G
