"""numpy reference for ``gmb_predict_with_grad``: posterior mean and variance with their gradients with respect to the test
point, built over ``oracle.gp_oracle``.  TEST INFRASTRUCTURE ONLY.

With ``V = K(X*, X) L^-T`` and ``W = K(X*, X) Sigma^-1 = V L^-1`` (row m = w_m)

    sigma^2(x*)        = k(x*, x*) [+ noise] - |v|^2
    d sigma^2 / d x*_d = d k(x*, x*) / d x*_d - 2 sum_n W_mn d k(x*_m, x_n) / d x*_d

``d k(x*, x_n) / d x*_d`` is the quantity of ``tests/grad_reference.py`` (same ``f' = oracle._stationary_dr2``, same
``sqrt(r^2 + 1e-12)``), weighted by ``W_mn`` instead of ``alpha_n``.  The prior term is 0 for the stationary and periodic forms
and ``2 tau (x*_l - c_l) F_mm`` for a linear dimension l (F_mm: the product of the coregion table entries at the point's own
categories); additive models sum their terms; the noise diagonal has no gradient.  Periodic models are the stationary model
on the warped features of ``tests/periodic_reference.py`` plus the chain rule through ``(sin, cos)(2 pi x / T)``.

``mean_var_grad`` is float64 throughout (the mean part IS ``grad_reference.mean_grad``); ``mean_var_grad_precise`` repeats the
computation in ``np.longdouble`` on the factor of ``tests/precise_reference.py``; ``fd_var_grad`` takes Richardson-extrapolated
central differences of a variance function.
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O

import grad_reference as GR
import periodic_reference as PR
import precise_reference as XR


def _term_weighted_grad(spec, theta, X, Xs, Wt, dtype=float):
    """(M, D): ``sum_n Wt_mn d k(x*_m, x_n) / d x*`` for ONE non-additive term and weights ``Wt`` (M, N)."""
    p = O.unpack_theta(spec, theta)
    ic = spec["idx_cont"]
    ls = np.broadcast_to(np.asarray(p["ls"], float), (len(ic),)).astype(dtype)
    G = np.zeros(Xs.shape, dtype=dtype)
    F = O._coreg_factor(spec, p, Xs, X)
    Fw = Wt * (1.0 if F is None else F)                            # (M, N)
    diff = (Xs[:, None, ic].astype(dtype) - X[None, :, ic].astype(dtype)) / ls
    S = dtype(p["eta"]) ** 2 * O._stationary_dr2(spec["kind"], np.einsum("mnk,mnk->mn", diff, diff)) * Fw
    A = np.einsum("mn,mnk->mk", S, diff)
    for k, col in enumerate(ic):
        G[:, col] += 2.0 / ls[k] * A[:, k]
    if spec["idx_lin"]:
        il = spec["idx_lin"]
        B = Fw @ (X[:, il] - p["c"]).astype(dtype)
        for l, col in enumerate(il):
            G[:, col] += dtype(p["tau"]) * B[:, l]
    return G


def _term_prior_grad(spec, theta, Xs, dtype=float):
    """(M, D): ``d k(x*, x*) / d x*`` of one non-additive term -- only its linear dimensions have one."""
    G = np.zeros(Xs.shape, dtype=dtype)
    if not spec["idx_lin"]:
        return G
    p = O.unpack_theta(spec, theta)
    Fmm = np.ones(len(Xs))
    tables = [(col, O.coregion_B(W, kap)) for (col, _), (W, kap) in zip(spec["coreg"], p["coreg"])]
    if spec["out_col"] >= 0:
        tables.append((spec["out_col"], O.coregion_B(p["W_out"], p["kappa_out"])))
    for col, B in tables:
        Fmm = Fmm * np.diag(B)[Xs[:, col].astype(np.int32)]
    for l, col in enumerate(spec["idx_lin"]):
        G[:, col] += 2.0 * dtype(p["tau"]) * (Xs[:, col] - p["c"][l]).astype(dtype) * Fmm
    return G


def _var_grad(spec, theta, X, Xs, W, dtype=float, block=1024):
    terms = O.additive_terms(spec, theta) if spec.get("additive") else [(spec, theta, None)]
    out = np.zeros(Xs.shape, dtype=dtype)
    for m0 in range(0, len(Xs), block):
        sl = slice(m0, m0 + block)
        for sp, th, _ in terms:
            th = np.asarray(th, float)
            out[sl] += _term_prior_grad(sp, th, Xs[sl], dtype) - 2.0 * _term_weighted_grad(sp, th, X, Xs[sl], W[sl], dtype)
    return out


def _mean_grad(spec, theta, X, Xs, alpha, dtype, block=1024):
    terms = O.additive_terms(spec, theta) if spec.get("additive") else [(spec, theta, None)]
    out = np.zeros(Xs.shape, dtype=dtype)
    for m0 in range(0, len(Xs), block):
        sl = slice(m0, m0 + block)
        for sp, th, _ in terms:
            out[sl] += _term_weighted_grad(sp, np.asarray(th, float), X, Xs[sl], alpha[None, :], dtype)
    return out


def _unwarp(spec, periods, Gw, wXs):
    """Gradient in the model's columns from the warped model's (features first): the chain rule through (sin, cos)."""
    s = 2 * len(spec["idx_cont"])
    G = Gw[:, s:].copy()
    for d, col in enumerate(spec["idx_cont"]):
        om = 2.0 * np.pi / float(periods[d])
        G[:, col] += om * (Gw[:, 2 * d] * wXs[:, 2 * d + 1] - Gw[:, 2 * d + 1] * wXs[:, 2 * d])
    return G


def _as_oracle_model(spec, theta, X, Xs, periodic, periods):
    X, Xs, theta = np.asarray(X, float), np.asarray(Xs, float), np.asarray(theta, float)
    if not periodic:
        return spec, theta, X, Xs
    w = PR.Warped(spec, periodic, periods)
    return w.spec, w.theta(theta), w.X(X), w.X(Xs)


def mean_var_grad(spec, theta, X, y, Xs, periodic=0, periods=None, with_noise=True):
    """``(mean, var, dmean, dvar)`` at the rows of ``Xs`` in float64: (M,), (M,), (M, D), (M, D)."""
    y = np.asarray(y, float)
    dmean = GR.mean_grad(spec, theta, X, y, Xs, periodic=periodic, periods=periods)
    sp, th, wX, wXs = _as_oracle_model(spec, theta, X, Xs, periodic, periods)
    L, v = O.factorize(sp, th, wX, y, dist_mode="direct")
    Kxs = O.cov_full(sp, th, wX, wXs, dist_mode="direct")                          # (N, M)
    A = solve_triangular(L, Kxs, lower=True, check_finite=False)                   # V^T
    W = solve_triangular(L, A, lower=True, trans="T", check_finite=False).T        # (M, N)
    mean = A.T @ v
    var = O.cov_diag(sp, th, wXs) - np.sum(A * A, axis=0)
    if with_noise:
        var = var + O.noise_diag(sp, th, wXs)
    Gw = _var_grad(sp, th, wX, wXs, W)
    dvar = _unwarp(spec, periods, Gw, wXs) if periodic else Gw
    return mean, var, dmean, dvar


def mean_var_grad_precise(spec, theta, X, y, Xs, periodic=0, periods=None):
    """``(dmean, dvar)`` in ``np.longdouble`` from the float64 Sigma and K(X, X*) of the oracle (taken as exact, as
    ``precise_reference.posterior`` does)."""
    LD = XR.LD
    sp, th, wX, wXs = _as_oracle_model(spec, theta, X, Xs, periodic, periods)
    post = XR.posterior(sp, th, wX, np.asarray(y, float))
    L, alpha = post["L"], post["alpha"]
    Kxs = O.cov_full(sp, th, wX, wXs, dist_mode="direct")
    W = XR.solve_upper_t(L, XR.solve_lower(L, Kxs)).T                               # (M, N) longdouble
    Gm = _mean_grad(sp, th, wX, wXs, alpha, LD)
    Gv = _var_grad(sp, th, wX, wXs, W, LD)
    if periodic:
        wl = wXs.astype(LD)
        return _unwarp(spec, periods, Gm, wl), _unwarp(spec, periods, Gv, wl)
    return Gm, Gv


def posterior_var(spec, theta, X, y, periodic=0, periods=None):
    """The oracle's noise-free predictive variance as a closure over a fixed factor (what the finite differences difference)."""
    sp, th, wX, _ = _as_oracle_model(spec, theta, X, X[:1], periodic, periods)
    L, _ = O.factorize(sp, th, wX, np.asarray(y, float), dist_mode="direct")
    w = PR.Warped(spec, periodic, periods) if periodic else None

    def var(Xs):
        Xs = np.asarray(Xs, float)
        P = w.X(Xs) if w else Xs
        A = solve_triangular(L, O.cov_full(sp, th, wX, P, dist_mode="direct"), lower=True, check_finite=False)
        return O.cov_diag(sp, th, P) - np.sum(A * A, axis=0)

    return var


fd_var_grad = GR.fd_mean_grad  # Richardson-extrapolated central differences (h, h / 2) of any f(Xs) -> (M,)
