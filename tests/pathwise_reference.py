"""numpy reference for the pathwise posterior draws (``gmb_paths_prepare`` / ``gmb_paths_eval`` / ``gmb_paths_eval_own``; DESIGN
§3.20), from the same ``(omega, phase, w, eps)`` the engine is handed:

    f_s(x) = phi(x)^T w_s + k(x, X) a_s,    a_s = Sigma^-1 (y - Phi(X) w_s - d o eps_s),    d^2 = sigma^2 + jitter,
    phi_f(x) = eta sqrt(2 / F) cos(omega_f^T u + b_f),    u = x / ls.

The kernel is ``oracle.gp_oracle``'s in direct-distance form (scaled differences, ``sqrt(r^2 + 1e-12)``), so a kinked kernel's
gradient at a coincident point is 0, as the engine's.  One stationary term over the continuous dimensions only.
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle import gp_oracle as O


def _pieces(spec, theta, dtype=np.float64):
    p = O.unpack_theta(spec, theta)
    ic = spec["idx_cont"]
    ls = np.broadcast_to(np.asarray(p["ls"], dtype), (len(ic),)) if not spec["ard"] else np.asarray(p["ls"], dtype)
    return p, ic, ls


def features(spec, theta, omega, phase, X, dtype=np.float64):
    """Phi(X): (len(X), F)"""
    p, ic, ls = _pieces(spec, theta, dtype)
    U = np.asarray(X, dtype)[:, ic] / ls
    F = len(phase)
    return dtype(p["eta"]) * np.sqrt(dtype(2.0) / dtype(F)) * np.cos(U @ np.asarray(omega, dtype).T + np.asarray(phase, dtype))


def scaled_differences(spec, theta, Xs, X, dtype=np.float64):
    """u*_m - u_n per continuous column: (M, N, Dc)"""
    _, ic, ls = _pieces(spec, theta, dtype)
    return np.asarray(Xs, dtype)[:, None, ic] / ls - np.asarray(X, dtype)[None, :, ic] / ls


def cross_kernel(spec, theta, Xs, X, dtype=np.float64):
    """K(Xs, X) from direct scaled differences: (M, N)"""
    p, _, _ = _pieces(spec, theta, dtype)
    d = scaled_differences(spec, theta, Xs, X, dtype)
    return dtype(p["eta"]) ** 2 * O.stationary_from_r2(spec["kind"], np.einsum("mnk,mnk->mn", d, d))


def coefficients(spec, theta, X, y, omega, phase, w, eps):
    """A = Sigma^-1 R, (N, S): R = y - Phi(X) w^T - d eps^T with d^2 the diagonal the covariance build adds to K"""
    p = O.unpack_theta(spec, theta)
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    d = np.sqrt(p["sigma"] ** 2 + spec["jitter"])
    R = np.asarray(y, float)[:, None] - features(spec, theta, omega, phase, X) @ np.asarray(w, float).T - d * np.asarray(eps, float).T
    return cho_solve(cho_factor(S, lower=True), R)


def posterior_mean(spec, theta, X, y, Xs):
    """k(x*, X) Sigma^-1 y with the direct-distance kernel: what the mean of an antithetic pair equals exactly"""
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    return cross_kernel(spec, theta, Xs, X) @ cho_solve(cho_factor(S, lower=True), np.asarray(y, float))


def all_draws(spec, theta, X, Xs, omega, phase, w, A, dtype=np.float64):
    """every draw at every point: (S, M)"""
    prior = features(spec, theta, omega, phase, Xs, dtype) @ np.asarray(w, dtype).T
    return (prior + cross_kernel(spec, theta, Xs, X, dtype) @ np.asarray(A, dtype)).T


def own_draws(spec, theta, X, Xs, draw, omega, phase, w, A, grad=True, dtype=np.float64):
    """point m on draw draw[m]: ``(val (M,), grad (M, D))`` -- the gradient with respect to the point, zero in the columns that
    are no continuous dimension (``None`` with ``grad=False``)"""
    p, ic, ls = _pieces(spec, theta, dtype)
    draw = np.asarray(draw, int)
    Am = np.asarray(A, dtype)[:, draw].T  # (M, N)
    wm = np.asarray(w, dtype)[draw]       # (M, F)
    Fn = len(phase)
    amp = dtype(p["eta"]) * np.sqrt(dtype(2.0) / dtype(Fn))
    U = np.asarray(Xs, dtype)[:, ic] / ls
    arg = U @ np.asarray(omega, dtype).T + np.asarray(phase, dtype)
    d = scaled_differences(spec, theta, Xs, X, dtype)
    r2 = np.einsum("mnk,mnk->mn", d, d)
    val = amp * np.sum(wm * np.cos(arg), axis=1) + dtype(p["eta"]) ** 2 * np.sum(Am * O.stationary_from_r2(spec["kind"], r2), axis=1)
    if not grad:
        return val, None
    g_data = 2.0 * p["eta"] ** 2 * np.einsum("mn,mnk->mk", Am * O._stationary_dr2(spec["kind"], r2), d) / ls
    g_prior = -amp * ((wm * np.sin(arg)) @ np.asarray(omega, dtype)) / ls
    G = np.zeros((len(Xs), spec["D"]), dtype)
    G[:, ic] = g_data + g_prior
    return val, G
