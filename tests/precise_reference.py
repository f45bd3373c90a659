"""Extended-precision reference of the GP solves (TEST INFRASTRUCTURE, CPU only).

The float64 oracle (oracle/gp_oracle.py) makes the same rounding errors as any backward-stable float64 computation: on an
ill-conditioned Sigma its alpha, posterior mean and Sigma^-1 are off by ~cond(Sigma) eps, and a kernel that is a hundred times
worse can still agree with it to the parity tests' bars.  This module takes the float64 Sigma, K(X, X*) and k** the oracle
builds (the problem, taken as exact) and solves it in ``np.longdouble`` (x87 80-bit: 64-bit mantissa, eps ~ 1.1e-19), so that
the engine and the float64 host can both be measured against something ~2000 times more accurate than either
(tests/test_precise_reference.py checks that against mpmath).

The Cholesky is blocked and right-looking: the trailing updates are longdouble ``@`` products (numpy's own loops -- BLAS has
no extended type), only the 64-wide diagonal blocks and panel solves run column by column.
"""
import numpy as np

from oracle import gp_oracle as O

LD = np.longdouble
NB = 64  # block width of the Cholesky and of the triangular solves


def _chol_unblocked(A):
    """In place on the lower triangle of a small longdouble block; returns L (zeros above the diagonal)."""
    n = A.shape[0]
    for j in range(n):
        d = A[j, j] - A[j, :j] @ A[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"longdouble Cholesky: pivot {j} = {float(d):.3e}")
        A[j, j] = np.sqrt(d)
        if j + 1 < n:
            A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    return np.tril(A)


def cholesky(S):
    """Lower Cholesky factor of the symmetric positive definite ``S`` (any float dtype), in longdouble."""
    A = np.array(S, dtype=LD)
    n = A.shape[0]
    for k in range(0, n, NB):
        e = min(k + NB, n)
        A[k:e, k:e] = _chol_unblocked(A[k:e, k:e])
        if e < n:
            # panel: L21 = A21 L11^-T, i.e. L11 L21^T = A21^T
            A[e:, k:e] = solve_lower(A[k:e, k:e], A[e:, k:e].T).T
            P = A[e:, k:e]
            A[e:, e:] -= P @ P.T
    return np.tril(A)


def solve_lower(L, B):
    """L^-1 B for lower-triangular longdouble L (B a vector or a matrix), blocked forward substitution."""
    X = np.array(B, dtype=LD)
    vec = X.ndim == 1
    if vec:
        X = X[:, None]
    n = L.shape[0]
    for k in range(0, n, NB):
        e = min(k + NB, n)
        if k:
            X[k:e] -= L[k:e, :k] @ X[:k]
        for j in range(k, e):
            if j > k:
                X[j] -= L[j, k:j] @ X[k:j]
            X[j] /= L[j, j]
    return X[:, 0] if vec else X


def solve_upper_t(L, B):
    """L^-T B for lower-triangular longdouble L (B a vector or a matrix), blocked backward substitution."""
    X = np.array(B, dtype=LD)
    vec = X.ndim == 1
    if vec:
        X = X[:, None]
    n = L.shape[0]
    U = L.T
    for e in range(n, 0, -NB):
        k = max(e - NB, 0)
        if e < n:
            X[k:e] -= U[k:e, e:] @ X[e:]
        for j in range(e - 1, k - 1, -1):
            if j + 1 < e:
                X[j] -= U[j, j + 1:e] @ X[j + 1:e]
            X[j] /= U[j, j]
    return X[:, 0] if vec else X


def posterior(spec, theta, X, y, Xs=None, grad=False, sigma=None):
    """The GP quantities of ``(spec, theta, X, y)`` in longdouble from the oracle's float64 Sigma (direct distances).

    Returns a dict: ``L`` (longdouble), ``v = L^-1 y``, ``logdet``, ``nlml``, ``alpha = Sigma^-1 y``; with ``Xs`` the posterior
    ``mean``, ``var`` (noiseless) and ``var_noise`` (pm.gp.Marginal.predict with and without pred_noise) from K(X, X*) and k**
    of the oracle; with ``grad`` also ``Sinv`` and the NLML gradient ``grad`` (the oracle's chain rule, ``O.grad_given_M``, on
    M = 1/2 (Sigma^-1 - alpha alpha^T) rounded to float64 once).  ``sigma`` replaces the oracle's Sigma (the same float64
    matrix built elsewhere)."""
    X = np.asarray(X, float)
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct") if sigma is None else np.asarray(sigma, float)
    N = S.shape[0]
    L = cholesky(S)
    v = solve_lower(L, np.asarray(y, float))
    logdet = 2 * np.sum(np.log(np.diag(L)))
    nlml = LD(0.5) * N * np.log(LD(2) * LD(np.pi)) + logdet / 2 + (v @ v) / 2
    alpha = solve_upper_t(L, v)
    out = {"L": L, "v": v, "logdet": logdet, "nlml": nlml, "alpha": alpha}
    if Xs is not None:
        Xs = np.asarray(Xs, float)
        Kxs = O.cov_full(spec, theta, X, Xs, dist_mode="direct")
        A = solve_lower(L, Kxs)
        kss = O.cov_diag(spec, theta, Xs).astype(LD)
        out["mean"] = Kxs.astype(LD).T @ alpha
        out["var"] = kss - np.sum(A * A, axis=0)
        out["var_noise"] = out["var"] + O.noise_diag(spec, theta, Xs).astype(LD)
    if grad:
        Linv = solve_lower(L, np.eye(N))
        Sinv = Linv.T @ Linv
        out["Sinv"] = Sinv
        M = ((Sinv - np.outer(alpha, alpha)) / 2).astype(float)
        out["grad"] = O.grad_given_M(spec, theta, X, M, dist_mode="direct")
    return out


def host_float64(spec, theta, X, y, Xs=None, grad=False):
    """The same quantities by the float64 host path a backward-stable computation takes: LAPACK potrf, triangular solves
    (alpha by the backward solve, the mean as (L^-1 K*)^T v like pm.gp.Marginal.predict) and the oracle's gradient with
    ``inverse="trsm"``."""
    from scipy.linalg import cho_factor, solve_triangular

    X = np.asarray(X, float)
    y = np.asarray(y, float)
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    L = np.tril(cho_factor(S, lower=True, check_finite=False)[0])
    v = solve_triangular(L, y, lower=True, check_finite=False)
    out = {"nlml": 0.5 * len(y) * np.log(2 * np.pi) + np.sum(np.log(np.diag(L))) + 0.5 * float(v @ v),
           "alpha": solve_triangular(L, v, lower=True, trans="T", check_finite=False)}
    if Xs is not None:
        Kxs = O.cov_full(spec, theta, X, np.asarray(Xs, float), dist_mode="direct")
        A = solve_triangular(L, Kxs, lower=True, check_finite=False)
        out["mean"] = A.T @ v
        out["var"] = O.cov_diag(spec, theta, Xs) - np.sum(A * A, axis=0)
        out["var_noise"] = out["var"] + O.noise_diag(spec, theta, Xs)
    if grad:
        # (this gradient forms alpha = L^-T (L^-1 y) through the explicit L^-1, unlike out["alpha"] above: e64_grad is the error
        # of the host path the parity tests pin, which includes that of the explicit-inverse alpha in its a a^T term)
        out["grad"] = O.nlml_and_grad(spec, theta, X, y, dist_mode="direct", inverse="trsm")[1]
    return out
