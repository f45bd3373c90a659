"""numpy reference for ``gmb_predict_batches``: the joint posterior of batches of q test points and its derivative with respect
to the batch's own coordinates, built over ``oracle.gp_oracle`` from the pieces of ``tests/var_grad_reference.py``.  TEST
INFRASTRUCTURE ONLY.

Batch b = rows ``[b q, (b + 1) q)`` of ``Xs``.  With ``V = K(X*, X) L^-T`` and ``W = V L^-1`` (row l = w_l = Sigma^-1 k(X, x_l))

    C_b                 = K(P_b, P_b) - V_b V_b^T + jitter I
    d C_b[j, l] / d x_j = d_1 k(x_j, x_l) - sum_n W_ln d k(x_j, x_n) / d x_j              (l != j)
    d C_b[j, j] / d x_j = d k(x_j, x_j) / d x_j - 2 sum_n W_jn d k(x_j, x_n) / d x_j

* the cross term is ``var_grad_reference._term_weighted_grad`` with every row's weights set to ``w_l``;
* the within-batch prior term ``d_1 k(x_j, x_l)`` is the same function with the batch itself as the "training" points and one-hot
  weights; on the diagonal it is ``var_grad_reference._term_prior_grad``;
* periodic models go through the warp of ``tests/periodic_reference.py`` and the chain rule, as in that file.

``joint_cov_precise`` forms ``C`` of ONE batch in ``np.longdouble`` on the factor of ``tests/precise_reference.py``: what the
finite differences of tests/test_predict_batches_cpu.py difference.
"""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp_oracle as O

import grad_reference as GR
import precise_reference as XR
import var_grad_reference as VG


def _terms(sp, th):
    return O.additive_terms(sp, th) if sp.get("additive") else [(sp, th, None)]


def batch_cov_grad(sp, th, wX, wXs, W, q):
    """``(B, q, q, Dw)`` in the (possibly warped) oracle model's columns: ``d C_b[j, l] / d x_j`` from ``W`` (M, N)."""
    M, Dw = wXs.shape
    B = M // q
    G = np.zeros((B, q, q, Dw))
    Wb = W.reshape(B, q, -1)
    eye = np.eye(q)
    for t_sp, t_th, _ in _terms(sp, th):
        t_th = np.asarray(t_th, float)
        self_prior = VG._term_prior_grad(t_sp, t_th, wXs).reshape(B, q, Dw)
        for l in range(q):
            Wt = np.repeat(Wb[:, l, :], q, axis=0)                                   # row (b, j) weighted by w_(b, l)
            cross = VG._term_weighted_grad(t_sp, t_th, wX, wXs, Wt).reshape(B, q, Dw)
            for b in range(B):
                P = wXs[b * q:(b + 1) * q]
                pair = VG._term_weighted_grad(t_sp, t_th, P, P, np.tile(eye[l], (q, 1)))  # row j: d_1 k(x_j, x_l)
                G[b, :, l] += pair - cross[b]
                G[b, l, l] += self_prior[b, l] - 2.0 * cross[b, l] - (pair[l] - cross[b, l])
    return G


def batch_posterior(spec, theta, X, y, Xs, q, jitter=0.0, periodic=0, periods=None, grad=True):
    """``(mean (B, q), cov (B, q, q), dmean (B, q, D), dcov (B, q, q, D))`` in float64 (``grad=False``: the first two)."""
    X, y, Xs, theta = np.asarray(X, float), np.asarray(y, float), np.asarray(Xs, float), np.asarray(theta, float)
    M, D = Xs.shape
    B = M // q
    assert B * q == M
    sp, th, wX, wXs = VG._as_oracle_model(spec, theta, X, Xs, periodic, periods)
    L, v = O.factorize(sp, th, wX, y, dist_mode="direct")
    Kxs = O.cov_full(sp, th, wX, wXs, dist_mode="direct")                            # (N, M)
    A = solve_triangular(L, Kxs, lower=True, check_finite=False)                     # V^T
    mean = (A.T @ v).reshape(B, q)
    cov = np.empty((B, q, q))
    for b in range(B):
        sl = slice(b * q, (b + 1) * q)
        Kpp = O.cov_full(sp, th, wXs[sl], wXs[sl], dist_mode="direct")
        np.fill_diagonal(Kpp, O.cov_diag(sp, th, wXs[sl]))  # (the prediction's k**: a stationary diagonal is exactly eta^2)
        C = Kpp - A[:, sl].T @ A[:, sl]
        cov[b] = 0.5 * (C + C.T) + jitter * np.eye(q)
    if not grad:
        return mean, cov
    W = solve_triangular(L, A, lower=True, trans="T", check_finite=False).T          # (M, N)
    dmean = GR.mean_grad(spec, theta, X, y, Xs, periodic=periodic, periods=periods).reshape(B, q, D)
    Gw = batch_cov_grad(sp, th, wX, wXs, W, q)
    if periodic:
        dcov = np.stack([VG._unwarp(spec, periods, Gw[:, :, l].reshape(M, -1), wXs).reshape(B, q, D) for l in range(q)], axis=2)
    else:
        dcov = Gw
    return mean, cov, dmean, dcov


def joint_cov_precise(spec, theta, X, y, periodic=0, periods=None):
    """The noise-free joint covariance of ONE batch as a closure over a fixed longdouble factor: ``C(P) -> (q, q)`` longdouble."""
    X, y, theta = np.asarray(X, float), np.asarray(y, float), np.asarray(theta, float)
    sp, th, wX, _ = VG._as_oracle_model(spec, theta, X, X[:1], periodic, periods)
    L = XR.posterior(sp, th, wX, y)["L"]

    def cov(P):
        P = np.asarray(P, float)
        wP = VG._as_oracle_model(spec, theta, X, P, periodic, periods)[3]
        A = XR.solve_lower(L, O.cov_full(sp, th, wX, wP, dist_mode="direct"))
        Kpp = O.cov_full(sp, th, wP, wP, dist_mode="direct")
        np.fill_diagonal(Kpp, O.cov_diag(sp, th, wP))
        return Kpp.astype(XR.LD) - A.T @ A

    return cov


def fd_cov_grad(cov, P, cols, h=1e-4):
    """Richardson-extrapolated central differences (h, h / 2) of ``cov(P)[j, l]`` with respect to ``P[j, cols]``: (q, q, D)."""
    P = np.asarray(P, float)
    q, D = P.shape
    out = np.zeros((q, q, D), dtype=XR.LD)

    def central(j, c, step):
        up, dn = P.copy(), P.copy()
        up[j, c] += step
        dn[j, c] -= step
        return (cov(up)[j] - cov(dn)[j]) / (2.0 * XR.LD(step))

    for j in range(q):
        for c in cols:
            out[j, :, c] = (4.0 * central(j, c, h / 2) - central(j, c, h)) / 3.0
    return out


# ---- a stand-in engine for the front end's CPU tests ----------------------------------------------------------------------------
def use_batch_oracle(monkeypatch):
    """``gumbi_amd.Engine`` replaced by a numpy stand-in with ``predict_batches`` (the front end's tests without a device); its
    class-level ``calls`` logs ``(B, q, grad)`` of every call."""
    from gumbi_amd.regression import hip_gp, icm
    from oracle_engine import OracleEngine

    class BatchOracleEngine(OracleEngine):
        calls = []

        def predict_batches(self, Xs, q, jitter=1e-6, grad=True):
            if not self._factored:
                raise ValueError("no valid factorisation")
            Xs = np.asarray(Xs, float)
            BatchOracleEngine.calls.append((len(Xs) // q, q, bool(grad)))
            return batch_posterior(self.spec, self.theta, self.X, self.y, Xs, q, jitter=jitter, grad=grad)

    monkeypatch.setattr(hip_gp, "Engine", BatchOracleEngine)
    monkeypatch.setattr(icm, "Engine", BatchOracleEngine)
    return BatchOracleEngine
