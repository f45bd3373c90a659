"""numpy reference for the posterior of the slope ``d f / d x*`` (``gmb_predict_slope``), built on ``grad_reference``'s term
machinery over ``oracle.gp_oracle``.  TEST INFRASTRUCTURE ONLY.

One term of the model is ``k(x*, x) = [eta^2 f(r^2) + tau sum_l (x*_l - c_l)(x_l - c_l)] F(x*, x)``.  The derivative of the latent
GP with respect to the test point is a GP with, per test point (no noise, no jitter),

    b_d[n]   = d k_S(x*, x_n) / d x*_d = sum_t F_mn [ eta^2 f'(r^2) 2 (x*_d - x_nd) / ls_d^2 + tau (x_nd - c_d) 1{d linear} ]
    E[g]     = B alpha,                       alpha = Sigma^-1 y                       (grad_reference.mean_grad)
    Cov[g]   = P - B Sigma^-1 B^T
    P_de     = delta_de sum_t F_t(x*, x*) [ -2 eta_t^2 f'_t(0) / ls_d^2 + tau_t 1{d linear in t} ]

``f' = oracle._stationary_dr2`` (it keeps ``sqrt(r^2 + 1e-12)``).  Periodic models are the stationary model on the warped features
of ``tests/periodic_reference.py`` pushed through the Jacobian J of ``x -> (sin, cos)(2 pi x / T)``: ``B = J B_w``,
``P = J P_w J^T``.  A selection of an additive model's terms sums the selected terms' B and P against the WHOLE model's factor.

``problem(name)`` defines the shapes the CPU and GPU tests share; ``fd_slope_cov`` is the independent check: Richardson central
differences of the oracle's joint posterior covariance.
"""
import functools

import numpy as np

import components_reference as CR
import leave_out_reference as LR
import periodic_reference as PR
from oracle import gp_oracle as O

NON_DIFFERENTIABLE = (O.KINDS["Matern12"], O.KINDS["Exponential"])


# ---- one stationary term --------------------------------------------------------------------------------------------------------
def term_B(spec, theta, X, Xs):
    """(M, D, N): ``d k(x*_m, x_n) / d x*_d`` of ONE non-additive term -- ``grad_reference._term_grad`` before its sum over n."""
    p = O.unpack_theta(spec, theta)
    ic = spec["idx_cont"]
    ls = np.broadcast_to(np.asarray(p["ls"], float), (len(ic),))
    F = O._coreg_factor(spec, p, Xs, X)
    F = np.ones((len(Xs), len(X))) if F is None else F
    diff = (Xs[:, None, ic] - X[None, :, ic]) / ls            # (M, N, d): u* - u
    S = p["eta"] ** 2 * O._stationary_dr2(spec["kind"], np.einsum("mnk,mnk->mn", diff, diff)) * F
    B = np.zeros((len(Xs), Xs.shape[1], len(X)))
    for k, col in enumerate(ic):
        B[:, col, :] += 2.0 / ls[k] * S * diff[:, :, k]
    for l, col in enumerate(spec["idx_lin"]):
        B[:, col, :] += p["tau"] * F * (X[:, col] - p["c"][l])[None, :]
    return B


def self_factor(spec, p, Xs):
    """(M,): the product of the coregion table entries at each point's own categories."""
    F = np.ones(len(Xs))
    tables = [(col, O.coregion_B(W, kap)) for (col, _), (W, kap) in zip(spec["coreg"], p["coreg"])]
    if spec["out_col"] >= 0:
        tables.append((spec["out_col"], O.coregion_B(p["W_out"], p["kappa_out"])))
    for col, Bt in tables:
        c = Xs[:, col].astype(np.int32)
        F = F * Bt[c, c]
    return F


def dr2_at_zero(kind):
    """``f'(0)`` as the code has it, the 1e-12 under the root included."""
    return float(O._stationary_dr2(kind, np.zeros(1))[0])


def term_P(spec, theta, Xs):
    """(M, D): the diagonal of the prior curvature of ONE non-additive term (P is diagonal)."""
    p = O.unpack_theta(spec, theta)
    ic = spec["idx_cont"]
    ls = np.broadcast_to(np.asarray(p["ls"], float), (len(ic),))
    F = self_factor(spec, p, Xs)
    P = np.zeros(Xs.shape)
    f0 = -2.0 * p["eta"] ** 2 * dr2_at_zero(spec["kind"])
    for k, col in enumerate(ic):
        P[:, col] += F * f0 / ls[k] ** 2
    for col in spec["idx_lin"]:
        P[:, col] += F * p["tau"]
    return P


def _selected(spec, theta, terms):
    parts = CR.term_list(spec, theta)
    return parts if terms is None else [parts[t] for t in CR.as_indices(terms, len(parts))]


def _stationary_B_P(spec, theta, X, Xs, terms):
    sel = _selected(spec, theta, terms)
    B = sum(term_B(sp, th, X, Xs) for sp, th in sel)
    Pd = sum(term_P(sp, th, Xs) for sp, th in sel)
    P = np.zeros((len(Xs), Xs.shape[1], Xs.shape[1]))
    idx = np.arange(Xs.shape[1])
    P[:, idx, idx] = Pd
    return B, P


# ---- the model: stationary, or warped --------------------------------------------------------------------------------------------
class Model:
    """What the reference needs of one problem: the spec / theta / points the oracle sees, and the Jacobian back to the model's
    own columns (the identity for a stationary model)."""

    def __init__(self, spec, theta, X, periodic=0, periods=None):
        self.D = np.asarray(X).shape[1]
        self.periodic = periodic
        if periodic:
            self.w = PR.Warped(spec, periodic, periods)
            self.spec, self.theta, self.X = self.w.spec, self.w.theta(np.asarray(theta, float)), self.w.X(X)
            self.om = 2.0 * np.pi / np.asarray(periods, float)
            self.cont = list(spec["idx_cont"])
        else:
            self.spec, self.theta, self.X = spec, np.asarray(theta, float), np.asarray(X, float)

    def pts(self, Xs):
        return self.w.X(Xs) if self.periodic else np.asarray(Xs, float)

    def jacobian(self, wXs):
        """(M, D, D_w) or None: d (oracle's columns) / d (model's columns) at the points."""
        if not self.periodic:
            return None
        s = 2 * len(self.cont)
        J = np.zeros((len(wXs), self.D, self.D + s))
        J[:, np.arange(self.D), s + np.arange(self.D)] = 1.0
        for d, col in enumerate(self.cont):  # features (2d, 2d + 1) = (sin, cos)(2 pi x / T_d)
            J[:, col, 2 * d] = self.om[d] * wXs[:, 2 * d + 1]
            J[:, col, 2 * d + 1] = -self.om[d] * wXs[:, 2 * d]
        return J

    def B_P(self, Xs, terms=None):
        """``(B (M, D, N), P (M, D, D))`` in the model's own columns."""
        wXs = self.pts(Xs)
        B, P = _stationary_B_P(self.spec, self.theta, self.X, wXs, terms)
        J = self.jacobian(wXs)
        if J is None:
            return B, P
        return np.einsum("mdw,mwn->mdn", J, B), np.einsum("mdw,mwv,mev->mde", J, P, J)

    def factor(self, y):
        L = O.cholesky_lower(O.sigma_matrix(self.spec, self.theta, self.X, dist_mode="direct"))
        return L, O.solve_lower(L, np.asarray(y, float))

    def joint_cov(self, y_unused, Xs, L):
        """The joint posterior covariance of the latent function at ``Xs`` (no noise, no jitter): what ``fd_slope_cov`` differences."""
        wXs = self.pts(Xs)
        V = O.solve_lower(L, O.cov_full(self.spec, self.theta, self.X, wXs, dist_mode="direct"))
        return O.cov_full(self.spec, self.theta, wXs, None, dist_mode="direct") - V.T @ V


def posterior(spec, theta, X, y, Xs, terms=None, periodic=0, periods=None, block=512):
    """``(dmean (M, D), dvar (M, D), dcov (M, D, D))``: the closed form above."""
    Xs = np.asarray(Xs, float)
    mdl = Model(spec, theta, X, periodic, periods)
    L, v = mdl.factor(y)
    M, D = Xs.shape
    dmean, dcov = np.empty((M, D)), np.empty((M, D, D))
    for m0 in range(0, M, block):
        B, P = mdl.B_P(Xs[m0:m0 + block], terms)
        mb = B.shape[0]
        V = O.solve_lower(L, B.reshape(mb * D, -1).T).T.reshape(mb, D, -1)   # V_d = b_d L^-T
        dmean[m0:m0 + mb] = V @ v
        dcov[m0:m0 + mb] = P - np.einsum("mdn,men->mde", V, V)
    idx = np.arange(D)
    return dmean, dcov[:, idx, idx].copy(), dcov


def prior_curvature(spec, theta, X, Xs, terms=None, periodic=0, periods=None):
    """P alone: (M, D, D)."""
    return Model(spec, theta, X, periodic, periods).B_P(np.asarray(Xs, float), terms)[1]


def fd_slope_cov(spec, theta, X, y, Xs, cols, h, periodic=0, periods=None):
    """Richardson-extrapolated central differences (h and h / 2) of the joint posterior covariance of f at (x* + a e_d, x* + b e_e):
    ``Cov[g_d, g_e] = d^2 C(x, x') / d x_d d x'_e`` at x = x' = x*.  (M, len(cols), len(cols))."""
    Xs = np.asarray(Xs, float)
    mdl = Model(spec, theta, X, periodic, periods)
    L, _ = mdl.factor(y)
    M = len(Xs)

    def mixed(d, e, step):
        out = np.empty(M)
        for m in range(M):
            pts = np.repeat(Xs[m:m + 1], 4, axis=0)
            pts[0, d] += step
            pts[1, d] -= step
            pts[2, e] += step
            pts[3, e] -= step
            C = mdl.joint_cov(None, pts, L)
            out[m] = (C[0, 2] - C[0, 3] - C[1, 2] + C[1, 3]) / (4.0 * step * step)
        return out

    out = np.empty((M, len(cols), len(cols)))
    for i, d in enumerate(cols):
        for j, e in enumerate(cols):
            out[:, i, j] = (4.0 * mixed(d, e, 0.5 * h) - mixed(d, e, h)) / 3.0
    return out


# ---- the problems ---------------------------------------------------------------------------------------------------------------------
PROBLEMS = ["matern52", "matern52_illcond", "matern32_1d", "three_term", "periodic", "matern52_periodic"]
POINT_COUNTS = [1, 129, 200]


@functools.lru_cache(maxsize=None)
def problem(name):
    """``(spec, theta, X, y, periodic, periods)``.

    matern52 / matern52_illcond  Matern-5/2, N = 700, d = 3 (six block columns, the last ragged, 3 columns padded to 4), sigma = 0.25 /
                                 0.02 (cond about 3e3 / 4.5e5)
    matern32_1d                  Matern-3/2, N = 200, d = 1
    three_term                   the additive model of components_reference (N = 300: two coregion tables, two outputs, hetero
                                 noise, a linear dimension)
    periodic / matern52_periodic ``Periodic`` (mode 2) and ``Matern52+Periodic`` (mode 1), N = 200, d = 2
    expquad_small                ExpQuad, N = 60, d = 2 (the finite-difference check)
    """
    if name in ("matern52", "matern52_illcond"):
        return LR.matern_problem(0.25 if name == "matern52" else 0.02) + (0, None)
    if name == "three_term":
        return LR.three_term_problem() + (0, None)
    if name == "matern32_1d":
        X, y, ls = O.synthetic_table(200, 1, seed=1201)
        spec = O.make_spec(1, range(1), kind="Matern32")
        return spec, O.pack_theta(spec, ls, 1.1, 0.25), X, y, 0, None
    if name == "expquad_small":
        X, y, ls = O.synthetic_table(60, 2, seed=2060)
        spec = O.make_spec(2, range(2), kind="ExpQuad")
        return spec, O.pack_theta(spec, ls, 1.1, 0.25), X, y, 0, None
    if name in ("periodic", "matern52_periodic"):
        mode, kind = (2, "ExpQuad") if name == "periodic" else (1, "Matern52")
        rng = np.random.default_rng(77 + mode)
        X = rng.uniform(-2.0, 2.0, (200, 2))
        periods = np.array([1.7, 2.9])
        y = np.sin(2 * np.pi * X[:, 0] / periods[0]) * np.cos(2 * np.pi * X[:, 1] / periods[1]) + 0.1 * rng.standard_normal(200)
        spec = O.make_spec(2, range(2), kind=kind)
        return spec, O.pack_theta(spec, [0.9, 1.3], 1.1, 0.2), X, y, mode, periods
    raise KeyError(name)


def cont_columns(spec):
    return sorted(set(spec["idx_cont"]) | set(spec["idx_lin"]))


@functools.lru_cache(maxsize=None)
def points(name, M, seed=1):
    """M test points: 0.3 off randomly chosen training rows along the differentiable columns, every other column kept; the first
    M // 8 exactly ON their training point."""
    spec, _, X, _, _, _ = problem(name)
    rng = np.random.default_rng(seed + M)
    Xs = X[rng.integers(0, len(X), M)].copy()
    cols = cont_columns(spec)
    on = M // 8
    Xs[on:, cols] += 0.3 * rng.standard_normal((M - on, len(cols)))
    Xs.setflags(write=False)
    return Xs


@functools.lru_cache(maxsize=None)
def reference(name, M, terms=None):
    """``posterior`` of a problem at ``points(name, M)``, computed once and shared read-only."""
    spec, theta, X, y, periodic, periods = problem(name)
    out = posterior(spec, theta, X, y, points(name, M), terms, periodic, periods)
    for a in out:
        a.setflags(write=False)
    return out


def p_scale(name, M, terms=None):
    """``max(1, max_d P_dd)`` over the points: the size of the two terms whose difference the covariance is."""
    spec, theta, X, _, periodic, periods = problem(name)
    P = prior_curvature(spec, theta, X, points(name, M), terms, periodic, periods)
    return max(1.0, float(np.max(np.abs(P))))


# ---- the Kronecker combination ----------------------------------------------------------------------------------------------------
def kron_combine(Q, Dd, means, covs, task):
    """IcmEngine's rule: with the P eigen-systems' slopes ``means[p]`` (M, D) and covariances ``covs[p]`` (M, D, D) at the points,
    ``dmean = sqrt(Dd[task]) sum_p Q[task, p] means[p]`` and ``dcov = Dd[task] sum_p Q[task, p]^2 covs[p]`` per point."""
    means, covs = np.asarray(means), np.asarray(covs)
    w = Q[task, :]                                      # (M, P)
    dmean = np.sqrt(Dd[task])[:, None] * np.einsum("mp,pmd->md", w, means)
    dcov = Dd[task][:, None, None] * np.einsum("mp,pmde->mde", w ** 2, covs)
    return dmean, dcov
