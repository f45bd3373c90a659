"""Averages of the posterior over groups of points in numpy on the oracle's building blocks -- what ``gmb_predict_groups`` and the
front end above it are held against.

The yardstick is the DEFINITION (``by_joint``): the full joint posterior of all M points -- ``O.sigma_matrix``, ``O.cov_full``,
``O.cholesky_lower``, ``O.solve_lower``, ``dist_mode="direct"``, latent function: no noise, no jitter -- then ``W mu`` and
``W C W^T`` with W the G x M matrix of the weights.  ``a_form`` is the engine's algebra, nothing of size M x M used as such:

    A = W K(X*, X)    Q = W K(X*, X*) W^T    V_A = A L^-T    mean = V_A v    cov = Q - V_A V_A^T

(CPU tests hold the two against each other; every GPU bar is against ``by_joint``.)  A selection of an additive model's terms
sums components_reference's per-term covariances.

Problems: leave_out_reference's Matern-5/2 table (N = 700, six block columns, ragged) at sigma = 0.25 and 0.02 (cond 3e3 / 4.5e5)
and the three-term additive model (N = 300: two coregion tables, two outputs, hetero noise, a linear dimension -- the kernels'
general path and the term walk).  Groups: sizes chosen around the kernels' edges (``SIZES``: one point, a staged piece of 128
and its neighbours, two tasks and a point, ...) and 130 groups of 1 - 3 points (G across a 128-row tile of C and into a second
row block of the Q pass).  The points are background rows of the table with one column overwritten per group.
"""
import functools

import numpy as np

import components_reference as CR
import leave_out_reference as LR
from oracle import gp_oracle as O
from oracle_engine import OracleEngine

GROUP_CHUNK = 512  # gumbi_amd/csrc/group_tasks.hpp (tests/test_group_average_cpu.py checks the binding says the same)
SIZES = [1, 2, 127, 128, 129, 2 * GROUP_CHUNK + 1, 300, 64, 5, 131]
PROBLEMS = ["matern", "matern_illcond", "three_term"]
WEIGHTS = ["mean", "null", "signed"]


def problem(name):
    """``(spec, theta, X, y)``."""
    if name == "three_term":
        return LR.three_term_problem()
    return LR.matern_problem(0.25 if name == "matern" else 0.02)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def weight_matrix(offsets, weights=None):
    """W (G x M): row g holds group g's weights, ``1 / |g|`` when ``weights`` is None."""
    offsets = np.asarray(offsets, dtype=np.int64)
    G, M = len(offsets) - 1, int(offsets[-1])
    W = np.zeros((G, M))
    for g in range(G):
        lo, hi = offsets[g], offsets[g + 1]
        W[g, lo:hi] = 1.0 / (hi - lo) if weights is None else np.asarray(weights, float)[lo:hi]
    return W


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def points(name, which):
    """``(Xs, offsets)`` of a problem: ``which`` = "sizes" (``SIZES``) or "many" (130 groups of 1 - 3 points).  Group g's points
    are background rows (drawn with replacement, seeded) with column 0 set to the group's own value."""
    _, _, X, _ = problem(name)
    rng = np.random.default_rng(17 if which == "sizes" else 23)
    sizes = SIZES if which == "sizes" else list(rng.integers(1, 4, 130))
    offsets = offsets_of(sizes)
    Xs = X[rng.integers(0, len(X), int(offsets[-1]))].copy()
    values = np.linspace(-1.8, 1.8, len(sizes))
    for g in range(len(sizes)):
        Xs[offsets[g]:offsets[g + 1], 0] = values[g]
    return _frozen(Xs, offsets)


@functools.lru_cache(maxsize=None)
def weights_of(name, which, kind):
    """The weights of a point set: "mean" explicit ``1 / |g|``, "null" None, "signed" the plain mean with the second half of the
    longest group negated (a contrast)."""
    _, offsets = points(name, which)
    if kind == "null":
        return None
    sizes = np.diff(offsets)
    w = np.concatenate([np.full(n, 1.0 / n) for n in sizes])
    if kind == "signed":
        g = int(np.argmax(sizes))
        w[offsets[g] + sizes[g] // 2:offsets[g + 1]] *= -1.0
    return _frozen(w)[0]


def weight_norms(offsets, weights):
    """``||w_g||_1`` per group (1 for a plain mean)."""
    return np.abs(weight_matrix(offsets, weights)).sum(axis=1)


def _selected(spec, theta, terms):
    """``[(sub_spec, sub_theta)]`` of the selection (every term for None)."""
    parts = CR.term_list(spec, theta)
    return parts if terms is None else [parts[t] for t in CR.as_indices(terms, len(parts))]


def _cov(spec, theta, terms, A, B):
    return sum(O.cov_full(sp, th, A, B, dist_mode="direct") for sp, th in _selected(spec, theta, terms))


def _factor(spec, theta, X, y):
    L = O.cholesky_lower(O.sigma_matrix(spec, np.asarray(theta, float), np.asarray(X, float), dist_mode="direct"))
    return L, O.solve_lower(L, np.asarray(y, float))


def joint_posterior(spec, theta, X, y, Xs, terms=None):
    """``(mu, C)`` of the latent function at all the points: M and M x M."""
    theta, X, Xs = np.asarray(theta, float), np.asarray(X, float), np.asarray(Xs, float)
    L, v = _factor(spec, theta, X, y)
    V = O.solve_lower(L, _cov(spec, theta, terms, X, Xs))
    return V.T @ v, _cov(spec, theta, terms, Xs, None) - V.T @ V


def by_joint(spec, theta, X, y, Xs, offsets, weights, terms=None):
    """``(mean, cov)`` = ``(W mu, W C W^T)``: the definition."""
    mu, C = joint_posterior(spec, theta, X, y, Xs, terms)
    W = weight_matrix(offsets, weights)
    return W @ mu, W @ C @ W.T


def a_form(spec, theta, X, y, Xs, offsets, weights, terms=None):
    """``(mean, cov)`` by the engine's algebra: G right-hand sides."""
    theta, X, Xs = np.asarray(theta, float), np.asarray(X, float), np.asarray(Xs, float)
    W = weight_matrix(offsets, weights)
    L, v = _factor(spec, theta, X, y)
    VA = O.solve_lower(L, (W @ _cov(spec, theta, terms, Xs, X)).T)
    Q = W @ _cov(spec, theta, terms, Xs, None) @ W.T
    return VA.T @ v, Q - VA.T @ VA


@functools.lru_cache(maxsize=None)
def reference(name, which, kind, terms=None):
    """``by_joint`` of a problem's point set and weights, computed once and shared read-only."""
    Xs, offsets = points(name, which)
    return _frozen(*by_joint(*problem(name), Xs, offsets, weights_of(name, which, kind), terms))


class GroupOracleEngine(OracleEngine):
    """The numpy stand-in of ``gumbi_amd.engine.Engine`` with ``predict_groups``, by the definition (test infrastructure: the
    front end's CPU tests monkeypatch it in)."""

    def predict(self, Xs, with_noise=True, terms=None):
        if terms is None:
            return super().predict(Xs, with_noise=with_noise)
        return CR.predict_terms(self.spec, self.theta, self.X, self.y, np.asarray(Xs, float), terms, with_noise)

    def predict_groups(self, Xs, offsets, weights=None, cov=False, terms=None):
        mean, full = by_joint(self.spec, self.theta, self.X, self.y, Xs, offsets, weights, terms)
        return (mean, np.diag(full).copy(), full) if cov else (mean, np.diag(full).copy())


def use_group_oracle(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", GroupOracleEngine)
    monkeypatch.setattr(icm, "Engine", GroupOracleEngine)
