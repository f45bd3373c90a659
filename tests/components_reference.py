"""The posterior of an additive model's components, restated in numpy on the oracle's building blocks (``O.additive_terms``,
``O.cov_full``, ``O.cov_diag``, ``O.noise_diag``, ``O.sigma_matrix``) -- what the engine's ``*_terms`` calls and
``gmb_predict_decompose`` are held against.

The model's covariance is a sum of T terms, ``K = sum_t K_t``; with ``L L^T = Sigma`` of the WHOLE model, ``v = L^-1 y`` and
``V_t = K_t(X*, X) L^-T``:

    mu_S  = sum_{t in S} V_t v                 cov_S = K_S(X*, X*) - V_S V_S^T,  V_S = sum_{t in S} V_t
    cov(f_t, f_u | y)(x*) = delta_tu k_t(x*, x*) - <V_t(x*), V_u(x*)>

Noise and jitter belong to no term; ``with_noise`` adds the model's noise diagonal to a selection's variance.  Everything is in
``dist_mode="direct"``, the oracle's form the GPU tests compare against.
"""
import functools

import numpy as np

import grad_reference as GR
from oracle import gp_oracle as O


def three_term_problem():
    """``tests/test_oracle.py::additive_problem``'s recipe with a second categorical column: two continuous dimensions (one
    linear), categorical columns 2 (3 levels) and 3 (2 levels), output column 4, two outputs x 150 rows (N = 300), hetero noise,
    seed 11.  Returns ``(spec, theta, X, y, Xs)`` with ``Xs = X[::4]``, column 0 shifted by 0.17 (M = 75)."""
    return _three_term_problem()


@functools.lru_cache(maxsize=None)
def _three_term_problem():
    n, P = 150, 2
    rng = np.random.default_rng(11)
    Xc = rng.standard_normal((n, 2))
    cat = rng.integers(0, 3, n).astype(float)
    cat2 = rng.integers(0, 2, n).astype(float)
    X1 = np.column_stack([Xc, cat[:, None], cat2[:, None]])
    X = np.vstack([np.column_stack([X1, np.full(n, p)]) for p in range(P)])
    spec = O.make_spec(X.shape[1], [0, 1], idx_lin=[1], coreg=[(2, 3), (3, 2)], out_col=4, n_out=P, hetero_noise=True, additive=True)
    theta = np.abs(rng.normal(1.0, 0.3, O.theta_size(spec))) + 0.2
    y = rng.standard_normal(len(X))
    Xs = X[::4].copy()
    Xs[:, 0] += 0.17
    return spec, theta, X, y, Xs


def term_list(spec, theta):
    """``[(sub_spec, sub_theta)]``: the model's terms as non-additive models (one entry for a non-additive spec)."""
    if spec.get("additive"):
        return [(sp, np.asarray(th, float)) for sp, th, _ in O.additive_terms(spec, theta)]
    return [(spec, np.asarray(theta, float))]


def as_indices(terms, T):
    """A selection -- a mask or an iterable of indices -- as a sorted list of term indices."""
    if isinstance(terms, (int, np.integer)):
        return [t for t in range(T) if (int(terms) >> t) & 1]
    return sorted(int(t) for t in terms)


class Components:
    """The whole model's factor and every term's solved cross-covariance ``A_t = L^-1 K_t(X, X*)`` (N x M), computed once."""

    def __init__(self, spec, theta, X, y, Xs):
        self.spec, self.theta = spec, np.asarray(theta, float)
        self.X, self.y, self.Xs = np.asarray(X, float), np.asarray(y, float), np.asarray(Xs, float)
        self.terms = term_list(spec, self.theta)
        self.T = len(self.terms)
        self.L = O.cholesky_lower(O.sigma_matrix(spec, self.theta, self.X, dist_mode="direct"))
        self.v = O.solve_lower(self.L, self.y)
        self.A = [O.solve_lower(self.L, O.cov_full(sp, th, self.X, self.Xs, dist_mode="direct")) for sp, th in self.terms]
        self.kss = [O.cov_diag(sp, th, self.Xs) for sp, th in self.terms]
        self.noise = O.noise_diag(spec, self.theta, self.Xs)

    def predict_terms(self, terms, with_noise=True):
        """``(mean, var)`` of the selection: ``gmb_predict_terms``."""
        sel = as_indices(terms, self.T)
        A = sum(self.A[t] for t in sel)
        var = sum(self.kss[t] for t in sel) - np.sum(A * A, axis=0)
        return A.T @ self.v, var + self.noise if with_noise else var

    def joint_terms(self, terms, with_noise=True, jitter=0.0):
        """``(mean, cov)`` of the selection, cov M x M: ``gmb_predict_joint_terms``."""
        sel = as_indices(terms, self.T)
        A = sum(self.A[t] for t in sel)
        C = sum(O.cov_full(*self.terms[t], self.Xs, None, dist_mode="direct") for t in sel) - A.T @ A
        C[np.diag_indices_from(C)] += (self.noise if with_noise else 0.0) + jitter
        return A.T @ self.v, C

    def decompose(self):
        """``(means (T, M), cov (T, T, M), noise (M))``: ``gmb_predict_decompose`` -- latent components, no noise, no jitter."""
        means = np.stack([A.T @ self.v for A in self.A])
        cov = np.empty((self.T, self.T, self.Xs.shape[0]))
        for t in range(self.T):
            for u in range(self.T):
                cov[t, u] = (self.kss[t] if t == u else 0.0) - np.sum(self.A[t] * self.A[u], axis=0)
        return means, cov, self.noise

    def grad_terms(self, terms):
        """``d mu_S / d x*`` (M, D): ``grad_reference.mean_grad``'s sum over terms, restricted to the selection -- each term's
        sub-spec differentiated against the WHOLE model's ``alpha = Sigma^-1 y``."""
        alpha = GR._alpha(self.spec, self.theta, self.X, self.y)
        return sum(GR._stationary_grad(*self.terms[t], self.X, self.Xs, alpha) for t in as_indices(terms, self.T))


def predict_terms(spec, theta, X, y, Xs, terms, with_noise=True):
    return Components(spec, theta, X, y, Xs).predict_terms(terms, with_noise)


def joint_terms(spec, theta, X, y, Xs, terms, with_noise=True, jitter=0.0):
    return Components(spec, theta, X, y, Xs).joint_terms(terms, with_noise, jitter)


def decompose(spec, theta, X, y, Xs):
    return Components(spec, theta, X, y, Xs).decompose()


def grad_terms(spec, theta, X, y, Xs, terms):
    return Components(spec, theta, X, y, Xs).grad_terms(terms)


def pack_lower(cov):
    """(T, T, M) -> the ABI's packed lower triangle, (T (T + 1) / 2, M): row ``t (t + 1) / 2 + u``, ``u <= t``."""
    T = cov.shape[0]
    return np.stack([cov[t, u] for t in range(T) for u in range(t + 1)])
