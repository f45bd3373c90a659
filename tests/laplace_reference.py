"""numpy reference of GP classification by the Laplace approximation (Rasmussen & Williams, Algorithms 3.1, 3.2, 5.1; logit link,
labels in {0, 1}, zero mean) -- TEST INFRASTRUCTURE ONLY.

With Sigma the float64 matrix the oracle builds for ``(spec, theta, X)`` (``oracle.gp_oracle.sigma_matrix``, direct distances;
taken as exact, as ``tests/precise_reference.py`` takes it)::

    pi = 1 / (1 + e^-f)    log p = sum y f - log(1 + e^f)    g = y - pi    W = pi (1 - pi)    s = sqrt(W)
    Newton from a = f = 0:  b = W f + g,  B = I + (s s^T) o Sigma = L L^T,  a^ = b - s o B^-1 (s o (Sigma b)),
        a <- a + t (a^ - a), f = Sigma a, t = 1 halved while Psi(a, f) = -1/2 a^T f + log p(y | f) falls (slack 1e-14 |Psi|);
        stop at max |f_new - f| <= tol max(1, max |f_new|)
    -log q = -Psi(a^, f^) + sum log L_ii          (B at the mode)
    gradient: R = (s s^T) o B^-1, s2 = -1/2 (1 - diag B^-1)(1 - 2 pi), u = s2 - R (Sigma s2), Z' = R + u u^T, a' = a^ + u,
        d(-log q)/dtheta = 1/2 tr((Z' - a' a'^T) dSigma/dtheta)        (the oracle's chain rule, ``O.grad_given_M``)
    predict: mean = k*^T (y - pi^), var = k** - |L^-1 (s o k*)|^2

``host`` runs this on LAPACK in float64 with the engine's stop rule (tol 1e-9); ``precise`` in ``np.longdouble`` with the Cholesky
and the solves of ``tests/precise_reference.py``, iterated to a step of 1e-17.  ``problem(name)`` defines the shapes the CPU and
the GPU tests share; ``references(name)`` computes both once.
"""
import functools

import numpy as np
from scipy.linalg import cholesky as _potrf
from scipy.linalg import solve_triangular as _trsm

import precise_reference as P
from oracle import gp_oracle as O

LD = np.longdouble
MAX_ITER, MAX_HALVINGS = 40, 20


class NoConvergence(RuntimeError):
    pass


# ---- the two arithmetic back ends ------------------------------------------------------------------------------------------------
class _Host:
    dtype = np.float64
    chol = staticmethod(lambda S: _potrf(S, lower=True, check_finite=False))
    solve_l = staticmethod(lambda L, B: _trsm(L, B, lower=True, check_finite=False))
    solve_lt = staticmethod(lambda L, B: _trsm(L, B, lower=True, trans="T", check_finite=False))


class _Precise:
    dtype = LD
    chol = staticmethod(P.cholesky)
    solve_l = staticmethod(P.solve_lower)
    solve_lt = staticmethod(P.solve_upper_t)


def likelihood(f, y):
    """pi, W, log p(y | f) from e^-|f| (nothing overflows or cancels at |f| = 60); the dtype of ``f``"""
    e = np.exp(-np.abs(f))
    r = 1 / (1 + e)
    pi = np.where(f >= 0, r, e * r)
    W = e * r * r
    lp = np.sum(y * f - (np.maximum(f, 0) + np.log1p(e)))
    return pi, W, lp


def _factor_b(be, S, s):
    B = (s[:, None] * s[None, :]) * S
    B[np.diag_indices_from(B)] += 1
    return be.chol(B)


def mode(S, y, be, tol, max_iter=MAX_ITER, floor=False):
    """Alg. 3.1 with the halved step.  Returns a dict: f, a, psi, iterations, halvings, step, and pi, W, s, L at the mode."""
    T = be.dtype
    S = np.asarray(S, dtype=T)
    y = np.asarray(y, dtype=T)
    N = len(y)
    a = np.zeros(N, dtype=T)
    f = np.zeros(N, dtype=T)
    pi, W, lp = likelihood(f, y)
    psi = lp - (a @ f) / 2
    iterations = halvings = 0
    step = T(0)
    converged = False
    for it in range(1, max_iter + 1):
        s = np.sqrt(W)
        b = W * f + (y - pi)
        L = _factor_b(be, S, s)
        rhs = s * (S @ b)
        ah = b - s * be.solve_lt(L, be.solve_l(L, rhs))
        t = T(1)
        accepted = False
        for h in range(MAX_HALVINGS + 1):
            ac = a + t * (ah - a)
            fc = S @ ac
            pic, Wc, lpc = likelihood(fc, y)
            psic = lpc - (ac @ fc) / 2
            if psic >= psi - T(1e-14) * abs(psi):
                accepted = True
                break
            t = t / 2
            if h < MAX_HALVINGS:
                halvings += 1
        iterations = it
        if not accepted:
            raise NoConvergence(f"Psi still falls after {MAX_HALVINGS} halvings in iteration {it}")
        prev, step = step, np.max(np.abs(fc - f))
        a, f, pi, W, psi = ac, fc, pic, Wc, psic
        scale = max(T(1), np.max(np.abs(f)))
        # (``floor``: the longdouble reference also stops where the step has reached its rounding floor -- far below the engine's
        # tol, no longer shrinking: f = Sigma a carries eps |Sigma| |a|, 1e-14 at eta = 100)
        if step <= T(tol) * scale or (floor and it > 1 and step <= T(1e-12) * scale and step >= prev / 2):
            converged = True
            break
    if not converged:
        raise NoConvergence(f"no convergence in {max_iter} Newton iterations (last step {float(step):.3g})")
    s = np.sqrt(W)
    return dict(f=f, a=a, psi=psi, iterations=iterations, halvings=halvings, step=step, pi=pi, W=W, s=s, L=_factor_b(be, S, s), S=S, y=y)


def _evaluate(be, spec, theta, X, y, Xs=None, grad=False, tol=1e-9, max_iter=MAX_ITER):
    X = np.asarray(X, float)
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    m = mode(S, y, be, tol, max_iter, floor=be is _Precise)
    T = be.dtype
    L, s, pi, a = m["L"], m["s"], m["pi"], m["a"]
    out = dict(m)
    out["nlq"] = -m["psi"] + np.sum(np.log(np.diag(L)))
    if Xs is not None:
        Xs = np.asarray(Xs, float)
        Kxs = O.cov_full(spec, theta, X, Xs, dist_mode="direct").astype(T)
        A = be.solve_l(L, s[:, None] * Kxs)
        out["mean"] = Kxs.T @ (m["y"] - pi)
        out["var"] = O.cov_diag(spec, theta, Xs).astype(T) - np.sum(A * A, axis=0)
    if grad:
        N = len(a)
        Linv = be.solve_l(L, np.eye(N, dtype=T))
        Binv = Linv.T @ Linv
        R = (s[:, None] * s[None, :]) * Binv
        s2 = -(1 - np.diag(Binv)) * (1 - 2 * pi) / 2
        u = s2 - R @ (m["S"] @ s2)
        ap = a + u
        M = ((R + np.outer(u, u) - np.outer(ap, ap)) / 2).astype(float)
        out["grad"] = O.grad_given_M(spec, theta, X, M, dist_mode="direct")
    return out


def host(spec, theta, X, y, Xs=None, grad=False, tol=1e-9, max_iter=MAX_ITER):
    """float64 on LAPACK, the engine's stop rule"""
    return _evaluate(_Host, spec, theta, X, y, Xs, grad, tol, max_iter)


def precise(spec, theta, X, y, Xs=None, grad=False):
    """longdouble, iterated to a step of 1e-17 (or to the step's rounding floor, see ``mode``)"""
    return _evaluate(_Precise, spec, theta, X, y, Xs, grad, tol=1e-17, max_iter=MAX_ITER)


def objective(spec, theta, X, y, precise_arithmetic=True):
    """-log q(y | theta) alone (central differences of it check the gradient)"""
    return (precise if precise_arithmetic else host)(spec, theta, X, y)["nlq"]


# ---- the shared problems --------------------------------------------------------------------------------------------------------
def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def _points(N, d, seed):
    return np.random.default_rng(seed).standard_normal((N, d))


def _drawn_labels(X, seed):
    rng = np.random.default_rng(seed + 1000)
    return (rng.random(len(X)) < _sigmoid(np.sin(2 * X[:, 0]) + 0.5 * X[:, 1])).astype(float)


#: name -> N; what the rest of a problem is: problem()
PROBLEMS = {
    "N100": 100,        # one ragged tile
    "N128": 128,        # one full tile
    "N129": 129,        # two tiles, one live row in the second
    "N300": 300,        # three tiles, ragged
    "eq-shared": 200,   # ExpQuad, one lengthscale
    "m12-lin": 200,     # Matern-1/2 plus a linear dimension
    "coreg": 210,       # a three-level categorical dimension
    "separated": 129,   # separable labels, ls = 3, eta = 30: |f^| in the tens, W down to 1e-11 and below
    "saturated": 129,   # ... eta = 100
}
TEST_POINTS = (1, 129, 200)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(spec, theta, X, y, Xs) of a named problem; every array read-only.  sigma = 0: Sigma = K + jitter I."""
    N = PROBLEMS[name]
    seed = 100 + N + len(name)
    Ms = max(TEST_POINTS)
    if name in ("N100", "N128", "N129", "N300"):
        d = 3 if name == "N300" else 2
        X = _points(N, d, seed)
        y = _drawn_labels(X, seed)
        spec = O.make_spec(d, range(d), kind="Matern52", ard=True)
        theta = O.pack_theta(spec, [1.0, 1.5, 2.0][:d], 1.5, 0.0)
    elif name == "eq-shared":
        X = _points(N, 2, seed)
        y = _drawn_labels(X, seed)
        spec = O.make_spec(2, range(2), kind="ExpQuad", ard=False)
        theta = O.pack_theta(spec, [1.2], 1.5, 0.0)
    elif name == "m12-lin":
        X = _points(N, 2, seed)
        y = _drawn_labels(X, seed)
        spec = O.make_spec(2, range(2), kind="Matern12", ard=True, idx_lin=[1])
        theta = O.pack_theta(spec, [1.0, 1.5], 1.2, 0.0, c=[0.1], tau=0.5)
    elif name == "coreg":
        X = np.column_stack([_points(N, 2, seed), np.arange(N) % 3]).astype(float)
        y = _drawn_labels(X, seed)
        spec = O.make_spec(3, range(2), kind="Matern52", ard=True, coreg=[(2, 3)])
        W = np.array([[0.9, 0.1], [0.7, -0.3], [0.5, 0.4]])
        theta = O.pack_theta(spec, [1.0, 1.5], 1.5, 0.0, coreg=[(W, [0.3, 0.2, 0.4])])
    else:  # separated, saturated: the labels are a function of x0, nothing to trade off against
        X = _points(N, 2, seed)
        y = (X[:, 0] > 0).astype(float)
        spec = O.make_spec(2, range(2), kind="Matern52", ard=False)
        theta = O.pack_theta(spec, [3.0], 30.0 if name == "separated" else 100.0, 0.0)
    Xs = np.random.default_rng(3).standard_normal((Ms, X.shape[1])) * 1.2
    if name == "coreg":
        Xs[:, 2] = np.arange(Ms) % 3
    for arr in (theta, X, y, Xs):
        arr.setflags(write=False)
    return spec, theta, X, y, Xs


@functools.lru_cache(maxsize=None)
def references(name):
    """longdouble and float64 results of a problem at its max(TEST_POINTS) test points, computed once: ``nlq``, ``grad``, ``f``,
    ``a``, ``mean``, ``var`` (longdouble, rounded to float64), ``h_*`` (the float64 host's) and the two iteration records"""
    spec, theta, X, y, Xs = problem(name)
    ref = precise(spec, theta, X, y, Xs, grad=True)
    h = host(spec, theta, X, y, Xs, grad=True)
    out = {}
    for k in ("nlq", "grad", "f", "a", "mean", "var", "W"):
        out[k] = np.asarray(ref[k], dtype=float)
        out["h_" + k] = np.asarray(h[k], dtype=float)
    for k in ("iterations", "halvings"):
        out[k] = int(ref[k])
        out["h_" + k] = int(h[k])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
