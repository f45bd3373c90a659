"""numpy reference of the sparse (FITC) approximation -- PyMC's ``MarginalSparse(approx="FITC")`` restated.  TEST INFRASTRUCTURE ONLY.

With Z the m inducing points, ``k`` the model's covariance without noise (``oracle.gp_oracle.cov_full`` / ``cov_diag``)::

    Kuu = k(Z, Z) + jitter I = Lu Lu^T       A = Lu^-1 k(Z, X)       lambda_i = max(k(x_i, x_i) - sum_k A_ki^2, 0) + sigma^2
    B = I + A Lambda^-1 A^T = L_B L_B^T      c = L_B^-1 A Lambda^-1 y
    NLML = 1/2 sum log lambda + sum log diag(L_B) + 1/2 (y^T Lambda^-1 y - c^T c) + N/2 log 2 pi
    predict: As = Lu^-1 k(Z, X*), C* = L_B^-1 As:  mean = As^T L_B^-T c,  var = k** - colsum(As^2) + colsum(C*^2) (+ sigma^2)

``nlml`` / ``predict`` / ``nlml_grad`` are dense float64 restatements (LAPACK: what a backward-stable float64 host computes);
``precise`` is the same in ``np.longdouble`` with the Cholesky and the triangular solves of ``tests/precise_reference.py``, from
covariance matrices that are themselves evaluated in longdouble; ``precise_grad`` differentiates that NLML by central differences
with one Richardson step.  The stationary models of the sparse path only: one output, no categorical or linear dimensions.

``problem(name)`` defines the shapes the CPU and the GPU tests share.
"""
import functools

import numpy as np
from scipy.linalg import cholesky as _potrf
from scipy.linalg import solve_triangular as _trsm

import precise_reference as P
from oracle import gp_oracle as O

LD = np.longdouble


# ---- the covariance pieces ------------------------------------------------------------------------------------------------------
def _pieces(spec, theta, X, Z, Xs=None):
    """float64: Kuu (with the jitter), k(Z, X), diag k(X, X), sigma^2 [, k(Z, X*), diag k(X*, X*)]"""
    p = O.unpack_theta(spec, theta)
    Kuu = O.cov_full(spec, theta, Z, None, dist_mode="direct") + spec["jitter"] * np.eye(len(Z))
    out = [Kuu, O.cov_full(spec, theta, Z, X, dist_mode="direct"), O.cov_diag(spec, theta, X), float(p["sigma"]) ** 2]
    if Xs is not None:
        out += [O.cov_full(spec, theta, Z, Xs, dist_mode="direct"), O.cov_diag(spec, theta, Xs)]
    return out


def _cov_ld(spec, theta, A, B):
    """k(A, B) in longdouble for a longdouble theta = [ls | eta | sigma] (direct distances; the oracle's kernel formulas)."""
    ic = spec["idx_cont"]
    n_ls = len(ic) if spec["ard"] else 1
    ls = np.asarray(theta[:n_ls], dtype=LD)
    r2 = O.square_dist(np.asarray(A, float)[:, ic], np.asarray(B, float)[:, ic], ls, mode="direct")
    assert r2.dtype == LD
    return LD(theta[n_ls]) ** 2 * O.stationary_from_r2(spec["kind"], r2)


# ---- float64 -------------------------------------------------------------------------------------------------------------------
def _state(spec, theta, X, y, Z):
    Kuu, Kuf, kdiag, s2 = _pieces(spec, theta, X, Z)
    Lu = _potrf(Kuu, lower=True, check_finite=False)
    A = _trsm(Lu, Kuf, lower=True, check_finite=False)
    gap = kdiag - np.sum(A * A, axis=0)
    lam = np.maximum(gap, 0.0) + s2
    B = np.eye(len(Z)) + (A / lam) @ A.T
    LB = _potrf(B, lower=True, check_finite=False)
    c = _trsm(LB, A @ (y / lam), lower=True, check_finite=False)
    return dict(Lu=Lu, A=A, lam=lam, LB=LB, c=c, gap=gap, s2=s2)


def nlml(spec, theta, X, y, Z):
    s = _state(spec, theta, X, y, Z)
    return float(0.5 * np.sum(np.log(s["lam"])) + np.sum(np.log(np.diag(s["LB"]))) + 0.5 * (y @ (y / s["lam"]) - s["c"] @ s["c"])
                 + 0.5 * len(y) * np.log(2 * np.pi))


def min_gap(spec, theta, X, y, Z):
    """min_i (k(x_i, x_i) - q_i): positive when no entry of lambda clips"""
    return float(np.min(_state(spec, theta, X, y, Z)["gap"]))


def predict(spec, theta, X, y, Z, Xs, with_noise=True):
    s = _state(spec, theta, X, y, Z)
    Ksu, kss = _pieces(spec, theta, X, Z, Xs)[4:]
    As = _trsm(s["Lu"], Ksu, lower=True, check_finite=False)
    Cs = _trsm(s["LB"], As, lower=True, check_finite=False)
    w = _trsm(s["LB"], s["c"], lower=True, trans="T", check_finite=False)
    var = kss - np.sum(As * As, axis=0) + np.sum(Cs * Cs, axis=0)
    return As.T @ w, var + (s["s2"] if with_noise else 0.0)


def nlml_grad(spec, theta, X, y, Z):
    """d NLML / d theta (theta = [ls | eta | sigma]) by hand-written reverse mode; nothing N x N::

        C = L_B^-1 A      alpha = (y - C^T c) / lambda      H = L_B^-T C Lambda^-1
        d_i = 1 / lambda_i - colsumsq(C)_i / lambda_i^2 - alpha_i^2
        T = H - (A alpha) alpha^T - A diag(d)      G_uf = Lu^-T T      G_uu = -1/2 G_uf (Lu^-T A)^T
        dNLML/dtheta_j = sum G_uf o dk(Z, X)/dtheta_j + sum G_uu o dk(Z, Z)/dtheta_j + 1/2 sum_i d_i dk(x_i, x_i)/dtheta_j
        dNLML/dsigma   = sigma sum_i d_i

    (a clipped entry of lambda is a constant)"""
    s = _state(spec, theta, X, y, Z)
    p = O.unpack_theta(spec, theta)
    A, lam, LB, Lu = s["A"], s["lam"], s["LB"], s["Lu"]
    C = _trsm(LB, A, lower=True, check_finite=False)
    alpha = (y - C.T @ s["c"]) / lam
    H = _trsm(LB, C, lower=True, trans="T", check_finite=False) / lam
    d = 1.0 / lam - np.sum(C * C, axis=0) / lam**2 - alpha**2
    T = H - np.outer(A @ alpha, alpha) - A * d
    Guf = _trsm(Lu, T, lower=True, trans="T", check_finite=False)
    Guu = -0.5 * Guf @ _trsm(Lu, A, lower=True, trans="T", check_finite=False).T
    ic = spec["idx_cont"]
    ls = np.broadcast_to(np.asarray(p["ls"], float), (len(ic),))
    eta = float(p["eta"])

    def pair_sums(G, Pn, Qn):  # sum G o dk(P, Q)/d ls_c (per column c) and /d eta
        diff = (Pn[:, None, ic] - Qn[None, :, ic]) / ls
        r2 = np.einsum("ijk,ijk->ij", diff, diff)
        Gk = G * eta**2 * O._stationary_dr2(spec["kind"], r2)
        g_ls = np.array([np.sum(Gk * diff[:, :, c] ** 2) * (-2.0 / ls[c]) for c in range(len(ic))])
        return g_ls, np.sum(G * eta**2 * O.stationary_from_r2(spec["kind"], r2)) * 2.0 / eta

    a_ls, a_eta = pair_sums(Guf, Z, X)
    b_ls, b_eta = pair_sums(Guu, Z, Z)
    g_ls = a_ls + b_ls
    if not spec["ard"]:
        g_ls = np.array([g_ls.sum()])
    return np.concatenate([g_ls, [a_eta + b_eta + 0.5 * np.sum(d) * 2.0 * eta], [float(p["sigma"]) * np.sum(d)]])


# ---- longdouble ----------------------------------------------------------------------------------------------------------------
def _state_ld(spec, theta, X, y, Z):
    theta = np.asarray(theta, dtype=LD)
    n_ls = len(spec["idx_cont"]) if spec["ard"] else 1
    eta, sigma = theta[n_ls], theta[n_ls + 1]
    Kuu = _cov_ld(spec, theta, Z, Z) + LD(spec["jitter"]) * np.eye(len(Z), dtype=LD)
    Lu = P.cholesky(Kuu)
    A = P.solve_lower(Lu, _cov_ld(spec, theta, Z, X))
    yl = np.asarray(y, dtype=LD)
    lam = np.maximum(eta**2 - np.sum(A * A, axis=0), LD(0)) + sigma**2
    B = np.eye(len(Z), dtype=LD) + (A / lam) @ A.T
    LB = P.cholesky(B)
    c = P.solve_lower(LB, A @ (yl / lam))
    val = (np.sum(np.log(lam)) / 2 + np.sum(np.log(np.diag(LB))) + (yl @ (yl / lam) - c @ c) / 2
           + LD(len(yl)) / 2 * np.log(LD(2) * LD(np.pi)))
    return dict(theta=theta, Lu=Lu, LB=LB, c=c, nlml=val, s2=sigma**2, eta2=eta**2)


def precise(spec, theta, X, y, Z, Xs=None):
    """longdouble ``nlml`` and, with ``Xs``, ``mean``, ``var`` (noiseless) and ``var_noise``"""
    s = _state_ld(spec, theta, X, y, Z)
    out = {"nlml": s["nlml"]}
    if Xs is not None:
        As = P.solve_lower(s["Lu"], _cov_ld(spec, s["theta"], Z, Xs))
        Cs = P.solve_lower(s["LB"], As)
        w = P.solve_upper_t(s["LB"], s["c"])
        out["mean"] = As.T @ w
        out["var"] = s["eta2"] - np.sum(As * As, axis=0) + np.sum(Cs * Cs, axis=0)
        out["var_noise"] = out["var"] + s["s2"]
    return out


def precise_grad(spec, theta, X, y, Z, rel_step=2e-3):
    """central differences of the longdouble NLML with one Richardson step: (4 D(h / 2) - D(h)) / 3, h = rel_step * theta_j"""
    theta = np.asarray(theta, dtype=LD)
    g = np.zeros(theta.size, dtype=LD)

    def f(j, h):
        t = theta.copy()
        t[j] += h
        return _state_ld(spec, t, X, y, Z)["nlml"]

    for j in range(theta.size):
        h = LD(rel_step) * theta[j]
        d1 = (f(j, h) - f(j, -h)) / (2 * h)
        d2 = (f(j, h / 2) - f(j, -h / 2)) / h
        g[j] = (4 * d2 - d1) / 3
    return g


# ---- a stand-in engine for the front end's CPU tests ----------------------------------------------------------------------------
def use_fitc_oracle(monkeypatch):
    """``gumbi_amd.Engine`` replaced by a numpy stand-in with the sparse calls (the front end's tests without a device)"""
    from gumbi_amd.regression import hip_gp
    from oracle_engine import OracleEngine

    class FitcOracleEngine(OracleEngine):
        Z = None

        def set_inducing(self, Z):
            if self.spec["coreg"] or self.spec["out_col"] >= 0 or self.spec["idx_lin"] or self.spec.get("additive"):
                raise ValueError("gmb_fitc_set_inducing: outside the sparse approximation's scope")
            self.Z = np.array(Z, dtype=float)
            self._fitc_theta = None

        def fitc_evaluate(self, theta, grad=True):
            self.set_theta(theta)
            val = nlml(self.spec, self.theta, self.X, self.y, self.Z)
            self._fitc_theta = self.theta.copy()
            return (val, nlml_grad(self.spec, self.theta, self.X, self.y, self.Z)) if grad else val

        def fitc_predict(self, Xs, with_noise=True):
            if self._fitc_theta is None or not np.array_equal(self._fitc_theta, self.theta):
                raise ValueError("gmb_fitc_predict: no sparse state is resident")
            return predict(self.spec, self.theta, self.X, self.y, self.Z, np.asarray(Xs, float), with_noise=with_noise)

    monkeypatch.setattr(hip_gp, "Engine", FitcOracleEngine)
    return FitcOracleEngine


# ---- the shared problems --------------------------------------------------------------------------------------------------------
def kmeans_points(X, m, seed):
    """m inducing points from seeded k-means of the whitened X (what ``pm.gp.util.kmeans_inducing_points`` does); when k-means
    comes back with fewer centres, midpoints of seeded pairs of rows of X fill up -- a problem has exactly the m it names."""
    from scipy.cluster.vq import kmeans

    X = np.asarray(X, float)
    scale = np.std(X, axis=0)
    scale[scale <= 1e-6] = 1.0
    Z = kmeans(X / scale, m, seed=seed)[0] * scale
    if len(Z) < m:
        rng = np.random.default_rng(seed)
        pairs = rng.integers(0, len(X), size=(m - len(Z), 2))
        Z = np.vstack([Z, 0.5 * (X[pairs[:, 0]] + X[pairs[:, 1]])])
    return np.ascontiguousarray(Z[:m])


#: name -> (kind, N, d, m, sigma, ard); N = None: taken from the engine's plan (two column tiles of X, see problem())
PROBLEMS = {
    "m52-ragged-0.2": ("Matern52", 700, 3, 130, 0.2, True),     # six ragged column blocks of 128; m over one tile, ragged; 3 columns padded to 4
    "m52-ragged-0.02": ("Matern52", 700, 3, 130, 0.02, True),
    "expquad-1d": ("ExpQuad", 200, 1, 100, 0.2, True),          # one m-tile
    "m32-2d": ("Matern32", 300, 2, 64, 0.02, True),
    "exponential-m1": ("Exponential", 300, 2, 1, 0.1, True),    # m = 1
    "expquad-shared": ("ExpQuad", 300, 2, 48, 0.1, False),      # one lengthscale for both columns
}
#: every kind at every padded width 1, 2, 4, 8, 16 of the derivative kernel: N = 200, m = 16, eta = 1.1, sigma = 0.25
DISPATCH = {f"{kind}-d{d}": (kind, 200, d, 16, 0.25, True) for kind in O.KINDS for d in (1, 2, 3, 5, 9)}
TILE_ROWS_SMALL_M = 32768  # columns of X per tile of the plan for small m (tests/test_fitc_cpu.py checks it against the engine)
SEAM = ("Matern52", TILE_ROWS_SMALL_M + 77, 2, 16, 0.2, True)  # two column tiles of X: the second one ragged
TEST_POINTS = (1, 129, 200)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(spec, theta, X, y, Z, Xs) of a named problem; every array read-only"""
    kind, N, d, m, sigma, ard = SEAM if name == "seam" else DISPATCH[name] if name in DISPATCH else PROBLEMS[name]
    X, y, ls = O.synthetic_table(N, d, seed=7 + N, sigma=sigma)
    spec = O.make_spec(d, range(d), kind=kind, ard=ard)
    theta = O.pack_theta(spec, ls if ard else [float(np.mean(ls))], 1.1 if name in DISPATCH else 1.0, sigma)
    Z = kmeans_points(X, m, seed=11)
    Xs = np.random.default_rng(3).standard_normal((max(TEST_POINTS), d)) * 1.2
    for a in (theta, X, y, Z, Xs):
        a.setflags(write=False)
    return spec, theta, X, y, Z, Xs


@functools.lru_cache(maxsize=None)
def references(name, grad=True):
    """longdouble and float64 results of a problem at its first max(TEST_POINTS) test points, computed once: a dict with
    ``nlml``, ``grad``, ``mean``, ``var``, ``var_noise`` (longdouble, rounded to float64) and ``h_*`` (the float64 host's)"""
    spec, theta, X, y, Z, Xs = problem(name)
    ref = precise(spec, theta, X, y, Z, Xs)
    out = {k: np.asarray(v, dtype=float) for k, v in ref.items()}
    out["h_nlml"] = nlml(spec, theta, X, y, Z)
    out["h_mean"], out["h_var_noise"] = predict(spec, theta, X, y, Z, Xs, with_noise=True)
    out["h_var"] = predict(spec, theta, X, y, Z, Xs, with_noise=False)[1]
    if grad:
        out["grad"] = np.asarray(precise_grad(spec, theta, X, y, Z), dtype=float)
        out["h_grad"] = nlml_grad(spec, theta, X, y, Z)
    return out
