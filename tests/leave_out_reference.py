"""Leave-one-out and leave-group-out predictions in numpy on the oracle's building blocks -- what ``gmb_loo`` / ``gmb_leave_out``
and the front end above them are held against.

The yardstick works BY DELETION (``by_deletion``): for the rows B it builds the oracle's Sigma (``O.sigma_matrix``,
``dist_mode="direct"``), deletes the rows and columns of B, factors what is left and predicts B from it like ``O.predict`` -- mean
and full covariance, with the model's noise on the diagonal when ``with_noise`` and NEVER the jitter.  Leave-one-out is the case
of one row.  ``closed_form`` is the other formulation, from ONE factor of the whole Sigma (Rasmussen & Williams 5.4.2):

    y_B | y_-B ~ N(y_B - C^-1 alpha_B, C^-1),   C = (Sigma^-1)_BB,  alpha = Sigma^-1 y;

Sigma holds the jitter, so ``C^-1`` exceeds the deletion covariance (with noise) by exactly ``jitter I``.  The closed form is used
by the CPU tests only (tests/test_leave_out_cpu.py holds the two against each other); every GPU bar is against deletion.

Problems: the three-term additive model of components_reference (N = 300: two coregion tables, two outputs, hetero noise, a linear
dimension) and a Matern-5/2 table, N = 700 = 5 * 128 + 60 (six block columns, the last ragged), d = 3, at sigma = 0.25
(cond(Sigma) 3e3) and sigma = 0.02 (cond 4.5e5, the conditioning case).
"""
import functools

import numpy as np

import components_reference as CR
from oracle import gp_oracle as O
from oracle_engine import OracleEngine

N_MATERN = 700


def three_term_problem():
    """``(spec, theta, X, y)`` of components_reference.three_term_problem."""
    return CR.three_term_problem()[:4]


@functools.lru_cache(maxsize=None)
def _matern(sigma):
    X, y, _ = O.synthetic_table(N_MATERN, 3, seed=5)
    spec = O.make_spec(3, range(3), kind="Matern52")
    theta = O.pack_theta(spec, [0.8, 1.1, 0.9], 1.2, sigma)
    return spec, theta, X, y


def matern_problem(sigma=0.25):
    """``(spec, theta, X, y)``: Matern-5/2, N = 700, d = 3, theta = (0.8, 1.1, 0.9, 1.2, sigma)."""
    return _matern(float(sigma))


def three_term_groups():
    """The groups of the three-term problem: 37 random rows (seed 3), rows 120..259 (m = 140: two block columns of C), the 90-odd
    rows of level 1 of column 2."""
    _, _, X, _ = three_term_problem()
    return {"random37": np.random.default_rng(3).choice(len(X), 37, replace=False).astype(np.int64),
            "rows120_260": np.arange(120, 260, dtype=np.int64),
            "level1_of_col2": np.flatnonzero(X[:, 2] == 1.0).astype(np.int64)}


def matern_groups():
    """The groups of the N = 700 table: every fifth row (140), rows 300..559 (m = 260: three block columns of C), the last row."""
    return {"every5th": np.arange(0, N_MATERN, 5, dtype=np.int64), "rows300_560": np.arange(300, 560, dtype=np.int64),
            "last": np.array([N_MATERN - 1], dtype=np.int64)}


class LeaveOut:
    """One problem: its Sigma (jitter included), noise diagonal and -- on first use -- the whole factor and alpha."""

    def __init__(self, spec, theta, X, y):
        self.spec, self.theta = spec, np.asarray(theta, float)
        self.X, self.y = np.asarray(X, float), np.asarray(y, float)
        self.N = len(self.y)
        self.jitter = float(spec["jitter"])
        self.sigma = O.sigma_matrix(spec, self.theta, self.X, dist_mode="direct")
        self.noise = O.noise_diag(spec, self.theta, self.X)
        self._inv = None

    def cond(self):
        return float(np.linalg.cond(self.sigma))

    # ---- the yardstick ----
    def by_deletion(self, rows, with_noise=True):
        """``(mean, cov)`` of the rows ``rows`` (in their order) from all the others: the rows deleted, the rest factored."""
        B = np.asarray(rows, dtype=np.int64).ravel()
        keep = np.setdiff1d(np.arange(self.N), B)
        L = O.cholesky_lower(self.sigma[np.ix_(keep, keep)])
        v = O.solve_lower(L, self.y[keep])
        # Sigma's off-diagonal is K, and its diagonal K + noise + jitter
        A = O.solve_lower(L, self.sigma[np.ix_(keep, B)])
        prior = self.sigma[np.ix_(B, B)].copy()
        prior[np.diag_indices_from(prior)] -= self.jitter + (0.0 if with_noise else self.noise[B])
        return A.T @ v, prior - A.T @ A

    def loo_by_deletion(self, rows, with_noise=True):
        """``(mean, var)`` of each row of ``rows`` left out ALONE (one factorisation per row)."""
        out = [self.by_deletion([i], with_noise) for i in np.asarray(rows, dtype=np.int64).ravel()]
        return np.array([m[0] for m, _ in out]), np.array([c[0, 0] for _, c in out])

    # ---- the closed form (CPU tests only) ----
    def _inverse(self):
        if self._inv is None:
            L = O.cholesky_lower(self.sigma)
            Linv = O.solve_lower(L, np.eye(self.N))
            self._inv = (Linv.T @ Linv, Linv.T @ O.solve_lower(L, self.y))
        return self._inv

    def closed_form(self, rows, with_noise=True):
        """``(mean, cov)`` of the rows from ONE factor of the whole Sigma; the jitter taken off the diagonal."""
        B = np.asarray(rows, dtype=np.int64).ravel()
        Sinv, alpha = self._inverse()
        Cinv = np.linalg.inv(Sinv[np.ix_(B, B)])
        Cinv = 0.5 * (Cinv + Cinv.T)
        cov = Cinv.copy()
        cov[np.diag_indices_from(cov)] -= self.jitter + (0.0 if with_noise else self.noise[B])
        return self.y[B] - Cinv @ alpha[B], cov

    def loo_closed_form(self, with_noise=True):
        """``(mean, var)`` of all N rows: ``y_i - alpha_i / d_i`` and ``1 / d_i - jitter`` (less the noise)."""
        Sinv, alpha = self._inverse()
        d = np.diag(Sinv)
        return self.y - alpha / d, 1.0 / d - self.jitter - (0.0 if with_noise else self.noise)


@functools.lru_cache(maxsize=None)
def problem(name):
    """``LeaveOut`` of ``"three_term"``, ``"matern"`` (sigma = 0.25) or ``"matern_illcond"`` (sigma = 0.02), computed once."""
    if name == "three_term":
        return LeaveOut(*three_term_problem())
    return LeaveOut(*matern_problem(0.25 if name == "matern" else 0.02))


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def loo_reference(name, with_noise=True):
    """Leave-one-out by deletion of EVERY row of the problem (N factorisations, made once: the noise-free variances are the same
    deletions' with the row's noise taken off; shared by the tests, read-only)."""
    if not with_noise:
        mean, var = loo_reference(name, True)
        return mean, _frozen(var - problem(name).noise)
    mean, var = problem(name).loo_by_deletion(np.arange(problem(name).N), True)
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


class LeaveOutOracleEngine(OracleEngine):
    """The numpy stand-in of ``gumbi_amd.engine.Engine`` with the two leave-out calls, by deletion (test infrastructure: the front
    end's CPU tests monkeypatch it in)."""

    def _problem(self):
        return LeaveOut(self.spec, self.theta, self.X, self.y)

    def loo(self, rows=None, with_noise=True):
        start, stop = (0, len(self.y)) if rows is None else rows
        return self._problem().loo_by_deletion(np.arange(start, stop), with_noise)

    def leave_out(self, idx, with_noise=True, cov=False):
        mean, full = self._problem().by_deletion(idx, with_noise)
        return (mean, np.diag(full).copy(), full) if cov else (mean, np.diag(full).copy())


def use_leave_out_oracle(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", LeaveOutOracleEngine)
    monkeypatch.setattr(icm, "Engine", LeaveOutOracleEngine)
