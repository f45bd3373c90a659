"""A numpy restatement of what ``gmb_append`` / ``gmb_truncate`` must compute, sharing no code with the engine.

Row i of a Cholesky factor depends on rows <= i of Sigma only, so K further observations keep the factor of the first N and add

    L' = [ L   0  ]      P  = Sigma[new, old] L^-T            (K x N)
         [ P   L* ]      L* = chol(Sigma[new, new] - P P^T)    (K x K)
    v' = [ v ; L*^-1 (y_new - P v) ]
    log det' = log det + sum log L*_ii

``bordered_update`` is that algebra on plain arrays; ``append`` applies it to a model of oracle/gp_oracle.py; ``blocked_append``
restates the ENGINE's route -- keep the block columns [0, I0) with I0 = floor(min(N_old, N_new) / 128), rebuild every row from
128 I0 on -- so that the choice of I0 (a partial last block is factored again, not patched) is pinned on the CPU as well.
tests/test_append_cpu.py holds all three against ``O.factorize`` at N + K.  ``AppendOracleEngine`` is the stand-in engine of the
front-end tests: ``append`` / ``truncate`` by concatenation, counting its calls.
"""
import numpy as np

from oracle import gp_oracle as O

TILE = 128


def bordered_update(L, v, S_cross, S_new, y_new):
    """(L', v', sum log diag L*) from the factor (L, v) of the old block, S_cross = Sigma[new, old], S_new = Sigma[new, new]."""
    L = np.asarray(L, float)
    P = O.solve_lower(L, np.asarray(S_cross, float).T).T if L.shape[0] else np.zeros((S_new.shape[0], 0))
    Ls = O.cholesky_lower(np.asarray(S_new, float) - P @ P.T)
    N, K = L.shape[0], Ls.shape[0]
    L2 = np.zeros((N + K, N + K))
    L2[:N, :N] = np.tril(L)
    L2[N:, :N] = P
    L2[N:, N:] = np.tril(Ls)
    v2 = np.concatenate([v, O.solve_lower(Ls, np.asarray(y_new, float) - P @ v)])
    return L2, v2, float(np.sum(np.log(np.diag(Ls))))


def append(spec, theta, X, y, Xn, yn, dist_mode="direct"):
    """Factor of (X, y), then the bordered update with (Xn, yn): (L', v', nlml')."""
    N = len(y)
    L, v = O.factorize(spec, theta, X, y, dist_mode=dist_mode)
    S = O.sigma_matrix(spec, theta, np.vstack([X, Xn]), dist_mode=dist_mode)
    L2, v2, ld_new = bordered_update(L, v, S[N:, :N], S[N:, N:], yn)
    nlml = 0.5 * len(v2) * np.log(2.0 * np.pi) + np.sum(np.log(np.diag(L))) + ld_new + 0.5 * float(v2 @ v2)
    return L2, v2, nlml


def blocked_append(spec, theta, X_all, y_all, N_old, N_new, dist_mode="direct"):
    """The engine's route from a factor at N_old to one at N_new (larger or smaller): rows from 128 I0 on are rebuilt."""
    I0 = min(N_old, N_new) // TILE
    keep = I0 * TILE
    L_old, v_old = O.factorize(spec, theta, X_all[:N_old], y_all[:N_old], dist_mode=dist_mode)
    S = O.sigma_matrix(spec, theta, X_all[:N_new], dist_mode=dist_mode)
    L2, v2, _ = bordered_update(L_old[:keep, :keep], v_old[:keep], S[keep:, :keep], S[keep:, keep:], y_all[keep:N_new])
    return L2, v2, I0


def layout(N):
    """(Np, Nr): columns and rows of the bordered factor buffer, padded to 128 (row N carries y)."""
    return -(-N // TILE) * TILE, -(-(N + 1) // TILE) * TILE


class AppendOracleEngine:
    """Mixin over an oracle engine of the front-end tests (``set_data`` keeps ``X`` and ``y``): ``append`` and ``truncate`` by
    concatenation -- what the HIP engine's calls must be equivalent to -- with call counters."""

    appends = 0
    truncates = 0
    log = None

    def append(self, X, y):
        X = np.asarray(X, float)
        y = np.asarray(y, float)
        if X.ndim != 2 or X.shape[1] != self.X.shape[1] or y.shape != (X.shape[0],):
            raise ValueError("append: bad shapes")
        type(self).appends += 1
        if type(self).log is not None:
            type(self).log.append(("append", X.copy(), y.copy()))
        factored = self._factored  # (the engine's contract: a valid factor stays valid)
        self.set_data(np.vstack([self.X, X]), np.concatenate([self.y, y]))
        self._factored = factored

    def truncate(self, n):
        n = int(n)
        if not 1 <= n <= len(self.y):
            raise ValueError("truncate: n out of range")
        type(self).truncates += 1
        if type(self).log is not None:
            type(self).log.append(("truncate", n))
        factored = self._factored
        self.set_data(self.X[:n], self.y[:n])
        self._factored = factored
