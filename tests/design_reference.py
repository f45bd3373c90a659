"""A batch of experiments by greedy integrated variance reduction in numpy on the oracle's building blocks -- what
``gmb_design_batch`` and the front end above it are held against.

The yardstick is the DEFINITION.  ``posterior_rows`` gives ``D0 = C(Xc, [Xc; Xr])``, the first M rows of the latent joint posterior
of the stacked set (group_average_reference's ``_cov`` / ``_factor``: ``O.cov_full``, ``O.cholesky_lower``, ``O.solve_lower``,
``dist_mode="direct"``; no noise, no jitter -- tests/test_design_cpu.py holds it against ``GA.joint_posterior``), ``greedy`` spells
the loop out:

    s_a = D[a, a] + noise_a,   gain_a = sum_r w_r D[a, M + r]^2 / s_a,   c = argmax (lowest index on a tie),
    D[a, p] -= (D[c, a] D[c, p]) (1 / s_c)

and records, for every step, what the GPU tests' bars are made of.  ``by_conditioning`` is the independent route: an oracle GP with
the picked points ADDED to the training set (any y) and its variances at the reference points.

Problems are group_average_reference's names, so the engine set-ups are shared.  Points: background rows of the table (seeded,
with replacement) with the continuous columns jittered; ``M_MAX`` candidates and ``R_MAX`` reference points per problem, of which
a case takes the first M and the first R -- one ``D0`` per problem serves every shape.
"""
import functools

import numpy as np

import group_average_reference as GA
from oracle import gp_oracle as O
from oracle_engine import OracleEngine

DESIGN_CHUNK = 2048  # gumbi_amd/csrc/design_plan.hpp (tests/test_design_cpu.py checks the binding says the same)
PROBLEMS = ["matern", "three_term"]
M_SIZES = [1, 127, 130]                       # below, at and across a 128-row tile; a padded candidate block
R_SIZES = [1, 129, 2 * DESIGN_CHUNK + 1]      # one reference point, a partial tile, three chunks with a ragged last
Q_SIZES = [0, 1, 8]
M_MAX, R_MAX, Q_MAX = max(M_SIZES), max(R_SIZES), max(Q_SIZES)
SEEDS = {"matern": 41, "three_term": 43}      # (chosen so that the gap condition of tests/test_design_cpu.py holds)

problem = GA.problem


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def jittered_rows(name, n, rng, scale=0.35):
    spec, _, X, _ = problem(name)
    rows = X[rng.integers(0, len(X), n)].copy()
    cols = list(spec["idx_cont"])
    rows[:, cols] += scale * rng.standard_normal((n, len(cols)))
    return rows


@functools.lru_cache(maxsize=None)
def points(name):
    """``(Xc, Xr)``: M_MAX candidates and R_MAX reference points of a problem."""
    rng = np.random.default_rng(SEEDS[name])
    return _frozen(jittered_rows(name, M_MAX, rng), jittered_rows(name, R_MAX, rng))


def noise_of(name, Xc, with_noise=True):
    spec, theta, _, _ = problem(name)
    return O.noise_diag(spec, np.asarray(theta, float), Xc) if with_noise else np.zeros(len(Xc))


def posterior_rows(spec, theta, X, y, Xc, Xr):
    """``(D0, var_r)``: M x (M + R) latent posterior covariance of the candidates with the stacked set, and the latent variances
    of the reference points by the prediction's formula ``k** - |V|^2``."""
    theta, X = np.asarray(theta, float), np.asarray(X, float)
    P = np.vstack([Xc, Xr])
    L, _ = GA._factor(spec, theta, X, y)
    V = O.solve_lower(L, GA._cov(spec, theta, None, X, P))
    M = len(Xc)
    D0 = GA._cov(spec, theta, None, np.asarray(Xc, float), P) - V[:, :M].T @ V
    var_r = O.cov_diag(spec, theta, Xr) - np.sum(V[:, M:] ** 2, axis=0)
    return D0, var_r


@functools.lru_cache(maxsize=None)
def full_rows(name):
    """``posterior_rows`` of a problem's whole point sets, computed once and shared read-only."""
    Xc, Xr = points(name)
    return _frozen(*posterior_rows(*problem(name), Xc, Xr))


def rows_of(name, M, R):
    """``(D0, var_r)`` of the first M candidates and the first R reference points."""
    D0, var_r = full_rows(name)
    cols = np.concatenate([np.arange(M), M_MAX + np.arange(R)])
    return D0[:M][:, cols].copy(), var_r[:R].copy()


def eps_c(D0):
    """The suite's joint-posterior bar (tests/test_gpu_joint.py): 1e-9 max(1, max|C|)."""
    return 1e-9 * max(1.0, float(np.max(np.abs(D0))))


def greedy(D0, noise, w, q, allow_repeats=True, same=None):
    """The loop, literally.  Returns a dict: ``picks``, ``gains`` (q each; -1 / 0 once no candidate has a positive finite gain),
    ``score0`` (the step-0 gain of every candidate, 0 for an excluded one), and per step ``bars`` (the GPU tests' bar of the pick's
    gain: ``(1 + 3 t) eps_C (2 sum_p w_p |D_ap| + gain_a) / s_a`` on this D), ``gaps`` (best gain minus the runner-up's;
    ``same[a]`` names candidates that are the SAME point and so tie by construction: they are no runner-up of each other) and
    ``score0_bars`` (the bar of every candidate at step 0)."""
    D = np.array(D0, dtype=np.float64)
    M = D.shape[0]
    w = np.asarray(w, float)
    noise = np.asarray(noise, float)
    mask = np.zeros(M, bool)
    eps = eps_c(D0)
    same = np.arange(M) if same is None else np.asarray(same)
    out = {"picks": np.full(q, -1, np.int64), "gains": np.zeros(q), "bars": np.zeros(q), "gaps": np.full(q, np.inf),
           "score0": None, "score0_bars": None}
    for t in range(max(q, 1)):
        s = np.diag(D[:, :M]) + noise
        with np.errstate(divide="ignore", invalid="ignore"):
            gain = (D[:, M:] ** 2 @ w) / s
            bar = (1 + 3 * t) * eps * (2.0 * (np.abs(D[:, M:]) @ w) + gain) / s
        ok = (s > 0) & np.isfinite(s) & np.isfinite(gain) & ~mask
        if t == 0:
            out["score0"], out["score0_bars"] = np.where(ok, gain, 0.0), np.where(ok, bar, 0.0)
        if q == 0:
            break
        cand = np.where(ok & (gain > 0), gain, -np.inf)
        c = int(np.argmax(cand))  # (the first of equals)
        if not np.isfinite(cand[c]):
            break
        others = cand[same != same[c]]
        out["picks"][t], out["gains"][t], out["bars"][t] = c, gain[c], bar[c]
        out["gaps"][t] = gain[c] - (np.max(others) if len(others) and np.isfinite(np.max(others)) else -np.inf)
        if not allow_repeats:
            mask[c] = True
        row = D[c].copy()
        D -= np.outer(row[:M], row) * (1.0 / s[c])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, M, R, with_noise=True, allow_repeats=True, q=Q_MAX):
    """``(greedy result, ivar0)`` of a case with uniform weights ``1 / R``; a smaller q is a prefix of it."""
    D0, var_r = rows_of(name, M, R)
    w = np.full(R, 1.0 / R)
    return greedy(D0, noise_of(name, points(name)[0][:M], with_noise), w, q, allow_repeats), float(w @ var_r)


DUP_M, DUP_R, DUP_TRAIN = 20, 129, (3, 17)


@functools.lru_cache(maxsize=None)
def duplicates_case(name, with_noise=True):
    """20 candidates of which number 3 is training point 17 and one is an exact copy, at a higher index, of the candidate that
    scores best, against 129 reference points, no repeats: ``(Xc, Xr, greedy result, ivar0, (lo, hi))`` with ``lo < hi`` the two
    copies.  They are the same point, so the reference gives them the same row and column of D0 to the bit (numpy's products need
    not) and names them to ``greedy`` as one (``same``): they tie at step 0, and the lower index is picked."""
    spec, theta, X, y = problem(name)
    Xc, Xr = points(name)
    Xc, Xr = Xc[:DUP_M].copy(), Xr[:DUP_R]
    Xc[DUP_TRAIN[0]] = X[DUP_TRAIN[1]]
    w = np.full(DUP_R, 1.0 / DUP_R)
    best = int(np.argmax(greedy(posterior_rows(spec, theta, X, y, Xc, Xr)[0], noise_of(name, Xc, with_noise), w, 0)["score0"]))
    lo, hi = (best, DUP_M - 1) if best < DUP_M - 1 else (0, best)
    Xc[hi if hi != best else lo] = Xc[best]
    D0, var_r = posterior_rows(spec, theta, X, y, Xc, Xr)
    D0[hi, :] = D0[lo, :]
    D0[:, hi] = D0[:, lo]
    same = np.arange(DUP_M)
    same[hi] = lo
    res = greedy(D0, noise_of(name, Xc, with_noise), w, Q_MAX, allow_repeats=False, same=same)
    return _frozen(Xc)[0], Xr, res, float(w @ var_r), (lo, hi)


def by_conditioning(spec, theta, X, y, Xc, Xr, picks, w):
    """``sum_r w_r var f(x_r)`` of an oracle GP with the picked candidates added to the training set (no y: the variance does
    not depend on it).  The added points carry the model's NOISE and not the training diagonal's jitter: the definition's s_a is
    ``var f + noise``, what a prediction with noise reports, and the jitter (1e-6) is a device of the factorisation, added to the
    diagonal of whatever is factorised -- ``O.predict`` on the grown data set would put it on the new points too, and differ
    from the definition by jitter / s_a, relatively."""
    picks = [int(p) for p in picks if p >= 0]
    theta, Xr = np.asarray(theta, float), np.asarray(Xr, float)
    N = len(X)
    X2 = np.vstack([np.asarray(X, float), np.asarray(Xc, float)[picks]])
    S = O.sigma_matrix(spec, theta, X2, dist_mode="direct")
    new = np.arange(N, len(X2))
    S[new, new] -= spec["jitter"]
    V = O.solve_lower(O.cholesky_lower(S), O.cov_full(spec, theta, X2, Xr, dist_mode="direct"))
    var = O.cov_diag(spec, theta, Xr) - np.sum(V * V, axis=0)
    return float(np.asarray(w, float) @ var)


class DesignOracleEngine(OracleEngine):
    """The numpy stand-in of ``gumbi_amd.engine.Engine`` with ``design_batch``, by the definition (test infrastructure: the front
    end's CPU tests monkeypatch it in)."""

    def design_batch(self, Xc, Xr, q, weights=None, with_noise=True, allow_repeats=True):
        Xc, Xr = np.asarray(Xc, float), np.asarray(Xr, float)
        D0, var_r = posterior_rows(self.spec, self.theta, self.X, self.y, Xc, Xr)
        w = np.full(len(Xr), 1.0 / len(Xr)) if weights is None else np.asarray(weights, float)
        noise = O.noise_diag(self.spec, self.theta, Xc) if with_noise else np.zeros(len(Xc))
        res = greedy(D0, noise, w, int(q), allow_repeats)
        return res["picks"], res["gains"], res["score0"], float(w @ var_r)


def use_design_oracle(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", DesignOracleEngine)
    monkeypatch.setattr(icm, "Engine", DesignOracleEngine)
