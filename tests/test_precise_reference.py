"""The extended-precision reference of the conditioning tests (tests/precise_reference.py) against mpmath at 40 digits and
against the float64 oracle.  CPU only."""
import mpmath as mp
import numpy as np
import pytest

import precise_reference as P
from oracle import gp_oracle as O


def _mp_lower(L, b):
    x = []
    for i in range(L.rows):
        x.append((b[i] - mp.fsum(L[i, k] * x[k] for k in range(i))) / L[i, i])
    return x


def _mp_upper_t(L, b):
    n = L.rows
    x = [mp.mpf(0)] * n
    for i in reversed(range(n)):
        x[i] = (b[i] - mp.fsum(L[k, i] * x[k] for k in range(i + 1, n))) / L[i, i]
    return x


def _ill_case(N=60):
    rng = np.random.default_rng(0)
    X = np.sort(rng.uniform(-2, 2, N))[:, None]
    y = np.sin(3 * X[:, 0])
    spec = O.make_spec(1, [0], kind="ExpQuad")
    theta = O.pack_theta(spec, [0.5], 3.0, 1e-9)  # jitter-limited
    Xs = np.vstack([X[::6] + 1e-3, np.linspace(-2.2, 2.2, 9)[:, None]])
    return spec, theta, X, y, Xs


def test_reference_matches_mpmath_on_an_ill_conditioned_sigma():
    """N = 60, cond(Sigma) ~ 1e8 - 1e9: every quantity against a 40-digit mpmath solve of the same float64 problem.  The
    posterior mean / variance, log det and NLML agree to ~1e-15 relative (the float64 rounding of the result); alpha, whose
    own condition number is cond(Sigma), to ~cond eps_longdouble: 2e-12 relative, 600 times closer than the float64 host's
1e-9.  The bars leave a factor of ~5 on what was measured."""
    spec, theta, X, y, Xs = _ill_case()
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    assert np.linalg.cond(S) > 1e8
    ref = P.posterior(spec, theta, X, y, Xs, grad=True)
    host = P.host_float64(spec, theta, X, y, Xs)
    N = len(y)
    with mp.workdps(40):
        Lm = mp.cholesky(mp.matrix(S.tolist()))
        v = _mp_lower(Lm, [mp.mpf(float(a)) for a in y])
        al = _mp_upper_t(Lm, v)
        Kxs = O.cov_full(spec, theta, X, Xs, dist_mode="direct")
        kss = O.cov_diag(spec, theta, Xs)
        mean = np.array([float(mp.fsum(mp.mpf(float(Kxs[i, j])) * al[i] for i in range(N))) for j in range(len(Xs))])
        var = []
        for j in range(len(Xs)):
            a = _mp_lower(Lm, [mp.mpf(float(Kxs[i, j])) for i in range(N)])
            var.append(float(mp.mpf(float(kss[j])) - mp.fsum(x * x for x in a)))
        var = np.array(var)
        logdet = float(2 * mp.fsum(mp.log(Lm[i, i]) for i in range(N)))
        nlml = float(mp.mpf(N) / 2 * mp.log(2 * mp.pi) + mp.mpf(logdet) / 2 + mp.fsum(x * x for x in v) / 2)
        Sinv = mp.inverse(mp.matrix(S.tolist()))
        sinv00 = float(Sinv[0, 0])
    alpha = np.array([float(a) for a in al])
    assert np.max(np.abs(np.asarray(ref["mean"], float) - mean)) < 1e-14 * np.max(np.abs(mean))
    assert np.max(np.abs(np.asarray(ref["var"], float) - var)) < 1e-15 * np.max(kss)
    assert abs(float(ref["logdet"]) - logdet) < 1e-14 * abs(logdet)
    assert abs(float(ref["nlml"]) - nlml) < 1e-14 * abs(nlml)
    err_a = np.max(np.abs(np.asarray(ref["alpha"], float) - alpha))
    assert err_a < 1e-2 * np.max(np.abs(host["alpha"] - alpha))
    assert err_a < 1e4 * np.finfo(np.longdouble).eps * np.linalg.cond(S) * np.max(np.abs(alpha))
    assert abs(float(ref["Sinv"][0, 0]) - sinv00) < 1e-3 * abs(sinv00) * np.finfo(float).eps * np.linalg.cond(S)


@pytest.mark.parametrize("kind", ["ExpQuad", "Matern32"])
def test_reference_matches_float64_oracle_when_well_conditioned(kind):
    X, y, ls = O.synthetic_table(150, 2, seed=4)
    spec = O.make_spec(2, [0, 1], kind=kind)
    theta = O.pack_theta(spec, ls, 1.1, 0.3)
    Xs = np.random.default_rng(1).standard_normal((40, 2))
    ref = P.posterior(spec, theta, X, y, Xs, grad=True)
    mu, var = O.predict(spec, theta, X, y, Xs, with_noise=True, dist_mode="direct")
    _, var0 = O.predict(spec, theta, X, y, Xs, with_noise=False, dist_mode="direct")
    val, g = O.nlml_and_grad(spec, theta, X, y)
    L, v = O.factorize(spec, theta, X, y, dist_mode="direct")

    def rel(a, b):
        return np.max(np.abs(np.asarray(a, float) - b)) / np.max(np.abs(b))

    assert rel(ref["mean"], mu) < 1e-12 and rel(ref["var_noise"], var) < 1e-12 and rel(ref["var"], var0) < 1e-12
    assert rel(ref["nlml"], val) < 1e-12 and rel(ref["grad"], g) < 1e-12
    assert rel(ref["L"], L) < 1e-12 and rel(ref["v"], v) < 1e-12
    assert rel(ref["alpha"], np.linalg.solve(O.sigma_matrix(spec, theta, X, dist_mode="direct"), y)) < 1e-12


def test_grad_given_m_is_the_second_half_of_nlml_and_grad():
    X, y, ls = O.synthetic_table(80, 3, seed=2)
    spec = O.make_spec(3, [0, 1, 2], kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    Sinv = np.linalg.inv(S)
    a = Sinv @ y
    g = O.grad_given_M(spec, theta, X, 0.5 * (Sinv - np.outer(a, a)))
    assert np.allclose(g, O.nlml_and_grad(spec, theta, X, y)[1], rtol=1e-9, atol=1e-9)
