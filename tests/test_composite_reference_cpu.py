"""tests/composite_reference.py against the float64 oracle and the longdouble solves, on every structure of
tests/test_gpu_composite_limits.py: the closed-form dSigma / dtheta against central differences of ``O.sigma_matrix``, its
longdouble contraction against the oracle's own chain rule, the coverage the problems promise, and the float64 host path's
error in units of the per-component floor the GPU bar is built on."""
import numpy as np
import pytest

import composite_reference as CR
from oracle import gp_oracle as O

EPS = np.finfo(float).eps
CASES = list(CR.CASES)


@pytest.mark.parametrize("case", CASES)
def test_dsigma_matches_central_differences_of_the_oracle(case):
    """Every parameter of every structure (on every third row of the table: the structure, not the size, is under test).

    D(h) = (Sigma(theta + h e_p) - Sigma(theta - h e_p)) / 2h = dSigma/dtheta_p + h^2/6 Sigma''' + O(h^4) + rounding.
    Rounding: an entry of Sigma is a product of at most seven factors behind one exp and one sqrt, good to ~8 eps |Sigma|, so
    the quotient carries at most 8 eps max|Sigma| / h.  Truncation: Sigma is linear in tau and kappa and quadratic in eta,
    sigma, c and W, so it vanishes for all but the lengthscales; there the h^2 coefficient is measured from the oracle itself by
    doubling the step, D(2h) - D(h) = h^2/2 Sigma''' + O(h^4), i.e. the truncation of D(h) is |D(2h) - D(h)| / 3 -- allowed
    twice over for the h^4 term.  h = 1e-5 max(1, |theta_p|) ~ eps^(1/3) balances the two (both ~1e-10 of entries of order 1);
    a wrong closed form is off by the size of the derivative itself."""
    spec, theta, X, _, _ = CR.case_problem(case)
    X = X[::3]
    smax = np.max(np.abs(O.sigma_matrix(spec, theta, X, dist_mode="direct")))

    def quotient(p, h):
        tp, tm = theta.copy(), theta.copy()
        tp[p] += h
        tm[p] -= h
        h_eff = (tp[p] - tm[p]) / 2  # (the step as the perturbed thetas hold it)
        return (O.sigma_matrix(spec, tp, X, dist_mode="direct") - O.sigma_matrix(spec, tm, X, dist_mode="direct")) / (2 * h_eff)

    names = CR.block_of(spec)
    worst, n = 0.0, 0
    for p, dS in enumerate(CR.dsigma(spec, theta, X)):
        h = 1e-5 * max(1.0, abs(theta[p]))
        D1, D2 = quotient(p, h), quotient(p, 2 * h)
        bar = 2 * np.max(np.abs(D2 - D1)) / 3 + 8 * EPS * smax / h
        err = np.max(np.abs(dS - D1))
        assert err <= bar, (case, names[p], p, err, bar)
        assert np.array_equal(dS, dS.T)
        worst, n = max(worst, err / bar), n + 1
    assert n == theta.size
    print(f"FD {case}: {n} parameters, worst err / bar {worst:.3f}")


@pytest.mark.parametrize("case", CASES)
def test_grad_reference_matches_the_oracle_chain_rule_on_the_longdouble_m(case):
    """precise_reference.posterior(grad=True)["grad"] is the oracle's float64 chain rule on the longdouble M rounded once:
    a different formula (per-table partial sums G, then (G + G^T) W) summing the same terms, so the two agree to the rounding
    of a float64 sum of that size, 8 eps A_p, in EVERY component."""
    ref = CR.reference(case)
    ratio = np.abs(ref["post_grad"] - ref["g"]) / (EPS * ref["A"])
    print(f"CHAIN {case}: worst |oracle - reference| / (eps A_p) = {np.max(ratio):.2f}; |g| {np.min(np.abs(ref['g'])):.2e} .. "
          f"{np.max(np.abs(ref['g'])):.2e}, A_p / |g_p| up to {np.max(ref['A'] / np.abs(ref['g'])):.1e}")
    assert np.all(ratio <= 8.0), CR.worst_by_block(ref["spec"], ratio)
    assert np.all(ref["A"] >= np.abs(ref["g"]))


@pytest.mark.parametrize("case", CASES)
def test_problem_deals_every_level_and_mixed_pairs_inside_and_across_tiles(case):
    spec, theta, X, y, Xs = CR.case_problem(case)
    d, n_lin, levels, n_out, hetero, kind, additive, N = CR.CASES[case]
    assert X.shape == (N, spec["D"]) and y.shape == (N,) and theta.shape == (O.theta_size(spec),)
    assert spec["kind"] == O.KINDS[kind] and len(spec["idx_lin"]) == n_lin and spec["additive"] == additive
    tables = list(spec["coreg"]) + ([(spec["out_col"], spec["n_out"])] if spec["out_col"] >= 0 else [])
    assert [L for _, L in tables] == list(levels) + ([n_out] if n_out else [])
    tile = np.arange(N) // 128
    for col, L in tables:
        c = X[:, col].astype(int)
        assert sorted(set(c)) == list(range(L)) and sorted(set(Xs[:, col].astype(int))) == list(range(L))
        mixed = c[:, None] != c[None, :]
        same_tile = tile[:, None] == tile[None, :]
        assert np.any(mixed & same_tile)
        for t in range(tile[-1] + 1):  # every diagonal tile, and every tile below the diagonal
            for u in range(t):
                assert np.any(mixed[np.ix_(tile == t, tile == u)])
            assert np.any(mixed[np.ix_(tile == t, tile == t)])
    w = np.linalg.eigvalsh(O.sigma_matrix(spec, theta, X, dist_mode="direct"))
    print(f"COND {case}: {w[-1] / w[0]:.3g}")
    assert w[-1] / w[0] < 1e4  # (the problems are meant to be well conditioned: measured 40 .. 1.3e3)


@pytest.mark.parametrize("case", CASES)
def test_float64_host_error_in_units_of_the_floor(case):
    """The GPU bar is K max(e64_p, floor_p) with floor_p >= 4 eps A_p: the host path lies within it by construction, what is
    measured here is how far e64_p stands above eps A_p.  Measured (worst component per block, all structures): every
    kernel and table block <= 3.9 (most <= 0.7) -- 4 eps A_p alone covers the host there; sigma and the noise table 0.7 .. 98,
    growing with cond(Sigma) (sigma 30 at cond 1.2e3 on big9, the noise table 98 at 1.3e3 on additive_big, 5.6 at cond 40 on
    max).  Those blocks contract M with a DIAGONAL matrix, i.e. they read diag(Sigma^-1) and alpha^2 and take the inverse's own
    relative error ~cond eps in full, where the smooth kernel derivatives average it out; A_p knows nothing of that error.  A
    floor of 4 eps A_p is therefore wrong for them, and composite_reference.gradient_floor raises it to the host's worst
    relative error within the block (asserted below: that this is needed in the diagonal blocks only, and that even there
    the host stays below cond eps A_p)."""
    ref = CR.reference(case)
    spec = ref["spec"]
    ratio = ref["e64"] / (EPS * ref["A"])
    by_block = CR.worst_by_block(spec, ratio)
    print(f"E64 {case}: " + "  ".join(f"{b} {r:.2f}" for b, r in by_block.items()))
    w = np.linalg.eigvalsh(O.sigma_matrix(spec, ref["theta"], ref["X"], dist_mode="direct"))
    for b, r in by_block.items():
        # "a few units" wherever dSigma is not diagonal (the host's BLAS may group its sums otherwise on another machine: twice
        # the floor's 4); the diagonal blocks stay below the solve's cond eps
        assert r <= (w[-1] / w[0] if b in ("sigma", "W_noise", "kappa_noise") else 8.0), (case, b, r)
    diagonal = np.array([b in ("sigma", "W_noise", "kappa_noise") for b in CR.block_of(spec)])
    assert np.all(ref["floor"][~diagonal] <= 8 * EPS * ref["A"][~diagonal])
    assert np.all(ref["floor"] >= 4 * EPS * ref["A"]) and np.all(ref["e64"] <= ref["floor"] * (1 + 1e-12))


def test_float64_bar_covers_the_host_against_the_longdouble_reference():
    """composite_reference.float64_bar (the bar of the tests whose reference is the float64 oracle) holds between the host path
    and the longdouble reference on every structure, with room: half of it is the other evaluation's."""
    for case in CASES:
        ref = CR.reference(case)
        M = CR.oracle_m(ref["spec"], ref["theta"], ref["X"], ref["y"])
        bar, A = CR.float64_bar(ref["spec"], ref["theta"], ref["X"], M)
        assert np.all(np.abs(A - ref["A"]) <= 1e-9 * ref["A"])
        assert np.all(ref["e64"] <= bar / 2), case
