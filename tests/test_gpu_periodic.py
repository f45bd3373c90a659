"""Periodic kernels on the MI355X (``gmb_set_periodic``; reference gumbi/regression/pymc/GP.py:416-447, 664-682) against the
numpy reference of tests/periodic_reference.py.  Needs a GPU (``-m gpu``).

Tolerances are the project's own bars for the corresponding checks, copied from where they are stated:

* covariance entrywise (tests/test_gpu_parity.py::test_covariance_build_matches_oracle_entrywise): ``16 eps eta^2`` for the
  kinds with a kink at r = 0 (direct differences on every tile), ``40 eps max(1, max |x/ls|^2) eta^2`` for the smooth kinds
  (the expansion's rounding scales with the squared norm of the scaled point -- here the warped point, ``sum_d 1/ls_d^2`` for
  ``<kind>+Periodic`` and a quarter of it for ``Periodic``);
* NLML 1e-10 relative, gradient 1e-8 relative to its largest entry, prediction mean 1e-10 / variance 1e-11 against the oracle's
  direct-distance mode (test_gpu_parity.py:397, 748, 752), the two prediction forms 1e-11 / 1e-12 apart (:331);
* joint covariance 1e-9 absolute, its mean 1e-8 relative, well-conditioned draws 1e-8 relative (tests/test_gpu_joint.py:6-12);
* Kronecker against stacked: NLML rtol 1e-10 / atol 1e-9, gradient 1e-7, predictions 1e-8 (tests/test_gpu_frontend.py:301-314).
"""
import numpy as np
import pytest

import periodic_reference as PR
from oracle import gp_oracle as O
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

FORMS = [("ExpQuad", 2)] + [(k, 1) for k in O.KINDS]  # "Periodic" and the five "<kind>+Periodic"
EPS = np.finfo(float).eps


def kspec(spec, mode, periods):
    from gumbi_amd.engine import KernelSpec

    return KernelSpec(D=spec["D"], idx_cont=spec["idx_cont"], kind=spec["kind"], ard=spec["ard"], idx_lin=spec["idx_lin"],
                      coreg=spec["coreg"], out_col=spec["out_col"], n_out=spec["n_out"], hetero_noise=spec["hetero_noise"],
                      jitter=spec["jitter"], additive=spec.get("additive", False), periodic=mode, periods=list(periods))


def make_engine(spec, mode, periods, theta, X, y):
    from gumbi_amd.engine import Engine

    eng = Engine(0)
    eng.set_data(X, y)
    eng.set_kernel(kspec(spec, mode, periods))
    eng.set_theta(theta)
    return eng


def case(kind, mode, N, d, ard=True, seed=0):
    rng = np.random.default_rng(1000 * d + N + seed)
    X = rng.standard_normal((N, d))
    periods = rng.uniform(2.5, 4.0, d)
    ls = rng.uniform(0.8, 1.6, d)
    f = sum(np.sin(2 * np.pi * X[:, k] / periods[k] + k) for k in range(d))
    y = f + 0.2 * rng.standard_normal(N)
    spec = O.make_spec(d, range(d), kind=kind, ard=ard)
    theta = O.pack_theta(spec, ls if ard else ls[:1], 1.3, 0.25)
    return spec, theta, X, y, periods


# ---- covariance build -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", FORMS)
@pytest.mark.parametrize("ard", [True, False])
@pytest.mark.parametrize("N,d", [(100, 1), (515, 1), (640, 2), (700, 3), (1300, 8)])  # one tile .. 11 tile rows; nc_pad 2, 4, 8, 16
def test_covariance_build_matches_reference_entrywise(gpu, kind, mode, ard, N, d):
    import torch

    spec, theta, X, y, periods = case(kind, mode, N, d, ard)
    w = PR.Warped(spec, mode, periods)
    eng = make_engine(spec, mode, periods, theta, X, y)
    Nr, Np = (N + 1 + 127) // 128 * 128, (N + 127) // 128 * 128
    out = torch.full((Np, Nr), float("nan"), dtype=torch.float64, device="cuda:0")  # column-major Nr x Np
    torch.cuda.synchronize()
    eng.blk_covariance(out.data_ptr(), Nr)
    S = out.cpu().numpy().T
    S_ref = w.sigma(theta, X)
    low = np.tril(np.ones((N, N), bool))
    err = float(np.max(np.abs(S[:N, :N][low] - S_ref[low])))
    if kind in ("Matern12", "Exponential"):
        tol = 16 * EPS * 1.3**2
    else:
        Xw = w.X(X)[:, : 2 * d] / w.theta(theta)[: (2 * d if ard else 1)]
        scale2 = float(np.max(np.sum(Xw**2, axis=1)))
        tol = 40 * EPS * max(1.0, scale2) * 1.3**2
    print(f"cov {kind} mode {mode} ard {ard} N {N} d {d}: max err {err:.3e} (tol {tol:.3e})")
    assert err < tol
    # the direct restatement of the PyMC formula (for <kind>+Periodic: the reference's own form at d = 1, the per-dimension form beyond)
    ls = np.broadcast_to(theta[: (d if ard else 1)], (d,))
    K_dir = PR.direct_cov(kind, mode, ls, 1.3, periods, X)
    off = ~np.eye(N, dtype=bool) & low
    # (+ 1e-13: the bound between the warped reference and this restatement, tests/test_periodic_cpu.py::
    # test_warped_oracle_is_the_pymc_formula -- the bar above is the engine against the warped reference, two references apart
    # by up to 1e-13 cannot both be met to 6e-15)
    assert np.max(np.abs(S[:N, :N][off] - K_dir[off])) < tol + 1e-13
    # y row and identity padding
    assert np.array_equal(S[N, :N], y)
    assert np.array_equal(np.tril(S[N:, N:Np]), np.tril(np.eye(Nr - N, Np - N)))
    eng.close()


# ---- NLML, gradient, prediction ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", FORMS)
@pytest.mark.parametrize("ard", [True, False])
@pytest.mark.parametrize("scheme", ["tiles", "launch_tree"])
def test_evaluate_and_predict_match_reference(gpu, kind, mode, ard, scheme):
    N, d = 700, 3
    spec, theta, X, y, periods = case(kind, mode, N, d, ard, seed=7)
    w = PR.Warped(spec, mode, periods)
    eng = make_engine(spec, mode, periods, theta, X, y)
    if scheme == "launch_tree":
        eng.set_chol_scheme(eng.CHOL_RECURSION)
        eng.set_grad_scheme(eng.GRAD_LAUNCH_TREE)
    val_r, grad_r = w.nlml_and_grad(theta, X, y)
    val, grad = eng.evaluate(theta)
    print(f"evaluate {kind} mode {mode} ard {ard} {scheme}: nlml rel {abs(val - val_r) / abs(val_r):.2e} grad rel {rel(grad, grad_r):.2e}")
    assert abs(val - val_r) < 1e-10 * max(1.0, abs(val_r)) and rel(grad, grad_r) < 1e-8
    val2, grad2 = eng.evaluate(theta)
    assert val2 == val and grad2.tobytes() == grad.tobytes()  # run to run: the same bits
    # the separate calls agree with the fused one
    eng.set_theta(theta)
    eng.factorize()
    val3, grad3 = eng.nlml(grad=True)
    assert abs(val3 - val_r) < 1e-10 * max(1.0, abs(val_r)) and rel(grad3, grad_r) < 1e-8
    # predictions: both forms, with and without noise; exact repetition with the period
    Xs = np.random.default_rng(3).standard_normal((333, d)) * 1.5
    eng.evaluate(theta)  # (leaves the inverse factor on the tile path: form 1 is then the product form)
    res = {}
    for form in (0, 1):
        eng.set_predict_form(form)
        for with_noise in (True, False):
            mu, var = eng.predict(Xs, with_noise=with_noise)
            mu_r, var_r = w.predict(theta, X, y, Xs, with_noise=with_noise)
            print(f"  predict form {form} noise {with_noise}: mean rel {rel(mu, mu_r):.2e} var abs {np.max(np.abs(var - var_r)):.2e}")
            assert rel(mu, mu_r) < 1e-10 and np.max(np.abs(var - var_r)) < 1e-11
            res[form, with_noise] = (mu, var)
            mu_b, var_b = eng.predict(Xs, with_noise=with_noise)
            assert mu_b.tobytes() == mu.tobytes() and var_b.tobytes() == var.tobytes()
    for with_noise in (True, False):
        (m0, v0), (m1, v1) = res[0, with_noise], res[1, with_noise]
        assert rel(m1, m0) < 1e-11 and np.max(np.abs(v1 - v0)) < 1e-12
    for k in (1, -2, 3):
        shift = k * periods * np.array([1.0, 0.0, 1.0])[:d]
        mu_k, var_k = eng.predict(Xs + shift, with_noise=True)
        mu, var = res[1, True]
        assert np.max(np.abs(mu_k - mu)) <= 1e-9 and np.max(np.abs(var_k - var)) <= 1e-9
    eng.close()


@pytest.mark.parametrize("kind,mode,N,d", [("ExpQuad", 2, 2304, 2), ("Matern52", 1, 2321, 4), ("Matern12", 1, 1153, 1)])
def test_larger_matrices_on_the_interior_tiles(gpu, kind, mode, N, d):
    """18 block columns: most tiles of the covariance build and of the gradient's trace reduction run on the matrix pipe
    (the split reduction folds its 2 n_cont column sums like the direct one)."""
    spec, theta, X, y, periods = case(kind, mode, N, d, seed=11)
    w = PR.Warped(spec, mode, periods)
    eng = make_engine(spec, mode, periods, theta, X, y)
    val_r, grad_r = w.nlml_and_grad(theta, X, y)
    val, grad = eng.evaluate(theta)
    print(f"evaluate {kind} mode {mode} N {N} d {d}: nlml rel {abs(val - val_r) / abs(val_r):.2e} grad rel {rel(grad, grad_r):.2e}")
    assert abs(val - val_r) < 1e-10 * max(1.0, abs(val_r)) and rel(grad, grad_r) < 1e-8
    Xs = np.random.default_rng(5).standard_normal((1500, d))
    mu, var = eng.predict(Xs)
    mu_r, var_r = w.predict(theta, X, y, Xs)
    assert rel(mu, mu_r) < 1e-10 and np.max(np.abs(var - var_r)) < 1e-11
    eng.close()


# ---- joint posterior --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mode", [("ExpQuad", 2), ("Matern52", 1), ("Exponential", 1)])
def test_joint_covariance_and_draws_match_reference(gpu, kind, mode):
    N, d, M = 600, 2, 150
    spec, theta, X, y, periods = case(kind, mode, N, d, seed=13)
    w = PR.Warped(spec, mode, periods)
    eng = make_engine(spec, mode, periods, theta, X, y)
    eng.factorize()
    Xs = np.random.default_rng(17).standard_normal((M, d)) * 1.5
    for with_noise in (True, False):
        jitter = 0.0 if with_noise else 1e-6
        mean, cov = eng.predict_joint(Xs, with_noise=with_noise, jitter=jitter)
        mean_r, cov_r = w.predict_joint(theta, X, y, Xs, with_noise=with_noise, jitter=jitter)
        assert np.array_equal(cov, cov.T)
        assert np.max(np.abs(cov - cov_r)) <= 1e-9 and np.max(np.abs(mean - mean_r)) <= 1e-8 * np.max(np.abs(mean_r))
        # diag(cov) against gmb_predict's variance.  The two differ BY THE REFERENCE'S OWN FORMULAS for the kinds that take
        # sqrt(r^2 + 1e-12): the full covariance evaluates the kind at r^2 = 0 (pm.gp.cov.Stationary.full: k(sqrt(1e-12)) < 1, what
        # cov_r holds), the marginal variance takes pm.gp.cov.Stationary.diag = 1 exactly -- eta^2 (k(0) - 1) = -8.4e-7 for
        # Exponential, -1.9e-12 for Matern-5/2, 0 for ExpQuad.  That offset is taken out; what is left is held to the bar
        # tests/test_gpu_joint.py sets between the engine's two forms.
        mu, var = eng.predict(Xs, with_noise=with_noise)
        offset = 1.3**2 * (float(O.stationary_from_r2(spec["kind"], np.zeros(1))[0]) - 1.0)
        gap = float(np.max(np.abs(np.diag(cov) - jitter - var - offset)))
        print(f"joint {kind} mode {mode} noise {with_noise}: |diag(cov) - var - offset| = {gap:.2e} (offset {offset:.3e})")
        assert gap <= 1e-11
    Z = np.random.default_rng(19).standard_normal((8, M))
    Y = eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0)
    Y_r, _, _ = w.draw_joint(theta, X, y, Xs, Z, with_noise=True, jitter=0.0)
    assert Y.shape == (8, M) and np.max(np.abs(Y - Y_r)) <= 1e-8 * np.max(np.abs(Y_r))
    assert eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0).tobytes() == Y.tobytes()
    eng.close()


# ---- additive model, Kronecker path ---------------------------------------------------------------------------------------------
def test_additive_model_matches_reference(gpu):
    rng = np.random.default_rng(23)
    N = 500
    X = np.column_stack([rng.standard_normal((N, 2)), rng.integers(0, 3, N).astype(float)])
    y = np.sin(X[:, 0]) + 0.3 * X[:, 2] + 0.2 * rng.standard_normal(N)
    for kind, mode, ard in (("Matern52", 1, True), ("ExpQuad", 2, False)):
        spec = O.make_spec(3, [0, 1], kind=kind, ard=ard, coreg=[(2, 3)], additive=True)
        n_ls = 2 if ard else 1
        theta = np.concatenate([rng.uniform(0.8, 1.5, n_ls), [1.1, 0.3], rng.standard_normal(6) * 0.5, rng.uniform(0.5, 1.5, 3),
                                rng.uniform(0.8, 1.5, n_ls), [0.7]])
        assert theta.size == O.theta_size(spec)
        periods = [3.0, 2.6]
        w = PR.Warped(spec, mode, periods)
        eng = make_engine(spec, mode, periods, theta, X, y)
        val_r, grad_r = w.nlml_and_grad(theta, X, y)
        val, grad = eng.evaluate(theta)
        print(f"additive {kind} mode {mode}: nlml rel {abs(val - val_r) / abs(val_r):.2e} grad rel {rel(grad, grad_r):.2e}")
        assert abs(val - val_r) < 1e-10 * max(1.0, abs(val_r)) and rel(grad, grad_r) < 1e-8
        Xs = np.column_stack([rng.standard_normal((200, 2)) * 1.5, rng.integers(0, 3, 200).astype(float)])
        mu, var = eng.predict(Xs)
        mu_r, var_r = w.predict(theta, X, y, Xs)
        assert rel(mu, mu_r) < 1e-10 and np.max(np.abs(var - var_r)) < 1e-11
        eng.close()


def test_kronecker_path_equals_the_stacked_engine(gpu):
    from gumbi_amd.regression.icm import IcmEngine

    rng = np.random.default_rng(29)
    N, P = 300, 2
    Xn = rng.standard_normal((N, 1))
    X = np.vstack([np.column_stack([Xn, np.full(N, p, float)]) for p in range(P)])
    y = np.concatenate([np.sin(2 * np.pi * Xn[:, 0] / 2.7 + p) + 0.2 * rng.standard_normal(N) for p in range(P)])
    periods = [2.7]
    for kind, mode in (("Matern32", 1), ("ExpQuad", 2)):
        spec = O.make_spec(2, [0], kind=kind, out_col=1, n_out=P, hetero_noise=True)
        theta = np.concatenate([[1.1, 1.2, 0.3], rng.standard_normal(2 * P) * 0.7, rng.uniform(0.5, 1.5, P),
                                rng.standard_normal(2 * P) * 0.7, rng.uniform(0.5, 1.5, P)])
        assert theta.size == O.theta_size(spec)
        ks = kspec(spec, mode, periods)
        kron = IcmEngine(device=0)
        kron.set_data(X, y)
        kron.set_kernel(ks)
        stacked = make_engine(spec, mode, periods, theta, X, y)
        kron.set_theta(theta)
        kron.factorize()
        stacked.factorize()
        vk, gk = kron.nlml(grad=True)
        vs, gs = stacked.nlml(grad=True)
        assert np.isclose(vk, vs, rtol=1e-10, atol=1e-9)
        assert np.max(np.abs(gk - gs)) < 1e-7 * max(1.0, np.max(np.abs(gs)))
        w = PR.Warped(spec, mode, periods)
        val_r, grad_r = w.nlml_and_grad(theta, X, y)
        assert abs(vs - val_r) < 1e-10 * max(1.0, abs(val_r)) and rel(gs, grad_r) < 1e-8
        pts = np.column_stack([rng.standard_normal(80) * 1.5, rng.integers(0, P, 80).astype(float)])
        for with_noise in (True, False):
            mk, vk2 = kron.predict(pts, with_noise=with_noise)
            ms, vs2 = stacked.predict(pts, with_noise=with_noise)
            assert np.max(np.abs(mk - ms)) < 1e-8 * max(1.0, np.max(np.abs(ms)))
            assert np.max(np.abs(vk2 - vs2)) < 1e-8 * max(1.0, np.max(np.abs(vs2)))
        shifted = pts.copy()
        shifted[:, 0] += 2 * periods[0]
        mk2, vk3 = kron.predict(shifted, with_noise=False)
        assert np.max(np.abs(mk2 - mk)) <= 1e-9 and np.max(np.abs(vk3 - vk2)) <= 1e-9
        kron.close()
        stacked.close()


# ---- the switch itself ----------------------------------------------------------------------------------------------------
def test_mode_off_is_bit_identical_to_never_calling_it(gpu):
    from gumbi_amd.engine import Engine, KernelSpec

    N, d = 700, 3
    X, y, ls = O.synthetic_table(N, d, seed=5)
    spec = O.make_spec(d, range(d), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.1, 0.25)
    Xs = np.random.default_rng(1).standard_normal((200, d))
    got = []
    for variant in ("never", "off", "on_then_off", "on_then_set_kernel"):
        eng = Engine(0)
        eng.set_data(X, y)
        ks = KernelSpec(D=d, idx_cont=list(range(d)), kind="Matern52")
        eng.set_kernel(ks)
        if variant == "off":
            eng.set_periodic(0, np.ones(d))
        elif variant == "on_then_off":
            eng.set_periodic(1, [2.0, 3.0, 4.0])
            eng.set_periodic(0, [2.0, 3.0, 4.0])
        elif variant == "on_then_set_kernel":
            eng.set_periodic(1, [2.0, 3.0, 4.0])
            eng.set_kernel(ks)  # resets the mode
        val, grad = eng.evaluate(theta)
        mu, var = eng.predict(Xs)
        got.append((val, grad.tobytes(), mu.tobytes(), var.tobytes()))
        eng.close()
    assert all(g == got[0] for g in got[1:])
    val_r, grad_r = O.nlml_and_grad(spec, theta, X, y)
    assert abs(got[0][0] - val_r) < 1e-10 * abs(val_r)


def test_set_periodic_invalidates_theta_and_the_factor(gpu):
    spec, theta, X, y, periods = case("Matern32", 1, 300, 2)
    eng = make_engine(spec, 1, periods, theta, X, y)
    eng.factorize()
    assert eng.factor_is_current()
    eng.set_periodic(1, periods * 1.5)
    assert not eng.factor_is_current()
    with pytest.raises(ValueError):
        eng.factorize()  # theta's prepared coordinates belong to the previous periods: set_theta first
    eng.set_theta(theta)
    eng.factorize()
    w = PR.Warped(spec, 1, periods * 1.5)
    val_r = w.nlml(theta, X, y)
    assert abs(eng.nlml() - val_r) < 1e-10 * max(1.0, abs(val_r))
    eng.close()


def test_set_periodic_refuses_bad_arguments(gpu):
    from gumbi_amd.engine import Engine, KernelSpec

    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((50, 9)), rng.standard_normal(50)
    eng = Engine(0)
    with pytest.raises(ValueError):
        eng.set_periodic(1, [1.0])  # no kernel yet
    eng.set_data(X, y)
    eng.set_kernel(KernelSpec(D=9, idx_cont=[0, 1], kind="Matern52"))
    for bad in ([2.0, 0.0], [2.0, -1.0], [np.nan, 2.0], [np.inf, 2.0]):
        with pytest.raises(ValueError, match="period"):
            eng.set_periodic(1, bad)
    for wrong_n in ([2.0], [2.0, 3.0, 4.0], []):
        with pytest.raises(ValueError):
            eng.set_periodic(1, wrong_n)
    with pytest.raises(ValueError):
        eng.set_periodic(3, [2.0, 3.0])
    with pytest.raises(ValueError, match="ExpQuad"):
        eng.set_periodic(2, [2.0, 3.0])  # pm.gp.cov.Periodic is ExpQuad on the warped inputs
    eng.set_periodic(1, [2.0, 3.0])
    eng.set_kernel(KernelSpec(D=9, idx_cont=[0, 1], kind="ExpQuad"))
    eng.set_periodic(2, [2.0, 3.0])
    eng.set_kernel(KernelSpec(D=9, idx_cont=list(range(9)), kind="ExpQuad"))
    for mode in (1, 2):
        with pytest.raises(ValueError, match="at most 8"):
            eng.set_periodic(mode, np.full(9, 2.0))
    eng.set_periodic(0, np.full(9, 2.0))  # off: nine dimensions are an ordinary model
    with pytest.raises(ValueError):
        KernelSpec(D=9, idx_cont=list(range(9)), kind="ExpQuad", periodic=1, periods=[2.0] * 9).to_c()
    eng.close()
