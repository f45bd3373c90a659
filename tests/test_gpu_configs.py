"""BASELINE.json configurations beyond C2 on the MI355X: C3 (N = 50k, d = 8, Matern-5/2 ARD) and
C4 (2-output ICM, N = 20k, d = 4 -> stacked 40k x 5), each as a mid-size direct comparison with
the oracle plus size-independent properties at the full size; and ``cross_validate`` (SURVEY
section 8f row 3) end to end."""
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"


def make_engine(spec, theta, X, y):
    from gumbi_amd.engine import Engine, KernelSpec

    eng = Engine(0)
    eng.set_data(X, y)
    eng.set_kernel(KernelSpec(D=spec["D"], idx_cont=spec["idx_cont"], kind=spec["kind"], ard=spec["ard"],
                              idx_lin=spec["idx_lin"], coreg=spec["coreg"], out_col=spec["out_col"],
                              n_out=spec["n_out"], hetero_noise=spec["hetero_noise"]))
    eng.set_theta(theta)
    return eng


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def sampled_rows_check(eng, spec, theta, X, rows):
    """(L L^T)[rows][:, rows] == Sigma[rows][:, rows] using only `rows` of the resident factor."""
    N = X.shape[0]
    Lr = np.stack([eng.copy_factor(int(r), 1, 0, N)[0] for r in rows])
    for a, ra in enumerate(rows):
        Lr[a, ra + 1:] = 0.0
    S = O.cov_full(spec, theta, X[rows], X[rows], dist_mode="direct")
    S[np.diag_indices_from(S)] += O.noise_diag(spec, theta, X[rows]) + spec["jitter"]
    assert rel(Lr @ Lr.T, S) < 1e-10


def icm_problem(n, d, seed=2021):
    """SURVEY.md section 8d C4 generator: same X for both outputs, stacked output-major."""
    rng = np.random.default_rng(seed)
    Xc = rng.standard_normal((n, d))
    ls = np.geomspace(0.7, 2.0, d)
    W = np.array([[1.0, 0.0], [0.6, 0.8]])
    kappa = np.array([0.1, 0.1])
    B = W @ W.T + np.diag(kappa)
    f = np.stack([np.sum(np.sin(Xc / ls + p), axis=1) / np.sqrt(d) for p in range(2)])
    F = np.linalg.cholesky(B) @ f
    noise_sd = 0.2 * np.sqrt(np.array([1.0, 2.25]))
    Y = F + noise_sd[:, None] * rng.standard_normal((2, n))
    X = np.vstack([np.column_stack([Xc, np.full(n, p)]) for p in range(2)])
    y = np.concatenate([(Y[p] - Y[p].mean()) / Y[p].std(ddof=1) for p in range(2)])
    spec = O.make_spec(d + 1, range(d), kind="ExpQuad", out_col=d, n_out=2, hetero_noise=True)
    Wn = np.array([[1.0, 0.0], [1.5, 0.0]])
    theta = O.pack_theta(spec, ls, 1.0, 0.2, W_out=W, kappa_out=kappa, W_noise=Wn, kappa_noise=[1e-3, 1e-3])
    return X, y, spec, theta


def test_c2_full_size_direct_parity_and_dense_grid(gpu):
    """C2 at its full size (N = 10k, d = 4, RBF-ARD) straight against the oracle (one LAPACK Cholesky of
    the 10k x 10k covariance on the host, seconds): NLML, and mean / variance at points sampled from the
    dense M = 20^4 = 160,000 grid over all four dims of SURVEY.md section 8d, which the engine predicts
    in full (M-tiled: the N x M solve never exists as a whole)."""
    import time

    N, d = 10_000, 4
    X, y, ls = O.synthetic_table(N, d)
    spec = O.make_spec(d, range(d))
    sigma = 0.2
    theta = O.pack_theta(spec, ls, 1.0, sigma)
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    g = np.linspace(-2.4, 2.4, 20)
    Xs = np.stack(np.meshgrid(g, g, g, g, indexing="ij"), axis=-1).reshape(-1, d)
    assert Xs.shape == (160_000, 4)
    eng.predict(Xs[:4096])
    t0 = time.perf_counter()
    mu, var = eng.predict(Xs, with_noise=True)
    dt = time.perf_counter() - t0
    assert np.all(np.isfinite(mu)) and np.all(var > sigma**2) and np.all(var <= 1.0 + sigma**2 + 1e-9)
    # N^2 M = 1.6e13 flops; anything below 10 TF/s would mean the M-tiling fell off the MFMA path
    assert float(N) ** 2 * len(Xs) / dt > 1.0e13, dt
    sub = np.random.default_rng(5).choice(len(Xs), 48, replace=False)
    mu_r, var_r = O.predict(spec, theta, X, y, Xs[sub], with_noise=True)
    assert rel(mu[sub], mu_r) < 1e-8 and np.max(np.abs(var[sub] - var_r)) < 1e-9
    # the same points in a different batch composition give the same numbers (tiling independence)
    mu_s, var_s = eng.predict(Xs[sub], with_noise=True)
    assert rel(mu_s, mu[sub]) < 1e-12 and np.max(np.abs(var_s - var[sub])) < 1e-12
    assert np.isclose(eng.nlml(), O.nlml(spec, theta, X, y), rtol=1e-10)
    # the prediction behind a FIT: the last evaluation left the inverse factor resident, K(X*, X) L^-T is one GEMM
    # (csrc/predict_form.hpp) -- same oracle, same tolerances, and 1e-10 from the solve form
    eng.evaluate(theta)
    mu_g, var_g = eng.predict(Xs[:20_000], with_noise=True)
    assert eng.timings()["predict_gemm_form"] == 1
    sub2 = sub[sub < 20_000] if np.any(sub < 20_000) else np.arange(8)
    assert rel(mu_g, mu[:20_000]) < 1e-10 and np.max(np.abs(var_g - var[:20_000])) < 1e-11
    mu_r2, var_r2 = O.predict(spec, theta, X, y, Xs[sub2], with_noise=True)
    assert rel(mu_g[sub2], mu_r2) < 1e-8 and np.max(np.abs(var_g[sub2] - var_r2)) < 1e-9
    eng.close()


def test_c3_midsize_parity(gpu):
    N, d = 4000, 8
    X, y, ls = O.synthetic_table(N, d)
    spec = O.make_spec(d, range(d), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    Xs = O.synthetic_grid(d, res=30)
    mu, var = eng.predict(Xs)
    mu_r, var_r = O.predict(spec, theta, X, y, Xs)  # PyMC-faithful distance expansion
    assert rel(mu, mu_r) < 1e-8 and np.max(np.abs(var - var_r)) < 1e-9
    assert np.isclose(eng.nlml(), O.nlml(spec, theta, X, y), rtol=1e-10)
    val, g = eng.nlml(grad=True)
    _, g_r = O.nlml_and_grad(spec, theta, X, y)
    assert np.max(np.abs(g - g_r)) < 1e-8 * max(1.0, np.max(np.abs(g_r)))


def test_c3_full_size_properties(gpu):
    """N = 50k, d = 8, Matern-5/2 ARD: 20 GB factor on one GPU."""
    N, d = 50_000, 8
    X, y, ls = O.synthetic_table(N, d)
    spec = O.make_spec(d, range(d), kind="Matern52")
    sigma = 0.2
    theta = O.pack_theta(spec, ls, 1.0, sigma)
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    tm = eng.timings()
    rows = np.sort(np.random.default_rng(3).choice(N, 5, replace=False))
    sampled_rows_check(eng, spec, theta, X, rows)
    Xs = O.synthetic_grid(d, res=20)
    mu, var = eng.predict(Xs, with_noise=True)
    mu0, var0 = eng.predict(Xs, with_noise=False)
    assert np.array_equal(mu, mu0) and np.allclose(var - var0, sigma**2, rtol=0, atol=1e-14)
    assert np.all(np.isfinite(mu)) and np.all(var0 > 0) and np.all(var0 <= 1.0 + 1e-9)
    # K-build bandwidth sanity: 10 GB written; must be far above anything a re-read pattern gives
    assert tm["kbuild_bytes"] / (tm["kbuild_ms"] * 1e-3) > 1.0e12
    nl = eng.nlml()
    assert np.isfinite(nl)
    eng.close()


def test_c3_full_size_sampled_parity_against_the_host(gpu):
    """C3 at its FULL size (N = 50k, d = 8, Matern-5/2 ARD) against the oracle's arithmetic on the host:
    the 50k x 50k covariance built block-wise with PyMC's distance expansion, one LAPACK dpotrf (20 GB), then mean / variance
    at 32 points sampled from the 10^4-point grid and the NLML -- posterior mean <= 1e-8 relative (the north star's tolerance),
    variance <= 1e-9 absolute, NLML <= 1e-10 relative.  The host side is stored (tests/golden/c3_host_goldens.npz, written by
    tests/golden/make_c3_host_goldens.py with tests/host_reference.py): it takes minutes and ~24 GB of host memory."""
    N, d = 50_000, 8
    gold = np.load(GOLD / "c3_host_goldens.npz")
    X, y, ls = O.synthetic_table(N, d)
    spec = O.make_spec(d, range(d), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    assert np.array_equal(theta, gold["theta"])
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    Xs = O.synthetic_grid(d, res=100)
    mu, var = eng.predict(Xs, with_noise=True)
    nl = eng.nlml()
    eng.close()
    sub = np.sort(np.random.default_rng(11).choice(len(Xs), 32, replace=False))
    assert np.array_equal(sub, gold["sub"])
    mu_r, var_r, nl_r = gold["mu"], gold["var"], float(gold["nlml"])
    print(f"host (stored): mean rel err {rel(mu[sub], mu_r):.2e}, var abs err {np.max(np.abs(var[sub] - var_r)):.2e}, "
          f"nlml rel err {abs(nl - nl_r) / abs(nl_r):.2e}")
    assert rel(mu[sub], mu_r) < 1e-8 and np.max(np.abs(var[sub] - var_r)) < 1e-9
    assert abs(nl - nl_r) <= 1e-10 * abs(nl_r)


def test_c5_size_on_one_gpu(gpu):
    """BASELINE.json configs[4] at its full size -- N = 100,000, d = 8, RBF-ARD -- on ONE MI355X (the
    strong-scaling base of the 8-GPU run; 80 GB factor + 80 GB gradient workspace of 288 GB): the path
    `PymcGP.fit` -> `find_MAP` -> `predict` reaches (gumbi/regression/pymc/GP.py:255-387, 799-813, 837-849) as
    factorise -> one objective + gradient evaluation -> re-factorise -> predict, checked through
    size-independent properties: L L^T = Sigma on sampled rows against the oracle's covariance, the
    `with_noise` shift, variances inside (0, prior], a finite NLML / gradient, and the posterior mean
    recomputed from its definition k(x*, X) alpha with the alpha = Sigma^-1 y the gradient call leaves."""
    import time

    N, d = 100_000, 8
    X, y, ls = O.synthetic_table(N, d)
    spec = O.make_spec(d, range(d), kind="ExpQuad")
    sigma = 0.2
    theta = O.pack_theta(spec, ls, 1.0, sigma)
    eng = make_engine(spec, theta, X, y)
    t0 = time.perf_counter()
    eng.factorize()
    t_fact = time.perf_counter() - t0
    rows = np.sort(np.random.default_rng(11).choice(N, 6, replace=False))
    sampled_rows_check(eng, spec, theta, X, rows)
    v = eng.copy_v()
    diag = np.array([eng.copy_factor(int(i), 1, int(i), 1)[0, 0] for i in np.random.default_rng(1).choice(N, 64)])
    assert np.all(diag > 0) and np.all(np.isfinite(v))
    nl = eng.nlml()
    t0 = time.perf_counter()
    val, g = eng.nlml(grad=True)
    t_grad = time.perf_counter() - t0
    assert val == nl and np.all(np.isfinite(g)) and g.shape == (d + 2,)
    alpha = eng.copy_alpha()
    assert np.isfinite(alpha).all()
    assert eng.factor_is_current()  # the gradient leaves the factorisation intact: no second factorize
    Xs = O.synthetic_grid(d, res=100)
    t0 = time.perf_counter()
    mu, var = eng.predict(Xs, with_noise=True)
    t_pred = time.perf_counter() - t0
    mu0, var0 = eng.predict(Xs, with_noise=False)
    assert np.array_equal(mu, mu0) and np.allclose(var - var0, sigma**2, rtol=0, atol=1e-14)
    assert np.all(np.isfinite(mu)) and np.all(var0 > 0) and np.all(var0 <= 1.0 + 1e-9)
    # mean = k(x*, X) alpha, straight from the definition, on a few grid points (alpha from the gradient call)
    sub = np.random.default_rng(2).choice(len(Xs), 16, replace=False)
    Ks = O.cov_full(spec, theta, Xs[sub], X, dist_mode="direct")
    assert rel(mu[sub], Ks @ alpha) < 1e-8
    print(f"C5 on one GPU: factorise {t_fact:.2f} s ({N**3 / 3 / t_fact / 1e12:.1f} TF/s), objective+gradient "
          f"{t_grad:.2f} s, predict(1e4) {t_pred:.2f} s")
    assert t_fact < 20 and t_grad < 40 and t_pred < 10
    eng.close()


def test_c4_midsize_parity_and_frontend_correlation(gpu):
    X, y, spec, theta = icm_problem(1500, 4)
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    rng = np.random.default_rng(0)
    Xs1 = rng.standard_normal((200, 4))
    Xs = np.vstack([np.column_stack([Xs1, np.full(200, p)]) for p in range(2)])
    mu, var = eng.predict(Xs)
    mu_r, var_r = O.predict(spec, theta, X, y, Xs)
    assert rel(mu, mu_r) < 1e-8 and np.max(np.abs(var - var_r)) < 1e-9
    val, g = eng.nlml(grad=True)
    val_r, g_r = O.nlml_and_grad(spec, theta, X, y)
    assert np.isclose(val, val_r, rtol=1e-10)
    assert np.max(np.abs(g - g_r)) < 1e-8 * max(1.0, np.max(np.abs(g_r)))


def test_c4_full_size_properties(gpu):
    """2-output ICM, N = 20k, d = 4: the stacked 40k x 5 system (K = B (x) K_x + D (x) I)."""
    n, d = 20_000, 4
    X, y, spec, theta = icm_problem(n, d)
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    rows = np.array([5, 7_777, 19_999, 20_000, 31_234, 39_999])
    sampled_rows_check(eng, spec, theta, X, rows)
    Xs1 = O.synthetic_grid(d, res=15)
    Xs = np.vstack([np.column_stack([Xs1, np.full(len(Xs1), p)]) for p in range(2)])
    mu, var = eng.predict(Xs, with_noise=True)
    _, var0 = eng.predict(Xs, with_noise=False)
    nz = O.noise_diag(spec, theta, Xs)
    assert np.allclose(var - var0, nz, rtol=0, atol=1e-13)
    assert nz[0] != nz[-1]  # heteroskedastic across outputs
    assert np.all(var0 > 0)
    eng.close()


@pytest.mark.parametrize("n,d,lin", [(700, 4, False), (900, 3, True)])
def test_kronecker_engine_matches_the_oracle_directly(gpu, n, d, lin):
    """IcmEngine (P systems of size N, gumbi_amd/regression/icm.py) straight against the ORACLE's stacked
    PN x PN evaluation -- not against the stacked HIP engine: NLML, every gradient entry (kernel parameters,
    output table W / kappa, noise table), posterior mean and variance with and without noise."""
    from gumbi_amd.engine import KernelSpec
    from gumbi_amd.regression.icm import IcmEngine

    X, y, spec, theta = icm_problem(n, d, seed=17)
    idx_lin = [1] if lin else []
    if lin:
        spec = O.make_spec(d + 1, range(d), kind="ExpQuad", idx_lin=idx_lin, out_col=d, n_out=2, hetero_noise=True)
        p = O.unpack_theta(icm_problem(n, d, seed=17)[2], theta)
        theta = O.pack_theta(spec, p["ls"], p["eta"], p["sigma"], c=[0.3], tau=0.7, W_out=p["W_out"], kappa_out=p["kappa_out"],
                             W_noise=p["W_noise"], kappa_noise=p["kappa_noise"])
    ks = KernelSpec(D=d + 1, idx_cont=list(range(d)), kind="ExpQuad", idx_lin=idx_lin, out_col=d, n_out=2, hetero_noise=True)
    kron = IcmEngine(0)
    kron.set_data(X, y)
    kron.set_kernel(ks)
    rng = np.random.default_rng(4)
    for trial in range(2):
        th = theta.copy() if trial == 0 else theta * np.exp(rng.normal(0, 0.15, theta.size))
        kron.set_theta(th)
        kron.factorize()
        val, g = kron.nlml(grad=True)
        val_r, g_r = O.nlml_and_grad(spec, th, X, y, dist_mode="direct")
        assert np.isclose(val, val_r, rtol=1e-10)
        assert np.max(np.abs(g - g_r)) < 1e-7 * max(1.0, np.max(np.abs(g_r)))
        Xs1 = rng.standard_normal((60, d))
        Xs = np.vstack([np.column_stack([Xs1, np.full(len(Xs1), p)]) for p in range(2)])
        kron.factorize()
        for with_noise in (True, False):
            mu, var = kron.predict(Xs, with_noise=with_noise)
            mu_r, var_r = O.predict(spec, th, X, y, Xs, with_noise=with_noise, dist_mode="direct")
            assert rel(mu, mu_r) < 1e-8 and np.max(np.abs(var - var_r)) < 1e-9
    kron.close()


def test_kronecker_path_keeps_every_system_resident(gpu, monkeypatch):
    """One inner engine per system (siblings sharing one set of HIP streams): after a gradient evaluation every
    factor is still resident, so predictions and repeated evaluations at the same theta factorise nothing; the
    single-shared-engine mode (systems that do not fit together) gives the same numbers."""
    from gumbi_amd.engine import KernelSpec
    from gumbi_amd.regression.icm import IcmEngine

    n, d = 700, 3
    X, y, spec, theta = icm_problem(n, d, seed=5)
    ks = KernelSpec(D=d + 1, idx_cont=list(range(d)), kind="ExpQuad", out_col=d, n_out=2, hetero_noise=True)
    Xs1 = np.random.default_rng(1).standard_normal((150, d))
    Xs = np.vstack([np.column_stack([Xs1, np.full(len(Xs1), p)]) for p in range(2)])
    kron = IcmEngine(0)
    kron.set_data(X, y)
    kron.set_kernel(ks)
    kron.set_theta(theta)
    kron.factorize()
    val, g = kron.nlml(grad=True)
    assert len(kron._engs) == 2 and kron.factor_is_current()
    calls = []
    for e in kron._engs:
        monkeypatch.setattr(e, "factorize", lambda orig=e.factorize: (calls.append(1), orig())[1])
    mu, var = kron.predict(Xs)
    mu_b, var_b = kron.predict(Xs[::-1])
    val2, g2 = kron.nlml(grad=True)
    assert not calls
    assert val2 == val and np.max(np.abs(g2 - g)) < 1e-10 * max(1.0, np.max(np.abs(g)))
    assert np.allclose(mu_b[::-1], mu, rtol=0, atol=1e-12) and np.allclose(var_b[::-1], var, rtol=0, atol=1e-12)
    kron.set_theta(theta * 1.01)
    assert not kron.factor_is_current()
    kron.nlml()
    assert len(calls) == 2 and kron.factor_is_current()
    kron.close()
    monkeypatch.setattr(IcmEngine, "RESIDENT_BYTES", 0.0)
    shared = IcmEngine(0)
    shared.set_data(X, y)
    shared.set_kernel(ks)
    shared.set_theta(theta)
    shared.factorize()
    val_s, g_s = shared.nlml(grad=True)
    mu_s, var_s = shared.predict(Xs)
    assert len(shared._engs) == 1 and not shared.factor_is_current()
    assert val_s == val and np.max(np.abs(g_s - g)) < 1e-10 * max(1.0, np.max(np.abs(g)))
    assert np.allclose(mu_s, mu, rtol=0, atol=1e-12) and np.allclose(var_s, var, rtol=0, atol=1e-12)
    shared.close()


def test_c4_full_size_kronecker_equals_stacked(gpu):
    """C4 at full size both ways: the stacked 40k x 40k system and the Kronecker form (two 20k x 20k
    systems, gumbi_amd/regression/icm.py) give the same NLML, gradient and predictions; the
    Kronecker evaluation is the cheaper one (P^2 = 4x fewer flops)."""
    import time

    from gumbi_amd.engine import KernelSpec
    from gumbi_amd.regression.icm import IcmEngine

    n, d = 20_000, 4
    X, y, spec, theta = icm_problem(n, d)
    ks = KernelSpec(D=d + 1, idx_cont=list(range(d)), kind="ExpQuad", out_col=d, n_out=2, hetero_noise=True)
    stacked = make_engine(spec, theta, X, y)
    kron = IcmEngine(0)
    kron.set_data(X, y)
    kron.set_kernel(ks)
    kron.set_theta(theta)
    out = {}
    for name, eng in (("stacked", stacked), ("kron", kron)):
        eng.factorize()
        eng.nlml(grad=True)  # warm-up (workspace allocation)
        eng.factorize()
        t0 = time.perf_counter()
        eng.factorize()
        val, g = eng.nlml(grad=True)
        out[name] = (val, g, time.perf_counter() - t0)
    (vs, gs, ts), (vk, gk, tk) = out["stacked"], out["kron"]
    assert np.isclose(vk, vs, rtol=1e-11)
    assert np.max(np.abs(gk - gs)) < 1e-7 * max(1.0, np.max(np.abs(gs)))
    Xs1 = O.synthetic_grid(d, res=12)
    Xs = np.vstack([np.column_stack([Xs1, np.full(len(Xs1), p)]) for p in range(2)])
    stacked.factorize()
    kron.factorize()
    ms, vs2 = stacked.predict(Xs)
    mk, vk2 = kron.predict(Xs)
    assert rel(mk, ms) < 1e-8 and np.max(np.abs(vk2 - vs2)) < 1e-9
    print(f"C4 MAP evaluation: stacked {ts:.3f} s, Kronecker {tk:.3f} s")
    assert tk < 0.6 * ts
    stacked.close()
    kron.close()


def test_cross_validate_runs_on_gpu(gpu):
    import gumbi_amd as gmb

    stdzr = gmb.Standardizer(
        **{"d": {"μ": -0.307, "σ2": 0.158**2}, "X": {"μ": -0.282, "σ2": 1.0}, "Y": {"μ": 4.48, "σ2": 0.75**2}},
        log_vars=["d", "Y"], logit_vars=["X"])
    es = pd.read_pickle(GOLD / "test_dataset.pkl")
    ds = gmb.DataSet.from_tidy(es, names_column="Parameter", stdzr=stdzr)
    gp = gmb.GP(ds, outputs="d")
    gp.specify_model(continuous_dims=["X", "Y"])
    gp.build_model()
    res = gp.cross_validate(n_train=50, seed=3, maxeval=40)
    assert set(res) == {"train", "test"}
    assert res["train"]["errors"].shape == (50,) and res["test"]["errors"].shape == (16,)
    assert np.all(np.isfinite(res["train"]["NLPDs"])) and np.all(np.isfinite(res["test"]["NLPDs"]))
    # natural-space errors of 'd' (values ~0.5-0.9) stay small on both splits
    assert np.mean(np.abs(res["train"]["errors"])) < 0.1 and np.mean(np.abs(res["test"]["errors"])) < 0.1


# ------------------------------------------------------------------------------------------- fits that fit
def _bench_module():
    import importlib.util
    import sys

    root = Path(__file__).resolve().parent.parent
    spec = importlib.util.spec_from_file_location("bench_fitq", root / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    sys.modules["bench_fitq"] = mod
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name,N", [("c2", 10_000), ("c3", 12_288)])
def test_headline_fit_reaches_the_optimum(gpu, name, N):
    """The fit bench.py times: the declared model of the bench -- ``ls_bounds`` lower limit
    of half a standard deviation through ``make_deltas_parray`` (reference pymc/GP.py:630-650,
    array_utils.py:8-33) -- fitted by ``find_MAP`` to convergence, at C2's full size and at a quarter of C3's:
    scipy reports convergence in a few dozen evaluations, the grid mean follows the generator's noise-free
    function (correlation > 0.95; predicting zero would give the RMSE of f itself) and sigma-hat is the
    generator's noise level to 10 %."""
    bench = _bench_module()
    cfg = dict(bench.CONFIGS[name], N=N)
    gp = bench.build_gp(cfg, device=0)
    assert np.all(gp._initial_theta()[: cfg["d"]] > 1.0)  # the start the bounds imply: O(1) length scales
    gp.find_MAP()
    mu, var = gp.predict(bench.synthetic_grid(cfg["d"], cfg["res"]))
    q = bench.fit_quality(gp, mu, cfg)
    gp.engine.close()
    assert q["converged"] and 10 <= q["n_eval"] <= 80 and q["rejected_evals"] == 0, q
    assert q["corr"] > 0.95 and q["rmse"] < 0.35 * q["rmse_of_predicting_zero"], q
    assert q["sigma_rel_err"] < 0.10, q
    assert np.all(var > 0)


def test_default_start_stalls_exactly_as_the_oracle_engine_says(gpu, monkeypatch):
    """The degenerate case stays pinned too: with the reference's DEFAULT lengthscale prior (limits from the
    smallest pairwise gap, gp_utils.py:34-46) and PyMC's initial point (l = 0.023 on z-scored inputs, where
    K = I) L-BFGS-B on a d = 8 Matern-5/2 table walks the white-noise plateau.  The HIP engine and the numpy
    oracle behind the SAME host code must trace the same objective values and end in the same place --
    NLML = N/2 (log 2 pi + 1), predictions ~ 0 -- so the stall is the model's, not the engine's."""
    import gumbi_amd as gmb
    from gumbi_amd.regression import hip_gp
    from oracle_engine import OracleEngine

    bench = _bench_module()
    cfg = dict(bench.CONFIGS["c3"], N=700)
    Xs = bench.synthetic_grid(cfg["d"], 20)

    def run():
        gp = bench.build_gp(cfg, device=0, ls_lower=None)
        start = gp._initial_theta()
        gp.find_MAP()
        mu, _ = gp.predict(Xs)
        out = (start, np.array(gp.nlml_trace), gp._theta_fitted.copy(), mu, gp.n_eval)
        gp.engine.close()
        return out

    s_hip, tr_hip, th_hip, mu_hip, n_hip = run()
    monkeypatch.setattr(hip_gp, "Engine", OracleEngine)
    s_cpu, tr_cpu, th_cpu, mu_cpu, n_cpu = run()
    assert np.allclose(s_hip, s_cpu, rtol=1e-12) and np.all(s_hip[:8] < 0.05)        # l = 0.023: the prior's mode
    k = min(len(tr_hip), len(tr_cpu), 5)
    assert k >= 5 and np.allclose(tr_hip[:k], tr_cpu[:k], rtol=1e-7), (tr_hip[:k], tr_cpu[:k])
    plateau = 0.5 * cfg["N"] * (np.log(2 * np.pi) + 1.0)
    assert abs(tr_hip[-1] - plateau) < 2.0 and abs(tr_cpu[-1] - plateau) < 2.0             # y ~ N(0, I)
    assert np.max(np.abs(mu_hip)) < 1e-6 and np.max(np.abs(mu_cpu)) < 1e-6                 # nothing learnt
    assert np.all(th_hip[:8] < 0.05) and np.all(th_cpu[:8] < 0.05)
    assert isinstance(gmb.GP, type)
