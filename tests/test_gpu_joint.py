"""The joint posterior on the MI355X -- ``gmb_predict_joint`` / ``gmb_draw_joint`` through ``gumbi_amd.engine.Engine`` --
against the oracle (``dist_mode="direct"``; tests/test_joint_cpu.py: ``JointOracleEngine``).

Bars and where they come from:

1. covariance: 1e-9 absolute, mean 1e-8 relative -- the project's bars for variance and mean (tests/test_gpu_parity.py:3-5);
   ``diag(cov)`` against ``gmb_predict``'s variance 1e-11, the bar between the engine's own two forms; solve form against
   product form of V 1e-10 relative.
2. well-conditioned draws (``with_noise=True``, ``jitter=0``; cond(C) 2 .. 40 on the synthetic cases): 1e-8 relative to
   max |Y_oracle|, the mean's bar -- a draw is an affine image of the same solves.  A symmetric 1e-13 perturbation of C moves
   the float64 draws by at most 9e-12 there, so the reference sits orders inside the bar and the bar catches any error in C
   above ~1e-10.
3. jitter-limited draws (``with_noise=False``, ``jitter=1e-6``; cond(C) 1e5 .. 3e6, the same perturbation moves draws by up
   to 3e-8): NO elementwise comparison -- it would measure conditioning.  ``draw_joint`` with Z = I returns the factor
   itself; it must be lower triangular with a positive diagonal and reproduce the matrix it factors within 50 x the backward
   error of numpy's Cholesky on the same matrix (floored at 4 eps max|C|): tests/test_gpu_conditioning.py records this engine's
   factor at 12 .. 39 x LAPACK's backward error on jitter-limited matrices, 50 is that worst x 1.25.  The measured ratio is
   printed per case (``BACKWARD joint/<case> <ratio>``).  The draw kernel is then checked against that factor as a plain
   product, 1e-12 relative.
4. state: nothing of the training factorisation is touched by a draw (bit-identical predict / nlml / gradient afterwards).
5. front end, 6. memory guard.
"""
import functools
from pathlib import Path

import numpy as np
import pytest

from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent
GOLD = np.load(HERE / "golden" / "gp_goldens.npz")
EPS = np.finfo(np.float64).eps


def kspec(spec):
    from gumbi_amd.engine import KernelSpec

    return KernelSpec(D=spec["D"], idx_cont=spec["idx_cont"], kind=spec["kind"], ard=spec["ard"],
                      idx_lin=spec["idx_lin"], coreg=spec["coreg"], out_col=spec["out_col"], n_out=spec["n_out"],
                      hetero_noise=spec["hetero_noise"], jitter=spec["jitter"], additive=spec.get("additive", False))


def make_engine(spec, theta, X, y):
    from gumbi_amd.engine import Engine

    eng = Engine(0)
    eng.set_data(X, y)
    eng.set_kernel(kspec(spec))
    eng.set_theta(theta)
    return eng


def synthetic(kind, d, N, Xs, seed=2021):
    X, y, ls = O.synthetic_table(N, d, seed=seed)
    spec = O.make_spec(d, range(d), kind=kind)
    return spec, O.pack_theta(spec, ls, 1.0, 0.3), X, y, Xs


@functools.lru_cache(maxsize=None)
def problem(case):
    """(spec, theta, X, y, Xs, fit): ``fit`` = the factor comes from evaluate(theta, grad=True), as after a MAP fit."""
    if case == "matern52_d2":
        return (*synthetic("Matern52", 2, 600, O.synthetic_grid(2, res=20)), False)
    if case == "expquad_d1":
        return (*synthetic("ExpQuad", 1, 300, O.synthetic_grid(1, res=100)), False)
    if case == "expquad_d2":
        return (*synthetic("ExpQuad", 2, 600, O.synthetic_grid(2, res=24)), False)
    if case == "composite":
        spec = O.make_spec(4, [0, 1], idx_lin=[1], coreg=[(2, 3)], out_col=3, n_out=2, hetero_noise=True)
        X, y, Xs, theta = (GOLD[f"composite_N140/{k}"] for k in ("X", "y", "Xs", "theta"))
        return spec, theta, X, y, Xs, False
    if case == "additive":
        from test_oracle import additive_problem

        spec, theta, X, y = additive_problem(n=300, two_outputs=False, lin=True, hetero=False)
        Xs = X[::3].copy()
        Xs[:, 0] += 0.17
        return spec, theta, X, y, Xs, False
    if case == "ragged":
        Xs = np.random.default_rng(333).standard_normal((333, 3))
        return (*synthetic("Matern52", 3, 1000, Xs, seed=1000), False)
    if case == "fit_4224":
        return (*synthetic("Matern52", 2, 4224, O.synthetic_grid(2, res=20), seed=4224), True)
    raise KeyError(case)


CASES = ["matern52_d2", "expquad_d1", "expquad_d2", "composite", "additive", "ragged", "fit_4224"]


def ready_engine(case, form=None):
    spec, theta, X, y, Xs, fit = problem(case)
    eng = make_engine(spec, theta, X, y)
    if form is not None:
        eng.set_predict_form(form)
    if fit:
        eng.evaluate(theta, grad=True)
    else:
        eng.factorize()
    return eng, Xs


@functools.lru_cache(maxsize=None)
def oracle_joint(case, with_noise, jitter):
    from test_joint_cpu import JointOracleEngine

    spec, theta, X, y, Xs, _ = problem(case)
    ref = JointOracleEngine()
    ref.set_data(X, y)
    ref.spec = spec
    ref.set_theta(theta)
    return ref.predict_joint(Xs, with_noise=with_noise, jitter=jitter)


# ---- 1. covariance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("case", CASES)
def test_joint_covariance_matches_oracle(gpu, case, with_noise):
    eng, Xs = ready_engine(case)
    fit = problem(case)[5]
    jitter = 0.0 if with_noise else 1e-6
    mean, cov = eng.predict_joint(Xs, with_noise=with_noise, jitter=jitter)
    assert eng.timings()["predict_gemm_form"] == (1 if fit else 0)
    mean_r, cov_r = oracle_joint(case, with_noise, jitter)
    err_c = float(np.max(np.abs(cov - cov_r)))
    err_m = float(np.max(np.abs(mean - mean_r)) / np.max(np.abs(mean_r)))
    print(f"JOINT cov/{case}/noise={int(with_noise)} max|dC| {err_c:.3e} mean rel {err_m:.3e}")
    assert np.array_equal(cov, cov.T)
    assert err_c <= 1e-9 and err_m <= 1e-8
    # the diagonal is gmb_predict's variance (+ jitter) on the same engine, and the mean its mean
    mu, var = eng.predict(Xs, with_noise=with_noise)
    assert np.max(np.abs(np.diag(cov) - jitter - var)) <= 1e-11
    assert np.max(np.abs(mean - mu)) <= 1e-10 * np.max(np.abs(mu))
    eng.close()


def test_solve_form_and_product_form_of_v_agree(gpu):
    eng_p, Xs = ready_engine("fit_4224")
    eng_s, _ = ready_engine("fit_4224", form=0)
    mean_p, cov_p = eng_p.predict_joint(Xs, with_noise=True)
    assert eng_p.timings()["predict_gemm_form"] == 1
    mean_s, cov_s = eng_s.predict_joint(Xs, with_noise=True)
    assert eng_s.timings()["predict_gemm_form"] == 0
    mean_r, cov_r = oracle_joint("fit_4224", True, 0.0)
    assert np.max(np.abs(cov_s - cov_r)) <= 1e-9 and np.max(np.abs(mean_s - mean_r)) <= 1e-8 * np.max(np.abs(mean_r))
    assert np.max(np.abs(cov_p - cov_s)) <= 1e-10 * np.max(np.abs(cov_s))
    Z = np.random.default_rng(1).standard_normal((8, Xs.shape[0]))
    Yp, Ys = eng_p.draw_joint(Xs, Z, with_noise=True, jitter=0.0), eng_s.draw_joint(Xs, Z, with_noise=True, jitter=0.0)
    assert np.max(np.abs(Yp - Ys)) <= 1e-8 * np.max(np.abs(Ys))
    eng_p.close()
    eng_s.close()


# ---- 2. draws, well-conditioned --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_draws_match_oracle_when_well_conditioned(gpu, case):
    eng, Xs = ready_engine(case)
    M = Xs.shape[0]
    Z = np.random.default_rng(1).standard_normal((8, M))
    Y, mean = eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0, return_mean=True)
    mean_r, cov_r = oracle_joint(case, True, 0.0)
    Y_r = mean_r[None, :] + Z @ O.cholesky_lower(cov_r).T
    err = float(np.max(np.abs(Y - Y_r)) / np.max(np.abs(Y_r)))
    print(f"JOINT draw/{case} rel err {err:.3e} cond(C) {np.linalg.cond(cov_r):.2e}")
    assert Y.shape == (8, M) and err <= 1e-8
    assert np.max(np.abs(mean - mean_r)) <= 1e-8 * np.max(np.abs(mean_r))
    # zero normals: the mean itself; one draw, odd counts of draws (the kernel's 16-draw sub-tiles)
    assert np.array_equal(eng.draw_joint(Xs, np.zeros((1, M)), with_noise=True, jitter=0.0)[0], mean)
    for S in (1, 17, 33):
        Zs = np.random.default_rng(S).standard_normal((S, M))
        Ys = eng.draw_joint(Xs, Zs, with_noise=True, jitter=0.0)
        assert np.max(np.abs(Ys - (mean_r[None, :] + Zs @ O.cholesky_lower(cov_r).T))) <= 1e-8 * np.max(np.abs(Y_r))
    eng.close()


# ---- 3. draws, jitter-limited ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_factor_behind_jitter_limited_draws(gpu, case):
    eng, Xs = ready_engine(case)
    M = Xs.shape[0]
    jitter = 1e-6
    _, cov = eng.predict_joint(Xs, with_noise=False, jitter=0.0)
    A = cov + jitter * np.eye(M)
    Y, mean = eng.draw_joint(Xs, np.eye(M), with_noise=False, jitter=jitter, return_mean=True)
    L = (Y - mean[None, :]).T  # row s of Y is mean + column s of the factor
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L))
    assert np.all(np.diag(L) > 0.0)
    L_host = np.linalg.cholesky(A)
    b_host = float(np.max(np.abs(L_host @ L_host.T - A)))
    b_gpu = float(np.max(np.abs(L @ L.T - A)))
    floor = 4.0 * EPS * float(np.max(np.abs(A)))
    print(f"BACKWARD joint/{case} {b_gpu / max(b_host, floor):.2f}  (gpu {b_gpu:.3e} host {b_host:.3e} floor {floor:.3e} "
          f"cond {np.linalg.cond(A):.2e})")
    assert b_gpu <= 50.0 * max(b_host, floor)
    # the draw kernel against the engine's own factor: a plain product
    Z = np.random.default_rng(2).standard_normal((8, M))
    Y2, mean2 = eng.draw_joint(Xs, Z, with_noise=False, jitter=jitter, return_mean=True)
    want = Z @ L.T
    assert np.array_equal(mean2, mean)
    assert np.max(np.abs((Y2 - mean2[None, :]) - want)) <= 1e-12 * max(np.max(np.abs(want)), np.max(np.abs(Y2)))
    eng.close()


def test_duplicate_test_points_with_the_default_jitter(gpu):
    """Coinciding test points make the noise-free C singular; with the default jitter it is positive definite by construction."""
    eng, Xs = ready_engine("expquad_d2")
    Xd = np.vstack([Xs[:40], Xs[:40]])
    Z = np.random.default_rng(3).standard_normal((4, 80))
    Y = eng.draw_joint(Xd, Z)  # with_noise=False, jitter=1e-6
    assert np.all(np.isfinite(Y))
    assert np.max(np.abs(Y[:, :40] - Y[:, 40:])) < 0.1  # the copies move together (apart by ~sqrt(jitter) z)
    eng.close()


# ---- 4. state --------------------------------------------------------------------------------------------------------------
def _predict_nlml_sequence(case, with_draws):
    """predict, nlml | (draws and a joint covariance) | predict, nlml, nlml with its gradient -- on a fresh engine."""
    _, _, _, _, Xs, _ = problem(case)
    Z = np.random.default_rng(4).standard_normal((5, Xs.shape[0]))
    eng, _ = ready_engine(case)
    out = [*eng.predict(Xs), eng.timings()["predict_gemm_form"], eng.nlml()]
    if with_draws:
        Y1 = eng.draw_joint(Xs, Z)
        assert eng.factor_is_current()
        Y2 = eng.draw_joint(Xs, Z)
        assert np.array_equal(Y1, Y2)  # a draw is a function of (model, theta, Xs, Z)
        eng.predict_joint(Xs)
        assert eng.factor_is_current()
    out += [*eng.predict(Xs), eng.timings()["predict_gemm_form"], eng.nlml()]
    val, g = eng.nlml(grad=True)
    eng.close()
    return out + [val, g]


@pytest.mark.parametrize("case", ["matern52_d2", "ragged", "additive", "fit_4224"])
def test_draws_leave_the_training_factorisation_alone(gpu, case):
    drew = _predict_nlml_sequence(case, True)
    mu0, var0, form0, nlml0, mu1, var1, form1, nlml1, val, g = drew
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1) and form0 == form1 and nlml0 == nlml1
    plain = _predict_nlml_sequence(case, False)
    for a, b in zip(drew, plain):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_draws_behind_a_separate_gradient_call(gpu):
    """factorize + nlml(grad): the tile path leaves U = L^-T resident and V takes the product form from then on."""
    spec, theta, X, y, Xs, _ = problem("ragged")
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    eng.nlml(grad=True)
    mu0, var0 = eng.predict(Xs)
    assert eng.timings()["predict_gemm_form"] == 1
    mean, cov = eng.predict_joint(Xs, with_noise=True)
    assert eng.timings()["predict_gemm_form"] == 1
    mean_r, cov_r = oracle_joint("ragged", True, 0.0)
    assert np.max(np.abs(cov - cov_r)) <= 1e-9 and np.max(np.abs(mean - mu0)) <= 1e-10 * np.max(np.abs(mu0))
    assert np.max(np.abs(np.diag(cov) - var0)) <= 1e-11
    mu1, var1 = eng.predict(Xs)
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    eng.close()


def test_bad_arguments_and_stale_factors_are_refused(gpu):
    spec, theta, X, y, Xs, _ = problem("expquad_d1")
    eng = make_engine(spec, theta, X, y)
    with pytest.raises(ValueError):
        eng.predict_joint(Xs)  # no factorisation yet
    eng.factorize()
    with pytest.raises(ValueError):
        eng.predict_joint(Xs, jitter=-1.0)
    with pytest.raises(ValueError):
        eng.draw_joint(Xs, np.zeros((2, Xs.shape[0] + 1)))
    with pytest.raises(ValueError):
        eng.predict_joint(np.zeros((4, 3)))
    eng.set_theta(theta * 1.1)
    with pytest.raises(ValueError):
        eng.draw_joint(Xs, np.zeros((1, Xs.shape[0])))
    eng.close()


# ---- 5. front end ----------------------------------------------------------------------------------------------------------
def frontend_gp(**kwargs):
    import gumbi_amd as gmb
    from test_joint_cpu import dataset

    return gmb.GP(dataset(), **kwargs)


def test_grid_samples_through_the_front_end(gpu):
    from test_joint_cpu import JointOracleEngine

    res = 12
    gp = frontend_gp(outputs="d").fit(continuous_dims=["X", "Y"], MAP_kwargs={"maxeval": 60})
    gp.prepare_grid(resolution=res)
    draws = gp.draw_grid_samples(n_draws=4)
    assert draws.shape == (4, res, res) and gp.predictions is draws and gp.predictions_X.shape == (res, res)
    assert not np.array_equal(gp.draw_grid_samples(n_draws=4).z.values(), draws.z.values())  # successive calls differ
    z = np.random.default_rng(6).standard_normal((4, res * res))
    got = gp.draw_grid_samples(n_draws=4, with_noise=True, z=z).z.values().reshape(4, -1)
    X, y = gp.get_shaped_data("mean")
    pa, _, _ = gp._prepare_points_for_prediction(gp.grid_points, output=gp._parse_prediction_output(None))
    ref = JointOracleEngine()
    ref.set_data(X, y)
    ref.set_kernel(gp.model.spec)
    ref.set_theta(gp._theta_fitted)
    want = ref.draw_joint(pa, z, with_noise=True, jitter=0.0)
    assert np.max(np.abs(got - want)) <= 1e-8 * np.max(np.abs(want))
    mean, cov = gp.predict_joint(pa, with_noise=True)
    mean_r, cov_r = ref.predict_joint(pa, with_noise=True)
    assert np.max(np.abs(cov - cov_r)) <= 1e-9 and np.max(np.abs(mean - mean_r)) <= 1e-8 * np.max(np.abs(mean_r))


def test_kronecker_path_raises(gpu):
    from gumbi_amd.regression.icm import IcmEngine

    gp = frontend_gp(outputs=["d", "c"])
    gp.fit(continuous_dims=["X"], MAP_kwargs={"maxeval": 10})
    assert isinstance(gp.engine, IcmEngine)
    pts = gp.parray(X=np.linspace(-1.0, 1.0, 9), stdzd=True)
    with pytest.raises(NotImplementedError, match="Kronecker"):
        gp.draw_point_samples(pts, output="d")


# ---- 6. memory guard -------------------------------------------------------------------------------------------------------
def test_a_request_that_cannot_fit_is_refused_before_anything_runs(gpu):
    import torch

    spec, theta, X, y, Xs, _ = problem("fit_4224")
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    mu0, var0 = eng.predict(Xs)
    total = torch.cuda.get_device_properties(0).total_memory
    Np = -(-X.shape[0] // 128) * 128
    # V alone (8 M Np bytes) exceeds what the device has left beside the engine
    M = (total - eng.resident_bytes()) // (8 * Np) + 1024
    big = np.zeros((M, X.shape[1]))  # (never touched: the call is refused before it copies anything)
    before = eng.resident_bytes()
    with pytest.raises(MemoryError, match=r"needs \d+ bytes") as err:
        eng.draw_joint(big, np.zeros((1, M)))
    assert "gmb_draw_joint" in str(err.value) and f"M = {M}" in str(err.value)
    assert eng.resident_bytes() == before and eng.factor_is_current()
    mu1, var1 = eng.predict(Xs)
    assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    mean, cov = eng.predict_joint(Xs)
    assert np.max(np.abs(np.diag(cov) - var1)) <= 1e-11
    eng.close()


def test_group_averages_that_cannot_fit_are_refused_before_anything_runs(gpu):
    """The guard of ``gmb_predict_groups``, without and with a covariance: G = M singleton groups, M as above, so that V for the
    G rows alone exceeds the device.  One check covers the call's own workspace and the joint posterior's buffers (``cov=True``).

    The covariance case goes through the C ABI with the engine's own status check: the front end would first ask numpy for the
    G x G result, which no host has.  The refused call writes none of its outputs, so one double stands in for it.

    ``gmb_loo`` and ``gmb_leave_out`` cannot be made to exceed the device at a test-sized N -- their row count is bounded by N --
    so their guard's arithmetic is covered on the host only (tools/workspace_budget_check.cpp, tests/test_workspace_budget_cpu.py).
    """
    import ctypes as C

    import torch

    from gumbi_amd.engine import GMB_HOST

    spec, theta, X, y, Xs, _ = problem("fit_4224")
    eng = make_engine(spec, theta, X, y)
    eng.factorize()
    mu0, var0 = eng.predict(Xs)
    total = torch.cuda.get_device_properties(0).total_memory
    Np = -(-X.shape[0] // 128) * 128
    M = (total - eng.resident_bytes()) // (8 * Np) + 1024
    big = np.zeros((M, X.shape[1]))  # (never touched: the call is refused before it copies anything)
    offsets = np.arange(M + 1, dtype=np.int64)
    mean, var, one = np.empty(M), np.empty(M), np.empty(1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)

    def without_cov():
        eng.predict_groups(big, offsets)

    def with_cov():
        rc = eng._lib.gmb_predict_groups(eng._h, ptr(big), M, big.shape[1], ptr(offsets), M, None, ptr(mean), ptr(var), ptr(one), M, GMB_HOST)
        eng._check(rc, "gmb_predict_groups")

    before = eng.resident_bytes()
    for call in (without_cov, with_cov):
        with pytest.raises(MemoryError, match=r"needs \d+ bytes") as err:
            call()
        text = str(err.value)
        print(f"{call.__name__}: {text}")
        assert "gmb_predict_groups" in text and f"M = {M}" in text and f"G = {M}" in text
        assert eng.resident_bytes() == before and eng.factor_is_current()
        mu1, var1 = eng.predict(Xs)
        assert np.array_equal(mu0, mu1) and np.array_equal(var0, var1)
    eng.close()
