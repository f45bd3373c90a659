"""The gradient of the posterior variance on the CPU (``-m "not gpu"``: runs anywhere).  ``var_grad_reference.mean_var_grad`` --
the closed form the HIP kernels implement, in numpy -- is pinned three ways:

1. its variance part against Richardson-extrapolated central differences (h = 1e-3 and h / 2) of the oracle's predictive
   variance, on the cases of tests/test_predict_grad_cpu.py.  Bars as there and for the same reason: 1e-9 of max|G| for ExpQuad /
   Matern52 / Matern32 and the composite / additive / periodic / shared-lengthscale models, 1e-7 for Matern12 / Exponential
   (whose third derivative is large near a training point: the differences, not the formula, set that error);
2. its mean part equals ``grad_reference.mean_grad`` exactly;
3. on every case the GPU test compares against (tests/test_gpu_var_grad.py: ``CASES``), the float64 reference lies within
   ``1e-10 max|G|`` of the same computation in extended precision (tests/precise_reference.py): the reference alone is 100 x
   inside the GPU bar of 1e-8.
"""
import numpy as np
import pytest

import grad_reference as GR
import var_grad_reference as VR
from oracle import gp_oracle as O
from test_gpu_parity import GOLD, golden_spec
from test_gpu_predict_grad import points, table
from test_gpu_var_grad import CASES, case, reference


# ---- 1. central differences ------------------------------------------------------------------------------------------------------
def fd_error(spec, theta, X, y, Xs, periodic=0, periods=None):
    G = VR.mean_var_grad(spec, theta, X, y, Xs, periodic=periodic, periods=periods)[3]
    fd = VR.fd_var_grad(VR.posterior_var(spec, theta, X, y, periodic=periodic, periods=periods), Xs, spec["idx_cont"])
    others = [c for c in range(Xs.shape[1]) if c not in spec["idx_cont"]]
    assert not np.any(G[:, others])  # categorical columns and the output index: exactly 0
    return float(np.max(np.abs(G - fd))) / float(np.max(np.abs(G)))


@pytest.mark.parametrize("kind", list(O.KINDS))
def test_reference_matches_finite_differences_for_every_kind(kind):
    spec, theta, X, y = table(300, 3, kind)
    err = fd_error(spec, theta, X, y, points(X, 50, [0, 1, 2]))
    print(f"{kind}: {err:.2e}")
    assert err <= (1e-7 if kind in ("Matern12", "Exponential") else 1e-9)


def test_reference_matches_finite_differences_on_the_composite_model():
    name = "composite_N140"
    spec, theta, X, y = golden_spec(name), GOLD[f"{name}/theta"], GOLD[f"{name}/X"], GOLD[f"{name}/y"]
    err = fd_error(spec, theta, X, y, points(X, 50, spec["idx_cont"]))
    print(f"composite: {err:.2e}")
    assert err <= 1e-9


def test_reference_matches_finite_differences_on_an_additive_model():
    from test_oracle import additive_problem

    spec, theta, X, y = additive_problem(n=150)
    err = fd_error(spec, theta, X, y, points(X, 50, spec["idx_cont"]))
    print(f"additive: {err:.2e}")
    assert err <= 1e-9


@pytest.mark.parametrize("kind,mode", [("Matern52", 1), ("ExpQuad", 2)])
def test_reference_matches_finite_differences_on_periodic_models(kind, mode):
    from test_gpu_periodic import case as periodic_case

    spec, theta, X, y, periods = periodic_case(kind, mode, 300, 2)
    err = fd_error(spec, theta, X, y, points(X, 50, [0, 1]), periodic=mode, periods=periods)
    print(f"{kind} periodic mode {mode}: {err:.2e}")
    assert err <= 1e-9


def test_reference_matches_finite_differences_with_a_shared_lengthscale():
    spec, theta, X, y = table(300, 3, "Matern52", ard=False)
    err = fd_error(spec, theta, X, y, points(X, 50, [0, 1, 2]))
    print(f"shared lengthscale: {err:.2e}")
    assert err <= 1e-9


# ---- 2. the mean part; values ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Matern52-N300-d3-M77", "composite_N140", "additive-N300", "Periodic"])
def test_mean_part_is_the_mean_gradient_reference_and_values_are_the_oracles(name):
    spec, theta, X, y, Xs, mode, periods = case(name)
    mean, var, dmean, dvar = reference(name)
    assert np.array_equal(dmean, GR.mean_grad(spec, theta, X, y, Xs, periodic=mode, periods=periods))
    if not mode:
        mu_o, var_o = O.predict(spec, theta, X, y, Xs, with_noise=True, dist_mode="direct")
        assert np.allclose(mean, mu_o, rtol=1e-12, atol=1e-14) and np.allclose(var, var_o, rtol=1e-12, atol=1e-14)
    noiseless = VR.mean_var_grad(spec, theta, X, y, Xs, periodic=mode, periods=periods, with_noise=False)
    assert np.array_equal(noiseless[3], dvar) and np.all(noiseless[1] < var)


# ---- 3. extended precision -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_reference_is_within_1e10_of_extended_precision(name):
    spec, theta, X, y, Xs, mode, periods = case(name)
    _, _, dmean, dvar = reference(name)
    if len(Xs) > 1000:  # the M-tiling case: every row of the reference is computed on its own, so a slice of the first tile and
        rows = np.r_[0:64, len(Xs) - 77:len(Xs)]  # the whole ragged second tile are compared (extended precision is slow)
        Xs, dmean, dvar = Xs[rows], dmean[rows], dvar[rows]
    pm, pv = VR.mean_var_grad_precise(spec, theta, X, y, Xs, periodic=mode, periods=periods)
    for got, ref, what in ((dmean, pm, "dmean"), (dvar, pv, "dvar")):
        scale = float(np.max(np.abs(ref)))
        err = float(np.max(np.abs(got - ref)))
        print(f"{name} {what}: float64 vs extended precision {err / scale:.2e} of max|G| = {scale:.3e}")
        assert err <= 1e-10 * scale
