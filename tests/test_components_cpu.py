"""The components of an additive model without a GPU: the numpy restatement the GPU tests compare against
(tests/components_reference.py) held to the identities it must satisfy, and the layers above the kernels -- header, binding, front
end -- checked for the new calls.

The identities, on the three-term problem (N = 300, M = 75; cond(Sigma) is printed, a few thousand): summed over the terms the
component means are ``O.predict``'s mean and the T x T covariances its noise-free variance -- two formulations of the same numbers
that share the factor, so they agree to rounding of sums of O(1) terms (a few 1e-13; the bar is 1e-11, two orders above, four
below the GPU tests' 1e-9) -- and every pointwise T x T covariance is positive definite (it is the posterior covariance of T
latent values)."""
import re
from pathlib import Path

import numpy as np
import pytest

import components_reference as CR
from oracle import gp_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_num_terms", "gmb_predict_terms", "gmb_predict_grad_terms", "gmb_predict_joint_terms", "gmb_draw_joint_terms",
             "gmb_predict_decompose"]


@pytest.fixture(scope="module")
def comps():
    return CR.Components(*CR.three_term_problem())


def test_three_term_problem_is_what_it_says(comps):
    spec, theta, X, y, Xs = CR.three_term_problem()
    assert X.shape == (300, 5) and Xs.shape == (75, 5) and comps.T == 3
    assert spec["additive"] and spec["coreg"] == [(2, 3), (3, 2)] and spec["out_col"] == 4 and spec["hetero_noise"] and spec["idx_lin"] == [1]
    cond = np.linalg.cond(O.sigma_matrix(spec, theta, X, dist_mode="direct"))
    print(f"cond(Sigma) = {cond:.3g}")
    assert cond < 1e6


def test_component_means_sum_to_the_prediction(comps):
    mu, _ = O.predict(comps.spec, comps.theta, comps.X, comps.y, comps.Xs, with_noise=False, dist_mode="direct")
    means, _, _ = comps.decompose()
    err = float(np.max(np.abs(means.sum(axis=0) - mu)))
    print(f"sum of means: abs {err:.2e}, rel {err / np.max(np.abs(mu)):.2e}")
    assert err <= 1e-11 * max(1.0, float(np.max(np.abs(mu))))


def test_component_covariances_sum_to_the_noise_free_variance(comps):
    _, var = O.predict(comps.spec, comps.theta, comps.X, comps.y, comps.Xs, with_noise=False, dist_mode="direct")
    _, cov, noise = comps.decompose()
    err = float(np.max(np.abs(cov.sum(axis=(0, 1)) - var)))
    print(f"sum of covariances: abs {err:.2e}")
    assert err <= 1e-11
    assert np.array_equal(noise, O.noise_diag(comps.spec, comps.theta, comps.Xs))
    _, var_n = O.predict(comps.spec, comps.theta, comps.X, comps.y, comps.Xs, with_noise=True, dist_mode="direct")
    assert float(np.max(np.abs(cov.sum(axis=(0, 1)) + noise - var_n))) <= 1e-11


def test_pointwise_component_covariance_is_positive_definite(comps):
    _, cov, _ = comps.decompose()
    assert np.array_equal(cov, cov.transpose(1, 0, 2))
    eig = np.linalg.eigvalsh(cov.transpose(2, 0, 1))
    print(f"smallest eigenvalue over the points: {eig.min():.3e}")
    assert eig.min() > 0.0


def test_selections_agree_with_the_decomposition(comps):
    """``predict_terms`` / ``joint_terms`` of a selection are the decomposition's rows and columns of that selection summed, and
    all terms together are the oracle's prediction."""
    means, cov, noise = comps.decompose()
    for sel in ([0], [1], [2], [0, 2], [1, 2], [0, 1, 2]):
        mu, var = comps.predict_terms(sel, with_noise=False)
        assert np.max(np.abs(mu - means[sel].sum(axis=0))) <= 1e-11
        assert np.max(np.abs(var - cov[np.ix_(sel, sel)].sum(axis=(0, 1)))) <= 1e-11
        jm, C = comps.joint_terms(sel, with_noise=True, jitter=0.0)
        assert np.array_equal(jm, mu) and np.max(np.abs(np.diag(C) - (var + noise))) <= 1e-11
    mu, var = comps.predict_terms(0b111, with_noise=True)
    mu_o, var_o = O.predict(comps.spec, comps.theta, comps.X, comps.y, comps.Xs, with_noise=True, dist_mode="direct")
    assert np.max(np.abs(mu - mu_o)) <= 1e-11 and np.max(np.abs(var - var_o)) <= 1e-11


def test_term_gradients_sum_to_the_total(comps):
    import grad_reference as GR

    total = GR.mean_grad(comps.spec, comps.theta, comps.X, comps.y, comps.Xs)
    parts = sum(comps.grad_terms([t]) for t in range(comps.T))
    assert np.max(np.abs(parts - total)) <= 1e-12 * np.max(np.abs(total))
    assert np.max(np.abs(comps.grad_terms(0b111) - total)) <= 1e-12 * np.max(np.abs(total))


def test_packed_triangle_order():
    cov = np.arange(9.0).reshape(3, 3, 1) + np.arange(9.0).reshape(3, 3, 1).transpose(1, 0, 2)
    assert CR.pack_lower(cov)[:, 0].tolist() == [cov[0, 0, 0], cov[1, 0, 0], cov[1, 1, 0], cov[2, 0, 0], cov[2, 1, 0], cov[2, 2, 0]]


# ---- header, binding, front end ---------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^int {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert "pymc/GP.py:839-841" in header
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    for method in ("predict_decompose", "num_terms"):
        assert hasattr(engine.Engine, method)
    import inspect

    for method in ("predict", "predict_grad", "predict_joint", "draw_joint"):
        assert inspect.signature(getattr(engine.Engine, method)).parameters["terms"].default is None
    assert "terms" not in inspect.signature(engine.Engine.predict_with_grad).parameters


def test_terms_mask_forms():
    from gumbi_amd.engine import terms_mask

    assert terms_mask(5) == 5 and terms_mask([0, 2]) == 5 and terms_mask({1}) == 2 and terms_mask(np.int64(3)) == 3
    assert terms_mask(0) == 0 and terms_mask([]) == 0  # (refused by the engine, which knows the model)
    with pytest.raises(ValueError):
        terms_mask([40])
    with pytest.raises(ValueError):
        terms_mask(-1)


def test_kronecker_and_distributed_engines_refuse_selections():
    from gumbi_amd.distributed import DistributedEngine
    from gumbi_amd.regression.icm import IcmEngine

    with pytest.raises(NotImplementedError, match="Kronecker"):
        IcmEngine.predict(object(), np.zeros((1, 2)), terms=1)
    with pytest.raises(NotImplementedError, match="Kronecker"):
        IcmEngine.predict_decompose(object(), np.zeros((1, 2)))
    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.predict(object(), np.zeros((1, 2)), terms=1)
    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.predict_decompose(object(), np.zeros((1, 2)))


def additive_gp(monkeypatch, additive):
    from test_gpu_frontend import example_gp
    from test_predict_grad_cpu import use_grad_oracle

    use_grad_oracle(monkeypatch)
    gp = example_gp()
    gp.specify_model(outputs=["d", "c"], continuous_dims=["X", "Y"], categorical_dims="Name", additive=additive)
    return gp.build_model()


def test_additive_levels_of_an_additive_and_a_plain_declaration(monkeypatch):
    gp = additive_gp(monkeypatch, True)
    assert gp.model.spec.additive
    assert gp.additive_levels == {"total": 0b11, "global": 0b01, "Name": 0b10}
    assert list(gp.gp_dict) == ["total", "global", "Name"] and all(v is gp.engine for v in gp.gp_dict.values())
    plain = additive_gp(monkeypatch, False)
    assert plain.additive_levels == {"total": 1} and list(plain.gp_dict) == ["total"]


def test_unknown_level_raises_value_error_listing_the_levels(monkeypatch):
    gp = additive_gp(monkeypatch, True)
    for call in (lambda: gp.predict(np.zeros((2, 4)), additive_level="Code"),
                 lambda: gp.predict_grad(np.zeros((2, 4)), additive_level="Code"),
                 lambda: gp.predict_joint(np.zeros((2, 4)), additive_level="Code")):
        with pytest.raises(ValueError, match=r"Code.*total.*global.*Name"):
            call()
    plain = additive_gp(monkeypatch, False)
    with pytest.raises(ValueError, match="total"):
        plain.predict(np.zeros((2, 4)), additive_level="global")
