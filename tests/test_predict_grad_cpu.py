"""The gradient of the posterior mean on the CPU (``-m "not gpu"``: runs anywhere).

1. ``grad_reference.mean_grad`` -- the closed form the HIP kernel implements, in numpy -- against Richardson-extrapolated
   central differences (h = 1e-3 and h / 2) of ``cov_full(...) @ alpha``, at test points 0.3 sigma off training points.
   Bars: 1e-9 of max|G| for ExpQuad / Matern52 / Matern32, 1e-7 for Matern12 / Exponential (whose third derivative is large
   near a training point: the differences, not the formula, set that error).  Worst errors measured when this file was
   written (N = 300, d = 3 unless stated):

       ExpQuad 4.4e-11   Matern52 1.5e-11   Matern32 7.2e-11   Matern12 5.3e-9   Exponential 3.9e-9
       composite N = 140 (linear + coregion + two outputs) 3.7e-11      additive N = 300 3.6e-10
       Matern52+Periodic d = 2 2.5e-11      Periodic d = 2 2.1e-11      shared lengthscale 2.3e-11

2. The front end -- ``HipGP.predict_grad`` / ``predict_points_grad`` / ``predict_grid_grad`` / ``_get_pgrad_norm`` and
   ``IcmEngine.predict_grad`` -- on an oracle-backed stand-in of the engine (tests/oracle_engine.py's pattern).
"""
import numpy as np
import pandas as pd
import pytest

import grad_reference as GR
import periodic_reference as PR
from oracle import gp_oracle as O
from oracle_engine import OracleEngine
from test_gpu_predict_grad import frontend_dataset, points, table
from test_gpu_parity import GOLD, golden_spec, rel


# ---- 1. the reference against finite differences -----------------------------------------------------------------------------
def fd_error(spec, theta, X, y, Xs, periodic=0, periods=None):
    G = GR.mean_grad(spec, theta, X, y, Xs, periodic=periodic, periods=periods)
    fd = GR.fd_mean_grad(GR.posterior_mean(spec, theta, X, y, periodic=periodic, periods=periods), Xs, spec["idx_cont"])
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
    case = "composite_N140"
    spec, theta, X, y = golden_spec(case), GOLD[f"{case}/theta"], GOLD[f"{case}/X"], GOLD[f"{case}/y"]
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


def test_kinked_kinds_have_zero_gradient_contribution_at_a_coincident_point():
    """Matern12 keeps sqrt(r^2 + 1e-12): the pair (x*, x_n) with x* = x_n contributes exactly 0, and the gradient stays finite."""
    spec, theta, X, y = table(120, 2, "Matern12")
    G = GR.mean_grad(spec, theta, X, y, X[:10])
    assert np.all(np.isfinite(G))


# ---- 2. the front end on an oracle-backed engine -----------------------------------------------------------------------------
class GradOracleEngine(PR.PeriodicOracleEngine):
    """``PeriodicOracleEngine`` + ``predict_grad`` from ``grad_reference`` (test infrastructure only)."""

    def predict_grad(self, Xs):
        Xs = np.asarray(Xs, float)
        if not self._factored:
            raise ValueError("no valid factorisation")
        if self._w is None:
            return GR.mean_grad(self.spec, self.theta, self.X, self.y, Xs)
        raise NotImplementedError


def use_grad_oracle(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", GradOracleEngine)
    monkeypatch.setattr(icm, "Engine", GradOracleEngine)


def fitted(monkeypatch, outputs, kronecker="auto", n=40):
    import gumbi_amd as gmb

    use_grad_oracle(monkeypatch)
    gp = gmb.GP(frontend_dataset(n, outputs), outputs=outputs if len(outputs) > 1 else outputs[0], kronecker=kronecker)
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 10})
    return gp


def test_point_gradient_layers_and_scaling(monkeypatch):
    gp = fitted(monkeypatch, ["y"])
    pts = gp.parray(a=np.linspace(0.8, 3.5, 9), b=np.linspace(11.0, 19.0, 9))
    grad = gp.predict_points_grad(pts, norm=False)
    assert grad.names == ["δ[y]/δ[a]", "δ[y]/δ[b]"] and grad.shape == (9,)
    pa, _, _ = gp._prepare_points_for_prediction(pts, output=["y"])
    Gz = GR.mean_grad(gp.model.spec.as_dict(), gp._theta_fitted, gp.model.X, gp.model.y, pa)
    assert np.array_equal(gp.predict_grad(pa), Gz)
    sy = np.sqrt(gp.stdzr["y"]["σ2"])
    want = {x: Gz[:, gp.dims.index(x)] * sy / np.sqrt(gp.stdzr[x]["σ2"]) for x in ("a", "b")}
    for x in ("a", "b"):
        assert np.allclose(grad[f"δ[y]/δ[{x}]"].values(), want[x], rtol=1e-14, atol=0)
    norm = gp.predict_points_grad(pts)
    assert norm.names == ["|∇|y"]
    assert np.allclose(norm["|∇|y"].values(), np.sqrt(want["a"] ** 2 + want["b"] ** 2), rtol=1e-14, atol=0)


def test_gradient_column_follows_the_model_dimension_order(monkeypatch):
    """The layer of a continuous dim takes ITS column of the engine's (M, D) gradient, wherever that dim sits in ``dims``."""
    gp = fitted(monkeypatch, ["y"])
    marker = np.arange(1.0, 1.0 + len(gp.dims))
    monkeypatch.setattr(gp.engine, "predict_grad", lambda Xs: np.tile(marker, (len(Xs), 1)))
    pts = gp.parray(a=np.array([1.0, 2.0]), b=np.array([12.0, 13.0]))
    grad = gp.predict_points_grad(pts, norm=False)
    for x in ("a", "b"):
        scale = np.sqrt(gp.stdzr["y"]["σ2"]) / np.sqrt(gp.stdzr[x]["σ2"])
        assert np.allclose(grad[f"δ[y]/δ[{x}]"].values(), marker[gp.dims.index(x)] * scale)


def test_grid_gradient_has_the_grid_shape(monkeypatch):
    gp = fitted(monkeypatch, ["y"])
    with pytest.raises(ValueError, match="prepare_grid"):
        gp.predict_grid_grad()
    gp.prepare_grid(resolution=6)
    grad = gp.predict_grid_grad(norm=False)
    assert grad.shape == (6, 6) and grad.names == ["δ[y]/δ[a]", "δ[y]/δ[b]"]
    flat = gp.predict_points_grad(gp.grid_points, norm=False)
    assert np.array_equal(grad["δ[y]/δ[a]"].values().ravel(), flat["δ[y]/δ[a]"].values())
    assert gp.predict_grid_grad().names == ["|∇|y"]


def test_two_outputs_on_stacked_points(monkeypatch):
    gp = fitted(monkeypatch, ["y", "w"], kronecker=False)
    pts = gp.parray(a=np.linspace(0.8, 3.5, 7), b=np.linspace(11.0, 19.0, 7))
    grad = gp.predict_points_grad(pts, norm=False)
    assert grad.names == ["δ[y]/δ[a]", "δ[y]/δ[b]", "δ[w]/δ[a]", "δ[w]/δ[b]"] and grad.shape == (7,)
    pa, tall, coords = gp._prepare_points_for_prediction(pts, output=["y", "w"])
    Gz = GR.mean_grad(gp.model.spec.as_dict(), gp._theta_fitted, gp.model.X, gp.model.y, pa)
    out_col = gp.dims.index(gp.out_col)
    for name, coord in zip(["y", "w"], coords):
        rows = Gz[pa[:, out_col] == coord]
        want = rows[:, gp.dims.index("b")] * np.sqrt(gp.stdzr[name]["σ2"]) / np.sqrt(gp.stdzr["b"]["σ2"])
        assert np.allclose(grad[f"δ[{name}]/δ[b]"].values(), want, rtol=1e-14, atol=0)
    assert gp.predict_points_grad(pts).names == ["|∇|y", "|∇|w"]
    one = gp.predict_points_grad(pts, output="w", norm=False)
    assert one.names == ["δ[w]/δ[a]", "δ[w]/δ[b]"]
    assert np.array_equal(one["δ[w]/δ[a]"].values(), grad["δ[w]/δ[a]"].values())


def test_kronecker_combination_equals_the_stacked_gradient(monkeypatch):
    """``IcmEngine.predict_grad`` (the P systems' gradients combined) against the stacked model's gradient at the same
    hyper-parameters; 1e-8 relative, the bar of the Kronecker engine against the oracle (tests/test_gpu_configs.py)."""
    from gumbi_amd.regression import icm

    gk = fitted(monkeypatch, ["y", "w"], kronecker="auto")
    assert isinstance(gk.engine, icm.IcmEngine)
    pts = gk.parray(a=np.linspace(0.8, 3.5, 11), b=np.linspace(11.0, 19.0, 11))
    pa, _, _ = gk._prepare_points_for_prediction(pts, output=["y", "w"])
    G = gk.predict_grad(pa)
    ref = GR.mean_grad(gk.model.spec.as_dict(), gk._theta_fitted, gk.model.X, gk.model.y, pa)
    print(f"Kronecker vs stacked: {rel(G, ref):.2e}")
    assert rel(G, ref) < 1e-8
    assert not np.any(G[:, -1])


def test_unfitted_models_and_sublevels_raise(monkeypatch):
    import gumbi_amd as gmb

    use_grad_oracle(monkeypatch)
    gp = gmb.GP(frontend_dataset(30, ["y"]), outputs="y")
    gp.specify_model(continuous_dims=["a", "b"])
    gp.build_model()
    with pytest.raises(ValueError, match="must be fit"):
        gp.predict_grad(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="must be fit"):
        gp.predict_points_grad(gp.parray(a=np.array([1.0]), b=np.array([12.0])))
    with pytest.raises(NotImplementedError):
        gp.predict_grad(np.zeros((3, 2)), additive_level="Name")


def test_distributed_engines_refuse():
    from gumbi_amd.distributed import DistributedEngine

    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.predict_grad(object(), np.zeros((1, 1)))
