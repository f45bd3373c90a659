"""Acquisition functions and the gradient-based ``propose_continuous`` on the CPU (``-m "not gpu"``).

1. ``gumbi_amd.acquisition``: the gradients of log-EI and UCB with respect to (mu, sigma^2) against central differences, for
   maximise and minimise; log-EI against the direct formula where that does not underflow, and finite with a usable gradient
   where it does.
2. ``HipGP.propose_continuous`` on an oracle-backed engine (tests/oracle_engine.py's pattern, ``predict_with_grad`` answered by
   tests/var_grad_reference.py): a 1-D fit with a known maximiser.
3. The gradient the search runs on: ``HipGP.acquisition_with_grad`` -- the chained ``dA/dmu dmu/dz + dA/dsigma^2 dsigma^2/dz``
   that ``propose_continuous`` hands to L-BFGS-B -- against central differences of its own value on 2-D models (one output,
   two outputs stacked and in Kronecker form, a categorical dimension), the jac scipy received against it, and the optimised
   restarts against their starts.
"""
import numpy as np
import pandas as pd
import pytest
from scipy.stats import norm

import var_grad_reference as VR
from oracle_engine import OracleEngine


# ---- 1. the acquisitions ---------------------------------------------------------------------------------------------------------
def central(f, x, h):
    return (f(x + h) - f(x - h)) / (2.0 * h)


@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("name", ["EI", "UCB"])
def test_gradients_match_central_differences(name, maximize):
    from gumbi_amd import acquisition as acq

    rng = np.random.default_rng(0)
    mu = rng.uniform(-2.0, 2.0, 200)
    var = rng.uniform(0.01, 1.5, 200)
    f = acq.get(name, best=0.7) if name == "EI" else acq.get(name, beta=2.0)
    value, d_mu, d_var = f(mu, var, maximize)
    # Richardson-extrapolated central differences, h = 1e-3: truncation ~ h^4 f^(5) / 30, rounding ~ eps |f| / h = 2e-13
    fd_mu = (4.0 * central(lambda m: f(m, var, maximize)[0], mu, 5e-4) - central(lambda m: f(m, var, maximize)[0], mu, 1e-3)) / 3.0
    # (in sigma^2 the step is RELATIVE, 1e-3 sigma^2: the variances go down to 0.01, where an absolute 1e-3 is a tenth of the value)
    fd_var = (4.0 * central(lambda v: f(mu, v, maximize)[0], var, 5e-4 * var) - central(lambda v: f(mu, v, maximize)[0], var, 1e-3 * var)) / 3.0
    assert np.max(np.abs(d_mu - fd_mu)) <= 1e-8 * np.max(np.abs(d_mu))
    assert np.max(np.abs(d_var - fd_var)) <= 1e-8 * np.max(np.abs(d_var))


@pytest.mark.parametrize("maximize", [True, False])
def test_log_ei_is_the_logarithm_of_ei_and_survives_underflow(maximize):
    from gumbi_amd import acquisition as acq

    mu = np.linspace(-3.0, 3.0, 61)
    var = np.full_like(mu, 0.49)
    best, s = 0.4, 0.7
    z = (mu - best) / s if maximize else (best - mu) / s
    ei = s * (z * norm.cdf(z) + norm.pdf(z))
    assert np.allclose(acq.expected_improvement(mu, var, best, maximize)[0], np.log(ei), rtol=1e-12, atol=1e-12)
    # 5 to 60 standard deviations on the wrong side of the incumbent (EI underflows beyond ~38): finite, monotone, and the
    # gradient still points towards the incumbent; continuous across the switch to the asymptotic series at z = -30
    far = np.linspace(5.0, 60.0, 221) * s
    mu_far = best - far if maximize else best + far
    value, d_mu, d_var = acq.expected_improvement(mu_far, np.full_like(far, 0.49), best, maximize)
    assert np.all(np.isfinite(value)) and np.all(np.diff(value) < 0)
    assert np.all(d_mu > 0) if maximize else np.all(d_mu < 0)
    assert np.all(d_var > 0)
    near = np.array([-30.0 - 1e-9, -30.0 + 1e-9])
    v = acq.expected_improvement(best + near * s if maximize else best - near * s, np.full(2, 0.49), best, maximize)
    assert abs(v[0][0] - v[0][1]) < 1e-6 and abs(v[1][0] - v[1][1]) < 1e-8 * abs(v[1][0])


def test_ucb_value_and_unknown_names():
    from gumbi_amd import acquisition as acq

    v, dm, dv = acq.upper_confidence_bound(np.array([1.0]), np.array([4.0]), beta=2.0, maximize=True)
    assert np.allclose(v, 1.0 + np.sqrt(2.0) * 2.0) and np.allclose(dm, 1.0) and np.allclose(dv, 0.5 * np.sqrt(2.0) / 2.0)
    v, dm, _ = acq.upper_confidence_bound(np.array([1.0]), np.array([4.0]), beta=2.0, maximize=False)
    assert np.allclose(v, -(1.0 - np.sqrt(2.0) * 2.0)) and np.allclose(dm, -1.0)
    with pytest.raises(ValueError):
        acq.get("PI")


# ---- 2. propose_continuous on an oracle-backed engine ------------------------------------------------------------------------------
class VarGradOracleEngine(OracleEngine):
    """``OracleEngine`` + ``predict_with_grad`` from ``var_grad_reference`` (test infrastructure only); counts its calls."""

    calls = None  # class-level log of M per predict_with_grad call; a test resets it to []

    def predict_with_grad(self, Xs, with_noise=True):
        if not self._factored:
            raise ValueError("no valid factorisation")
        Xs = np.asarray(Xs, float)
        if VarGradOracleEngine.calls is not None:
            VarGradOracleEngine.calls.append(len(Xs))
        return VR.mean_var_grad(self.spec, self.theta, self.X, self.y, Xs, with_noise=with_noise)


def fitted_1d(monkeypatch, n=40):
    import gumbi_amd as gmb
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", VarGradOracleEngine)
    monkeypatch.setattr(icm, "Engine", VarGradOracleEngine)
    monkeypatch.setattr(VarGradOracleEngine, "calls", [])
    rng = np.random.default_rng(5)
    a = np.sort(rng.uniform(0.0, 6.0, n))
    y = 2.0 + np.sin(a) + 0.02 * rng.standard_normal(n)  # maximiser of the surface inside [0, 6]: a = pi / 2
    ds = gmb.DataSet(pd.DataFrame({"a": a, "y": y}), outputs=["y"])
    gp = gmb.GP(ds, outputs="y")
    gp.fit(continuous_dims=["a"], MAP_kwargs={"maxeval": 30})
    return gp, a


@pytest.mark.parametrize("acquisition", ["EI", "UCB"])
def test_proposal_is_inside_the_bounds_and_beats_every_raw_sample(monkeypatch, acquisition):
    gp, a = fitted_1d(monkeypatch)
    prop = gp.propose_continuous(acquisition=acquisition, maximize=True, num_restarts=4, raw_samples=64, seed=3)
    assert prop is gp.proposal and prop.names == ["a"]
    value = float(prop["a"].values().ravel()[0])
    assert a.min() - 1e-9 <= value <= a.max() + 1e-9          # default bounds: the range of the training data
    lo, hi = gp.optimization_bounds
    assert lo.shape == hi.shape == (1,) and lo[0] < hi[0]
    assert gp.proposal_acquisition >= np.max(gp.proposal_raw_acquisition)
    assert abs(value - np.pi / 2) < 0.5                       # the surface's maximiser (EI and UCB both sit near it)
    # every objective evaluation was ONE engine call at M = num_restarts
    assert VarGradOracleEngine.calls and set(VarGradOracleEngine.calls) == {4}
    assert len(VarGradOracleEngine.calls) == gp.proposal_result.nfev


def test_minimising_and_explicit_bounds(monkeypatch):
    gp, a = fitted_1d(monkeypatch)
    bounds = gp.parray(a=np.array([3.0, 6.0]))
    prop = gp.propose_continuous(acquisition="EI", maximize=False, bounds=bounds, num_restarts=3, raw_samples=32, seed=0)
    value = float(prop["a"].values().ravel()[0])
    assert 3.0 - 1e-9 <= value <= 6.0 + 1e-9
    assert abs(value - 3 * np.pi / 2) < 0.5                   # the minimiser of 2 + sin(a) on [3, 6]
    assert gp.proposal_acquisition >= np.max(gp.proposal_raw_acquisition)
    again = gp.propose_continuous(acquisition="EI", maximize=False, bounds=bounds, num_restarts=3, raw_samples=32, seed=0)
    assert float(again["a"].values().ravel()[0]) == value      # seeded: the same proposal


def test_batches_and_unfitted_models_raise(monkeypatch):
    import gumbi_amd as gmb

    gp, _ = fitted_1d(monkeypatch)
    with pytest.raises(NotImplementedError, match="q > 1"):
        gp.propose_continuous(q=2)
    with pytest.raises(ValueError, match='"EI" or "UCB"'):
        gp.propose_continuous(acquisition="PI")
    fresh = gmb.GP(gp.data, outputs="y")
    fresh.specify_model(continuous_dims=["a"])
    fresh.build_model()
    with pytest.raises(ValueError, match="must be fit"):
        fresh.propose_continuous()


# ---- 3. the chained gradient and what the optimiser does with it ------------------------------------------------------------------
def use_oracle(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", VarGradOracleEngine)
    monkeypatch.setattr(icm, "Engine", VarGradOracleEngine)
    monkeypatch.setattr(VarGradOracleEngine, "calls", [])


def fitted_2d(monkeypatch, outputs, kronecker="auto", n=40):
    import gumbi_amd as gmb
    from test_gpu_predict_grad import frontend_dataset

    use_oracle(monkeypatch)
    gp = gmb.GP(frontend_dataset(n, outputs), outputs=outputs if len(outputs) > 1 else outputs[0], kronecker=kronecker)
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 15})
    return gp


def fitted_categorical(monkeypatch):
    from test_joint_cpu import model_2d_categorical

    use_oracle(monkeypatch)
    return model_2d_categorical()


def check_chained_gradient(gp, **kw):
    """``acquisition_with_grad``'s gradient against Richardson-extrapolated central differences (h = 1e-3, h / 2) of its value,
    one coordinate at a time.  Bar 1e-6 max|grad|: the extrapolation's truncation is h^4 f^(5) / 30 = 3e-14 f^(5) and the
    rounding eps |f| / h = 2e-13 |f|; with lengthscales of a few tenths in standardized units f^(5) stays below ~1e5 |f'|, so
    both are orders below the bar, while a wrong sign, column or restart order is an O(1) error."""
    lo, hi = np.asarray(gp.model.X, float)[:, [gp.dims.index(d) for d in gp.continuous_dims]].min(0), None
    hi = np.asarray(gp.model.X, float)[:, [gp.dims.index(d) for d in gp.continuous_dims]].max(0)
    Z = lo + (hi - lo) * np.random.default_rng(11).random((7, len(lo)))
    value, grad = gp.acquisition_with_grad(Z, **kw)
    assert value.shape == (7,) and grad.shape == Z.shape
    fd = np.zeros_like(grad)
    for k in range(Z.shape[1]):
        def central(h):
            E = np.zeros_like(Z)
            E[:, k] = h
            return (gp.acquisition_with_grad(Z + E, **kw)[0] - gp.acquisition_with_grad(Z - E, **kw)[0]) / (2.0 * h)
        fd[:, k] = (4.0 * central(5e-4) - central(1e-3)) / 3.0
    err = float(np.max(np.abs(grad - fd))) / float(np.max(np.abs(grad)))
    print(f"chained gradient vs differences {kw}: {err:.2e}")
    assert np.max(np.abs(grad)) > 0 and err <= 1e-6
    assert np.all(np.abs(grad[:, 0] - grad[:, 1]) > 0)  # (two different columns: a swapped mapping cannot hide)
    return Z, value, grad


@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("acquisition", ["EI", "UCB"])
def test_chained_gradient_matches_differences_of_the_acquisition(monkeypatch, acquisition, maximize):
    gp = fitted_2d(monkeypatch, ["y"])
    check_chained_gradient(gp, acquisition=acquisition, maximize=maximize)


def recomputed(gp, prop, output, acquisition, maximize, best=None, levels=None):
    """The acquisition at ``prop`` from the public ``predict_points`` (noise-free), in standardized units."""
    from gumbi_amd import acquisition as acq

    pts = gp.append_categorical_points(prop, levels) if levels else prop
    pz = gp.predict_points(pts, output=output, with_noise=False).z
    f = acq.get(acquisition, best=best) if acquisition == "EI" else acq.get(acquisition)
    return float(f(np.ravel(pz.μ), np.ravel(pz.σ2), maximize)[0][0])


def test_the_optimiser_receives_that_gradient_and_improves_on_its_starts(monkeypatch):
    gp = fitted_2d(monkeypatch, ["y"])
    n = 5
    prop = gp.propose_continuous(acquisition="EI", maximize=True, num_restarts=n, raw_samples=40, seed=2, gtol=1e-9, ftol=1e-15)
    res = gp.proposal_result
    # the jac scipy holds at its last point IS minus the chained gradient, restart by restart, coordinate by coordinate
    value, grad = gp.acquisition_with_grad(res.x.reshape(n, 2), acquisition="EI", maximize=True)
    assert np.array_equal(res.jac, -grad.ravel()) and res.fun == -float(np.sum(value))
    # the lock-step run strictly improved on the starts (the best n raw samples) ...
    start_total = float(np.sum(np.sort(gp.proposal_raw_acquisition)[-n:]))
    print(f"summed log EI: starts {start_total:.6f} -> optimised {-res.fun:.6f} in {res.nit} iterations")
    assert res.nit >= 1 and -res.fun > start_total + 1e-6
    # ... and ended at a first-order optimum of the box-constrained problem, coordinate by coordinate: dA/dz = 0 for a coordinate
    # strictly inside its bounds, pointing out of the box for one on a bound (gtol = 1e-9 was asked for; 1e-5 is the bar)
    lo, hi = gp.optimization_bounds
    Zr = res.x.reshape(n, 2)
    at_lo, at_hi = Zr <= lo + 1e-12, Zr >= hi - 1e-12
    free = ~(at_lo | at_hi)
    print(f"free coordinates {int(free.sum())} of {free.size}, max |dA/dz| on them {np.max(np.abs(grad[free])):.2e}")
    assert free.any() and np.max(np.abs(grad[free])) <= 1e-5
    assert np.all(grad[at_lo] <= 1e-5) and np.all(grad[at_hi] >= -1e-5)
    assert gp.proposal_acquisition > np.max(gp.proposal_raw_acquisition)
    best = float(np.max(gp.model.y))
    assert abs(recomputed(gp, prop, None, "EI", True, best=best) - gp.proposal_acquisition) <= 1e-8 * max(1.0, abs(gp.proposal_acquisition))


@pytest.mark.parametrize("kronecker", [False, "auto"])
def test_one_output_among_several(monkeypatch, kronecker):
    """Two outputs, stacked and in Kronecker form: ``output`` picks the task column of the points and the EI incumbent."""
    from gumbi_amd.regression import icm

    gp = fitted_2d(monkeypatch, ["y", "w"], kronecker=kronecker)
    assert isinstance(gp.engine, icm.IcmEngine) == (kronecker == "auto")
    with pytest.raises(ValueError, match="ONE output"):
        gp.propose_continuous()
    check_chained_gradient(gp, output="w", acquisition="EI", maximize=True)
    va = gp.acquisition_with_grad(np.zeros((1, 2)), output="y")[0]
    vb = gp.acquisition_with_grad(np.zeros((1, 2)), output="w")[0]
    assert va[0] != vb[0]
    prop = gp.propose_continuous(output="w", acquisition="EI", maximize=True, num_restarts=3, raw_samples=24, seed=4)
    X, y = np.asarray(gp.model.X, float), np.asarray(gp.model.y, float)
    oc = gp.dims.index(gp.out_col)
    best = float(np.max(y[X[:, oc] == gp.categorical_coords[gp.out_col]["w"]]))  # the incumbent: the best observed w
    got = recomputed(gp, prop, "w", "EI", True, best=best)
    assert abs(got - gp.proposal_acquisition) <= 1e-8 * max(1.0, abs(gp.proposal_acquisition))
    assert gp.proposal_acquisition >= np.max(gp.proposal_raw_acquisition)


def test_categorical_levels_fix_the_categories(monkeypatch):
    gp = fitted_categorical(monkeypatch)
    levels = gp.categorical_levels["Name"]
    with pytest.raises(AttributeError, match="every categorical dimension"):
        gp.propose_continuous()
    cat0, cat1 = {"Name": levels[0]}, {"Name": levels[1]}
    check_chained_gradient(gp, categorical_levels=cat1, acquisition="UCB", maximize=False)
    v0 = gp.acquisition_with_grad(np.zeros((1, 2)), categorical_levels=cat0, acquisition="UCB")[0]
    v1 = gp.acquisition_with_grad(np.zeros((1, 2)), categorical_levels=cat1, acquisition="UCB")[0]
    assert v0[0] != v1[0]
    prop = gp.propose_continuous(acquisition="UCB", maximize=False, categorical_levels=cat1, num_restarts=3, raw_samples=24, seed=4,
                                 beta=2.0)
    assert set(prop.names) == {"X", "Y"}
    got = recomputed(gp, prop, None, "UCB", False, levels=cat1)
    assert abs(got - gp.proposal_acquisition) <= 1e-8 * max(1.0, abs(gp.proposal_acquisition))


def test_beta_never_reaches_the_optimiser(monkeypatch):
    import warnings

    gp, _ = fitted_1d(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # scipy warns about unknown options
        gp.propose_continuous(acquisition="EI", beta=3.0, num_restarts=2, raw_samples=8, seed=0)
        a = gp.propose_continuous(acquisition="UCB", beta=0.0, num_restarts=2, raw_samples=8, seed=0)
    # beta = 0: UCB is the mean, whose maximiser over [0, 6] is pi / 2
    assert abs(float(a["a"].values().ravel()[0]) - np.pi / 2) < 0.3


def test_distributed_engines_refuse():
    from gumbi_amd.distributed import DistributedEngine

    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.predict_with_grad(object(), np.zeros((1, 1)))
