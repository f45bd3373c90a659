"""Periodic kernels without a GPU (``-m "not gpu"``): the numpy reference of tests/periodic_reference.py against the two PyMC
formulas, its gradient against central differences, and the front end (``build_model(continuous_kernel="Periodic" |
"<kind>+Periodic", period=...)``, reference gumbi/regression/pymc/GP.py:416-447, 664-682) on the engine-shaped stand-in.

tests/test_gpu_periodic.py compares libgumbi_hip.so with the same reference.
"""
import ctypes

import numpy as np
import pytest

import periodic_reference as PR
from oracle import gp_oracle as O
from test_joint_cpu import STDZR, dataset, points_1d

FORMS = [("ExpQuad", 2)] + [(k, 1) for k in O.KINDS]  # "Periodic" and the five "<kind>+Periodic"


def _case(kind, mode, n_cont, ard=True, N=60, seed=5):
    rng = np.random.default_rng(seed + n_cont)
    X = rng.standard_normal((N, n_cont))
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(N)
    ls = rng.uniform(0.7, 1.6, n_cont)
    periods = rng.uniform(2.5, 4.0, n_cont)
    spec = O.make_spec(n_cont, range(n_cont), kind=kind, ard=ard)
    theta = O.pack_theta(spec, ls if ard else ls[:1], 1.3, 0.3)
    return spec, theta, X, y, (ls if ard else np.repeat(ls[:1], n_cont)), periods


@pytest.mark.parametrize("kind,mode,n_cont", [("ExpQuad", 2, 1), ("ExpQuad", 2, 3)] + [(k, 1, 1) for k in O.KINDS])
@pytest.mark.parametrize("ard", [True, False])
def test_warped_oracle_is_the_pymc_formula(kind, mode, n_cont, ard):
    spec, theta, X, y, ls, periods = _case(kind, mode, n_cont, ard)
    w = PR.Warped(spec, mode, periods)
    Xs = np.random.default_rng(1).standard_normal((23, n_cont)) * 2.0
    for other in (None, Xs):
        got = w.cov(theta, X, other)
        want = PR.direct_cov(kind, mode, ls, 1.3, periods, X, other)
        err = np.max(np.abs(got - want))
        print(f"{kind} mode {mode} n_cont {n_cont} ard {ard}: max |warped - direct| = {err:.2e}")
        assert err <= 1e-13


def test_plus_periodic_per_dimension_form_in_three_dimensions():
    """The per-dimension form this project implements for n_cont > 1 (the reference's own is only well-formed for one)."""
    spec, theta, X, y, ls, periods = _case("Matern32", 1, 3)
    got = PR.Warped(spec, 1, periods).cov(theta, X)
    assert np.max(np.abs(got - PR.direct_cov("Matern32", 1, ls, 1.3, periods, X))) <= 1e-13


@pytest.mark.parametrize("kind,mode", FORMS)
@pytest.mark.parametrize("ard", [True, False])
def test_reference_gradient_matches_central_differences(kind, mode, ard):
    """Same step and bound as tests/test_oracle.py::test_gradient_matches_finite_differences."""
    spec, theta, X, y, ls, periods = _case(kind, mode, 3, ard, N=90, seed=11)
    w = PR.Warped(spec, mode, periods)
    val, g = w.nlml_and_grad(theta, X, y)
    assert g.shape == theta.shape and np.isclose(val, w.nlml(theta, X, y), rtol=1e-12)
    h = 1e-6
    for i in range(theta.size):
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = (w.nlml(tp, X, y) - w.nlml(tm, X, y)) / (2 * h)
        assert abs(fd - g[i]) <= 2e-6 * max(1.0, abs(g[i])), (i, fd, g[i])


def test_reference_gradient_of_an_additive_model():
    rng = np.random.default_rng(3)
    N = 70
    X = np.column_stack([rng.standard_normal((N, 2)), rng.integers(0, 3, N)])
    y = rng.standard_normal(N)
    spec = O.make_spec(3, [0, 1], kind="Matern52", coreg=[(2, 3)], additive=True)
    theta = np.concatenate([[0.9, 1.2, 1.1, 0.3], rng.standard_normal(6) * 0.5, [0.8, 1.1, 0.9], [1.3, 0.8, 0.7]])
    assert theta.size == O.theta_size(spec)
    w = PR.Warped(spec, 1, [3.0, 2.6])
    _, g = w.nlml_and_grad(theta, X, y)
    h = 1e-6
    for i in range(theta.size):
        tp, tm = theta.copy(), theta.copy()
        tp[i] += h
        tm[i] -= h
        fd = (w.nlml(tp, X, y) - w.nlml(tm, X, y)) / (2 * h)
        assert abs(fd - g[i]) <= 2e-5 * max(1.0, abs(g[i])), (i, fd, g[i])  # (test_oracle.py's bound for additive models)


# ---- front end on the stand-in engine ---------------------------------------------------------------------------------
def _stdzr():
    import gumbi_amd as gmb

    return gmb.Standardizer(**{k: dict(v) for k, v in STDZR.items()}, log_vars=["d", "c", "Y"], logit_vars=["X"])


def _period(**steps):
    from gumbi_amd.array_utils import make_deltas_parray

    return make_deltas_parray(stdzr=_stdzr(), scale="standardized", **{k: [v] for k, v in steps.items()})


@pytest.mark.parametrize("name,kind,mode", [("Periodic", "ExpQuad", 2), ("Matern52+Periodic", "Matern52", 1)])
def test_front_end_builds_fits_predicts_and_draws(monkeypatch, name, kind, mode):
    import gumbi_amd as gmb

    PR.use_periodic_oracle(monkeypatch)
    gp = gmb.GP(dataset(), outputs="d", seed=3)
    gp.specify_model(continuous_dims=["X", "Y"])
    period = _period(Y=3.25, X=2.5)  # (layer order is not the order of continuous_dims)
    gp.build_model(continuous_kernel=name, period=period)
    assert gp.model.spec.kind == kind and gp.model.spec.periodic == mode and gp.model_specs["continuous_kernel"] == name
    # the engine received (mode, period.z of each dimension in continuous_dims order)
    want = [float(np.squeeze(period.z[d + "_z"].values())) for d in gp.continuous_dims]
    assert gp.continuous_dims == ["X", "Y"] and np.allclose(want, [2.5, 3.25], rtol=1e-12, atol=0)  # (X is a logit variable)
    TX, TY = want
    assert PR.PeriodicOracleEngine.received == [(mode, want)]
    assert gp.model.spec.theta_size() == 4  # periods are data, not parameters
    gp.find_MAP(maxeval=25)
    assert np.all(np.isfinite(gp.nlml_trace)) and len(gp.nlml_trace) >= 2
    gp.prepare_grid(resolution=6)
    pred = gp.predict_grid()
    assert pred.shape == (6, 6) and np.all(np.isfinite(pred.z.μ)) and np.all(pred.z.σ2 > 0)
    draws = gp.draw_grid_samples(n_draws=3)
    assert draws.shape == (3, 6, 6) and np.all(np.isfinite(draws.z.values()))
    # the posterior repeats with the period in every dimension
    rng = np.random.default_rng(0)
    Xs = rng.standard_normal((40, 2))
    mu, var = gp.predict(Xs)
    for shift in ([TX, 0.0], [0.0, -TY], [2 * TX, TY]):
        mu2, var2 = gp.predict(Xs + np.array(shift))
        assert np.max(np.abs(mu2 - mu)) <= 1e-10 and np.max(np.abs(var2 - var)) <= 1e-10
    mu3, _ = gp.predict(Xs + np.array([1.0, 0.0]))
    assert np.max(np.abs(mu3 - mu)) > 1e-4  # (and with nothing else)


def test_every_periodic_name_builds_and_needs_a_period(monkeypatch):
    import gumbi_amd as gmb
    from gumbi_amd.engine import KERNEL_KINDS, resolve_kernel_name

    PR.use_periodic_oracle(monkeypatch)
    names = ["Periodic"] + [k + "+Periodic" for k in KERNEL_KINDS]
    assert len(names) == 6 and list(KERNEL_KINDS) == ["ExpQuad", "Matern52", "Matern32", "Matern12", "Exponential"]
    for name in names:
        gp = gmb.GP(dataset(), outputs="d")
        gp.specify_model(continuous_dims=["X"])
        with pytest.raises(ValueError, match="[Pp]eriod"):
            gp.build_model(continuous_kernel=name)
        period = _period(X=2.0)
        T = float(np.squeeze(period.z["X_z"].values()))
        gp.build_model(continuous_kernel=name, period=period)
        kind, mode = resolve_kernel_name(name)
        assert (gp.model.spec.kind, gp.model.spec.periodic, gp.model.spec.periods) == (kind, mode, [T]) and abs(T - 2.0) < 1e-12
        gp.find_MAP(maxeval=3)
        mu, _ = gp.predict(np.array([[0.3], [0.3 + T]]))
        assert abs(mu[0] - mu[1]) <= 1e-10
    for k in KERNEL_KINDS:
        assert resolve_kernel_name(k) == (k, 0)
    with pytest.raises(ValueError):
        resolve_kernel_name("Cosine+Periodic")


def test_partial_period_too_many_dimensions_and_distributed_are_refused(monkeypatch):
    import gumbi_amd as gmb

    PR.use_periodic_oracle(monkeypatch)
    gp = gmb.GP(dataset(), outputs="d")
    gp.specify_model(continuous_dims=["X", "Y"])
    with pytest.raises(ValueError, match="Y"):
        gp.build_model(continuous_kernel="ExpQuad+Periodic", period=_period(X=2.0))
    with pytest.raises(ValueError):
        gp.build_model(continuous_kernel="Periodic", period=_period(X=2.0))
    # a non-periodic kernel ignores nothing silently: it builds as before, with the mode off
    gp.build_model(continuous_kernel="ExpQuad")
    assert gp.model.spec.periodic == 0 and PR.PeriodicOracleEngine.received[-1] == (0, [])

    # nine continuous dimensions: two prepared columns each do not fit the engine's sixteen
    import pandas as pd

    rng = np.random.default_rng(1)
    dims = [f"x{i}" for i in range(9)]
    df = pd.DataFrame(rng.standard_normal((30, 10)), columns=dims + ["out"])
    ds = gmb.DataSet(df, outputs=["out"], stdzr=gmb.Standardizer(**{n: {"μ": 0.0, "σ2": 1.0} for n in dims + ["out"]}))
    from gumbi_amd.array_utils import make_deltas_parray

    per9 = make_deltas_parray(stdzr=ds.stdzr, scale="standardized", **{n: [2.0] for n in dims})
    for name in ("Periodic", "Matern32+Periodic"):
        gp9 = gmb.GP(ds, outputs="out")
        gp9.specify_model(continuous_dims=dims)
        with pytest.raises(ValueError, match="at most 8"):
            gp9.build_model(continuous_kernel=name, period=per9)
    gp8 = gmb.GP(ds, outputs="out")
    gp8.specify_model(continuous_dims=dims[:8])
    gp8.build_model(continuous_kernel="Periodic", period=per9)  # (further layers of `period` are not an error)
    assert len(gp8.model.spec.periods) == 8

    gpd = gmb.GP(dataset(), outputs="d", distributed=True)
    gpd.specify_model(continuous_dims=["X"])
    with pytest.raises(NotImplementedError, match="distributed"):
        gpd.build_model(continuous_kernel="Periodic", period=_period(X=2.0))


def test_kronecker_engine_forwards_the_periods(monkeypatch):
    import gumbi_amd as gmb
    from gumbi_amd.regression import icm

    PR.use_periodic_oracle(monkeypatch)
    gp = gmb.GP(dataset(), outputs=["d", "c"])
    gp.specify_model(continuous_dims=["X"])
    period = _period(X=2.5)
    T = float(np.squeeze(period.z["X_z"].values()))
    gp.build_model(continuous_kernel="Matern32+Periodic", period=period)
    assert isinstance(gp.engine, icm.IcmEngine)
    gp.find_MAP(maxeval=4)
    assert PR.PeriodicOracleEngine.received and all(r == (1, [T]) for r in PR.PeriodicOracleEngine.received)
    pts = points_1d(gp, M=5)
    pa, _, _ = gp._prepare_points_for_prediction(pts, output=["d", "c"])
    mu, var = gp.predict(pa)
    shifted = pa.copy()
    shifted[:, 0] += T
    mu2, var2 = gp.predict(shifted)
    assert np.max(np.abs(mu2 - mu)) <= 1e-10 and np.max(np.abs(var2 - var)) <= 1e-10


def test_kernel_spec_carries_the_periods_beside_the_struct():
    from gumbi_amd.engine import KernelSpec, _Spec

    spec = KernelSpec(D=3, idx_cont=[0, 2], kind="Matern52", periodic=1, periods=[2.0, 3.5])
    d = spec.as_dict()
    assert d["periodic"] == 1 and d["periods"] == [2.0, 3.5] and d["kind"] == 1
    again = KernelSpec(**{**d, "kind": "Matern52"})
    assert again.as_dict() == d
    assert KernelSpec(D=1, idx_cont=[0]).as_dict()["periodic"] == 0 and KernelSpec(D=1, idx_cont=[0]).as_dict()["periods"] == []
    assert ctypes.sizeof(_Spec) == 176 and ctypes.sizeof(spec.to_c()) == 176  # the periods do not travel inside gmb_kernel_spec
    assert spec.theta_size() == KernelSpec(D=3, idx_cont=[0, 2], kind="Matern52").theta_size()
    with pytest.raises(ValueError, match="at most 8"):
        KernelSpec(D=9, idx_cont=list(range(9)), periodic=2, periods=[1.0] * 9).to_c()
    with pytest.raises(ValueError, match="periods"):
        KernelSpec(D=2, idx_cont=[0, 1], periodic=1, periods=[1.0]).to_c()


@pytest.mark.parametrize("name", ["Periodic", "Matern32+Periodic"])
def test_cross_validate_rebuilds_a_periodic_model(monkeypatch, name):
    """``cross_validate`` rebuilds the training model from ``model_specs``: the periods travel in it."""
    import gumbi_amd as gmb

    PR.use_periodic_oracle(monkeypatch)
    gp = gmb.GP(dataset(), outputs="d", seed=3)
    gp.specify_model(continuous_dims=["X"])
    period = _period(X=2.5)
    T = float(np.squeeze(period.z["X_z"].values()))
    gp.build_model(continuous_kernel=name, period=period)
    assert gp.model_specs["period"] is period
    gp.find_MAP(maxeval=5)
    n_before = len(PR.PeriodicOracleEngine.received)
    cv = gp.cross_validate(pct_train=0.7, seed=1, maxeval=5)
    mode = gp.model.spec.periodic
    assert PR.PeriodicOracleEngine.received[n_before:] == [(mode, [T])]  # the split's engine got the same kernel
    for part in ("train", "test"):
        assert np.all(np.isfinite(cv[part]["NLPDs"])) and np.all(np.isfinite(cv[part]["errors"]))
    # a model that is not periodic keeps the specs it had
    gp.build_model(continuous_kernel="ExpQuad")
    assert "period" not in gp.model_specs
