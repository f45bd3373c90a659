"""Appending observations to the resident factor, on the CPU (``-m "not gpu"``):

1. the algebra -- tests/append_reference.py's bordered update, plain and by the engine's block route, against ``O.factorize`` at
   N + K on ``O.synthetic_table`` with sigma = 0.2;
2. the ABI -- the header declares ``gmb_append`` / ``gmb_truncate`` / ``gmb_blk_gemm_splitk``, engine.py binds them, version 16;
3. ``HipGP.condition_on`` and ``HipGP.propose_continuous(q, sequential=True)`` on an oracle-backed engine whose ``append`` and
   ``truncate`` are concatenation and slicing (tests/append_reference.py: ``AppendOracleEngine``) and count their calls.
"""
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

import append_reference as AR
from oracle import gp_oracle as O
from test_acquisition_cpu import VarGradOracleEngine

ROOT = Path(__file__).resolve().parent.parent


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


# ---- 1. the algebra ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(300, 200), (1000, 16), (383, 1), (120, 20)])
def test_bordered_update_equals_a_fresh_factorisation(N, K):
    X, y, ls = O.synthetic_table(N + K, 2, sigma=0.2)
    spec = O.make_spec(2, range(2), kind="ExpQuad")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    L_r, v_r = O.factorize(spec, theta, X, y, dist_mode="direct")
    nlml_r = O.nlml(spec, theta, X, y, dist_mode="direct")
    L, v, nlml = AR.append(spec, theta, X[:N], y[:N], X[N:], y[N:])
    print(f"bordered ({N}, {K}): L {rel(L, L_r):.2e} v {rel(v, v_r):.2e} nlml {abs(nlml - nlml_r) / abs(nlml_r):.2e}")
    # three orders inside the GPU tests' 1e-10 (the issue's own figures: 1.3e-14 and 1.3e-13)
    assert rel(L, L_r) <= 1e-13 and rel(v, v_r) <= 1e-12 and abs(nlml - nlml_r) <= 1e-13 * abs(nlml_r)
    # the engine's route: keep floor(N / 128) block columns, rebuild every row behind them
    Lb, vb, I0 = AR.blocked_append(spec, theta, X, y, N, N + K)
    assert I0 == N // 128
    assert rel(Lb, L_r) <= 1e-13 and rel(vb, v_r) <= 1e-12
    # ... and back: truncation keeps floor(n / 128) block columns of the LARGER factor
    Lt, vt, I0t = AR.blocked_append(spec, theta, X, y, N + K, N)
    assert I0t == N // 128
    assert rel(Lt, L_r[:N, :N]) <= 1e-13


def test_layout_sizes():
    assert AR.layout(100) == (128, 128) and AR.layout(127) == (128, 128) and AR.layout(128) == (128, 256)
    assert AR.layout(383) == (384, 384) and AR.layout(384) == (384, 512) and AR.layout(10000) == AR.layout(10001)


# ---- 2. the ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_entry_points():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    assert re.search(r"#define\s+GMB_ABI_VERSION\s+16\b", header)
    assert engine.ABI_VERSION == 16
    for name in ("gmb_append", "gmb_truncate", "gmb_blk_gemm_splitk"):
        assert re.search(rf"\bint\s+{name}\s*\(", header), name
        assert name in engine.exported_symbols(), name
    assert len(engine._SIGNATURES["gmb_append"][1]) == 6 and len(engine._SIGNATURES["gmb_truncate"][1]) == 2
    assert len(engine._SIGNATURES["gmb_blk_gemm_splitk"][1]) == 15
    assert re.search(r"\bint64_t\s+gmb_num_obs\s*\(", header) and "gmb_num_obs" in engine.exported_symbols()
    for method in ("append", "truncate", "blk_gemm_splitk"):
        assert callable(getattr(engine.Engine, method))


def test_kronecker_and_distributed_engines_refuse():
    from gumbi_amd.distributed import DistributedEngine
    from gumbi_amd.regression.icm import IcmEngine

    for cls, word in ((IcmEngine, "Kronecker"), (DistributedEngine, "distributed")):
        with pytest.raises(NotImplementedError, match=word):
            cls.append(object(), np.zeros((1, 1)), np.zeros(1))
        with pytest.raises(NotImplementedError, match=word):
            cls.truncate(object(), 1)


# ---- 3. the front end ---------------------------------------------------------------------------------------------------------------
class CountingEngine(AR.AppendOracleEngine, VarGradOracleEngine):
    pass


def use_engine(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", CountingEngine)
    monkeypatch.setattr(icm, "Engine", CountingEngine)
    monkeypatch.setattr(CountingEngine, "appends", 0)
    monkeypatch.setattr(CountingEngine, "truncates", 0)
    monkeypatch.setattr(CountingEngine, "log", [])
    monkeypatch.setattr(VarGradOracleEngine, "calls", None)


def table(n, seed=0):
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 4.0, n), rng.uniform(10.0, 20.0, n)
    lot = rng.choice(["k", "m", "z"], n)
    y = 3.0 + np.sin(a) * np.cos(0.3 * b) + 0.3 * (lot == "m") - 0.2 * (lot == "z") + 0.05 * rng.standard_normal(n)
    return pd.DataFrame({"a": a, "b": b, "lot": lot, "y": y})


def fitted(monkeypatch, df, categorical=True, **gp_kwargs):
    import gumbi_amd as gmb

    use_engine(monkeypatch)
    gp = gmb.GP(gmb.DataSet(df, outputs=["y"]), outputs="y", **gp_kwargs)
    gp.fit(continuous_dims=["a", "b"], categorical_dims="lot" if categorical else None, MAP_kwargs={"maxeval": 12})
    return gp


def test_condition_on_equals_a_fresh_gp_on_the_merged_data(monkeypatch):
    import gumbi_amd as gmb

    df = table(60)
    old, new = df.iloc[:45], df.iloc[45:]
    gp = fitted(monkeypatch, old)
    MAP = {k: np.array(v, copy=True) for k, v in gp.MAP.items()}
    theta = gp._theta_fitted.copy()
    gp.prepare_grid(resolution=5)
    assert gp.condition_on(new) is gp
    assert CountingEngine.appends == 1 and CountingEngine.truncates == 0
    assert gp.MAP.keys() == MAP.keys() and all(np.array_equal(gp.MAP[k], MAP[k]) for k in MAP)
    assert len(gp.model.y) == 60 and gp.model.X.shape == (60, 3) and len(gp.data.wide) == 60
    assert gp.data.stdzr is gp.stdzr and gp.grid_points is None and gp.predictions is None
    # the same rows through a fresh GP on the merged table with the SAME standardizer and the same hyper-parameters
    fresh = gmb.GP(gmb.DataSet(df.reset_index(drop=True), outputs=["y"], stdzr=gp.stdzr), outputs="y")
    fresh.specify_model(continuous_dims=["a", "b"], categorical_dims="lot")
    fresh.build_model()
    fresh.find_MAP(theta=theta)
    assert np.array_equal(fresh.model.X, gp.model.X) and np.array_equal(fresh.model.y, gp.model.y)
    pts = gp.parray(a=np.linspace(0.6, 3.9, 9), b=np.linspace(10.5, 19.5, 9))
    for level in ("k", "m", "z"):
        p = gp.append_categorical_points(pts, {"lot": level})
        got, want = gp.predict_points(p).z, fresh.predict_points(p).z
        assert rel(np.ravel(got.μ), np.ravel(want.μ)) <= 1e-10 and np.max(np.abs(np.ravel(got.σ2) - np.ravel(want.σ2))) <= 1e-10
    # a DataSet is taken as well, and the grid can be prepared again on the merged data
    more = table(8, seed=9)
    gp.condition_on(gmb.DataSet(more, outputs=["y"]))
    assert CountingEngine.appends == 2 and len(gp.model.y) == 68
    gp.prepare_grid(resolution=4)


def test_condition_on_maps_levels_to_the_fitted_models_codes(monkeypatch):
    df = table(40)
    gp = fitted(monkeypatch, df)
    code = gp.categorical_coords["lot"]
    assert code == {"k": 0, "m": 1, "z": 2}
    new = pd.DataFrame({"a": [1.5, 2.5], "b": [12.0, 18.0], "lot": ["z", "z"], "y": [3.1, 2.9]})  # alone, "z" would be code 0
    gp.condition_on(new)
    kind, X_new, y_new = CountingEngine.log[-1]
    assert kind == "append" and X_new.shape == (2, 3)
    assert np.array_equal(X_new[:, gp.dims.index("lot")], [2.0, 2.0])
    assert np.allclose(X_new[:, gp.dims.index("a")], gp.stdzr.stdz("a", np.array([1.5, 2.5])))
    assert np.allclose(y_new, gp.stdzr.stdz("y", np.array([3.1, 2.9])))
    with pytest.raises(ValueError, match="not seen"):
        gp.condition_on(pd.DataFrame({"a": [1.0], "b": [11.0], "lot": ["q"], "y": [3.0]}))
    with pytest.raises(ValueError, match="lacks the column"):
        gp.condition_on(pd.DataFrame({"a": [1.0], "lot": ["k"], "y": [3.0]}))
    assert CountingEngine.appends == 1 and len(gp.model.y) == 42


def test_condition_on_refit_starts_at_the_map(monkeypatch):
    df = table(50, seed=2)
    gp = fitted(monkeypatch, df.iloc[:40], categorical=False)
    MAP = gp.MAP
    seen = {}
    real = gp.find_MAP

    def spy(*args, **kwargs):
        seen.update(kwargs)
        return real(*args, maxeval=3, **kwargs)

    monkeypatch.setattr(gp, "find_MAP", spy)
    gp.condition_on(df.iloc[40:], refit=True)
    assert seen.get("start") is MAP
    assert CountingEngine.appends == 1 and len(gp.model.y) == 50


def test_condition_on_refuses_kronecker_and_unfitted_models(monkeypatch):
    import gumbi_amd as gmb
    from gumbi_amd.regression import icm
    from test_gpu_predict_grad import frontend_dataset

    use_engine(monkeypatch)
    gp = gmb.GP(frontend_dataset(20, ["y", "w"]), outputs=["y", "w"])
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 3})
    assert isinstance(gp.engine, icm.IcmEngine)
    with pytest.raises(NotImplementedError, match="Kronecker"):
        gp.condition_on(gp.data.wide.iloc[:2])
    with pytest.raises(NotImplementedError, match="Kronecker"):
        gp.propose_continuous(output="y", q=2, sequential=True, num_restarts=2, raw_samples=4)
    unfit = gmb.GP(frontend_dataset(20, ["y"]), outputs="y")
    unfit.specify_model(continuous_dims=["a", "b"])
    unfit.build_model()
    with pytest.raises(ValueError, match="must be fit"):
        unfit.condition_on(unfit.data.wide.iloc[:2])


def test_sequential_batch_proposes_distinct_points_and_restores_the_engine(monkeypatch):
    gp = fitted(monkeypatch, table(40, seed=4), categorical=False)
    X0, y0 = gp.model.X.copy(), gp.model.y.copy()
    pts = gp.parray(a=np.linspace(0.6, 3.9, 7), b=np.linspace(10.5, 19.5, 7))
    before = gp.predict_points(pts).z
    one = gp.propose_continuous(acquisition="EI", num_restarts=3, raw_samples=32, seed=1)
    value_one = gp.proposal_acquisition
    assert CountingEngine.appends == 0 and CountingEngine.truncates == 0 and isinstance(value_one, float)
    prop = gp.propose_continuous(acquisition="EI", num_restarts=3, raw_samples=32, seed=1, q=3, sequential=True)
    assert prop is gp.proposal and prop.shape == (3,) and set(prop.names) == {"a", "b"}
    # q - 1 fantasies (the last pick needs none) and ONE truncation back to the real observations
    assert CountingEngine.appends == 2 and CountingEngine.truncates == 1
    assert CountingEngine.log[-1] == ("truncate", 40)
    assert isinstance(gp.proposal_acquisition, list) and len(gp.proposal_acquisition) == 3
    Z = np.column_stack([prop.z[d + "_z"].values() for d in ("a", "b")])
    lo, hi = gp.optimization_bounds
    assert np.all(Z >= lo - 1e-12) and np.all(Z <= hi + 1e-12)
    for i in range(3):
        for j in range(i):
            assert not np.array_equal(Z[i], Z[j]), "a greedy batch proposes distinct points"
    # the first pick is the single-point search (same seed, same posterior)
    assert np.array_equal(Z[0], np.array([one.z[d + "_z"].values()[0] for d in ("a", "b")]))
    assert gp.proposal_acquisition[0] == value_one
    # every fantasy sat at its pick (the parray keeps natural units: the way back to z costs a rounding)
    for (kind, Xf, yf), z in zip(CountingEngine.log[:2], Z[:2]):
        assert kind == "append" and np.allclose(Xf[0], z, rtol=1e-12, atol=1e-12) and yf.shape == (1,)
    # nothing is left behind
    assert np.array_equal(gp.model.X, X0) and np.array_equal(gp.model.y, y0) and len(gp.engine.y) == 40
    after = gp.predict_points(pts).z
    assert np.array_equal(np.ravel(after.μ), np.ravel(before.μ)) and np.array_equal(np.ravel(after.σ2), np.ravel(before.σ2))


def test_sequential_batch_truncates_when_the_search_raises(monkeypatch):
    gp = fitted(monkeypatch, table(30, seed=6), categorical=False)
    y0 = gp.model.y.copy()
    real = gp._propose_one
    count = {"n": 0}

    def failing(*args, **kwargs):
        count["n"] += 1
        if count["n"] == 2:
            raise RuntimeError("search failed")
        return real(*args, **kwargs)

    monkeypatch.setattr(gp, "_propose_one", failing)
    with pytest.raises(RuntimeError, match="search failed"):
        gp.propose_continuous(num_restarts=2, raw_samples=16, seed=0, q=3, sequential=True)
    assert CountingEngine.appends == 1 and CountingEngine.truncates == 1
    assert len(gp.engine.y) == 30 and np.array_equal(gp.model.y, y0)


def test_batches_without_sequential_still_raise(monkeypatch):
    gp = fitted(monkeypatch, table(30, seed=6), categorical=False)
    with pytest.raises(NotImplementedError, match="q > 1"):
        gp.propose_continuous(q=2)
    with pytest.raises(NotImplementedError, match="fantasy"):
        gp.propose_continuous(q=2, sequential=True, fantasy="sample")
    with pytest.raises(ValueError):
        gp.propose_continuous(q=0, sequential=True)
    assert CountingEngine.appends == 0 and CountingEngine.truncates == 0


def test_condition_on_a_single_new_row(monkeypatch):
    """The Bayesian-optimisation step itself: ONE measurement of a single-output model (the base plumbing squeezes such a table to
    a 0-d y; the rows must reach the engine as (1, D) and (1,))."""
    import gumbi_amd as gmb

    df = table(41, seed=3)
    for categorical in (False, True):
        gp = fitted(monkeypatch, df.iloc[:40], categorical=categorical)
        theta = gp._theta_fitted.copy()
        gp.condition_on(df.iloc[40:])
        kind, X_new, y_new = CountingEngine.log[-1]
        assert kind == "append" and X_new.shape == (1, len(gp.dims)) and y_new.shape == (1,)
        assert CountingEngine.appends == 1 and gp.model.X.shape == (41, len(gp.dims)) and gp.model.y.shape == (41,)
        fresh = gmb.GP(gmb.DataSet(df.reset_index(drop=True), outputs=["y"], stdzr=gp.stdzr), outputs="y")
        fresh.specify_model(continuous_dims=["a", "b"], categorical_dims="lot" if categorical else None)
        fresh.build_model()
        fresh.find_MAP(theta=theta)
        assert np.array_equal(fresh.model.X, gp.model.X) and np.array_equal(fresh.model.y, gp.model.y)
        gp.condition_on(table(1, seed=8))  # ... and once more
        assert gp.model.y.shape == (42,)


def test_condition_on_a_single_row_of_two_outputs(monkeypatch):
    import gumbi_amd as gmb
    from test_gpu_predict_grad import frontend_dataset

    use_engine(monkeypatch)
    wide = frontend_dataset(21, ["y", "w"]).wide
    gp = gmb.GP(gmb.DataSet(wide.iloc[:20].reset_index(drop=True), outputs=["y", "w"]), outputs=["y", "w"], kronecker=False)
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 3})
    gp.condition_on(wide.iloc[20:])
    kind, X_new, y_new = CountingEngine.log[-1]
    assert X_new.shape == (2, 3) and y_new.shape == (2,) and sorted(X_new[:, 2]) == [0.0, 1.0]
    assert gp.model.y.shape == (42,)


def test_the_clean_up_never_replaces_the_searchs_error(monkeypatch):
    gp = fitted(monkeypatch, table(30, seed=6), categorical=False)
    real = gp._propose_one
    count = {"n": 0}

    def failing(*args, **kwargs):
        count["n"] += 1
        if count["n"] == 2:
            raise RuntimeError("search failed")
        return real(*args, **kwargs)

    def broken_truncate(n):
        raise MemoryError("truncate failed")

    monkeypatch.setattr(gp, "_propose_one", failing)
    monkeypatch.setattr(gp.engine, "truncate", broken_truncate)
    with pytest.warns(RuntimeWarning, match="restoring the engine"), pytest.raises(RuntimeError, match="search failed"):
        gp.propose_continuous(num_restarts=2, raw_samples=16, seed=0, q=3, sequential=True)


def test_a_fantasy_that_is_not_positive_definite_leaves_a_factored_engine(monkeypatch):
    gp = fitted(monkeypatch, table(30, seed=6), categorical=False)
    pts = gp.parray(a=np.linspace(0.6, 3.9, 5), b=np.linspace(10.5, 19.5, 5))
    before = gp.predict_points(pts).z
    real = gp.engine.append

    def append_not_pd(X, y):
        real(X, y)
        gp.engine._factored = False  # (what gmb_append leaves behind GMB_ENOTPD: the new data, no factor)
        raise np.linalg.LinAlgError("not positive definite")

    monkeypatch.setattr(gp.engine, "append", append_not_pd)
    with pytest.raises(np.linalg.LinAlgError):
        gp.propose_continuous(num_restarts=2, raw_samples=16, seed=0, q=2, sequential=True)
    assert len(gp.engine.y) == 30 and gp.engine.factor_is_current() and len(gp.model.y) == 30
    after = gp.predict_points(pts).z
    assert np.array_equal(np.ravel(after.μ), np.ravel(before.μ))
