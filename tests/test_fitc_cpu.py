"""The sparse (FITC) approximation on the CPU (``-m "not gpu"``: runs anywhere).

1. tests/fitc_reference.py against itself: the float64 restatement against the longdouble one, the hand-written reverse-mode
   gradient against Richardson-extrapolated central differences of the longdouble NLML, on every problem the GPU tests use
   (no entry of lambda clips on any of them: ``min_gap > 0``).
2. FITC with Z = X against the exact oracle.  Then Q = K + O(jitter) and Lambda = sigma^2 I to the same order, so FITC is the
   exact GP up to the two jitters (1e-6 on Kuu, and the exact model's own 1e-6 on Sigma, which FITC does not have).
   Measured on the case below (ExpQuad, N = m = 60 on a jittered 1-D lattice 0.6 lengthscales apart, sigma = 0.3):
   |NLML - exact| = 6.13e-5, max |mean - exact| = 7.60e-5, max |var - exact| = 7.04e-6; asserted at 10 x that.
3. ``m = 1``.
4. ``fitc_plan``: the tiles cover every column once, and the declared bytes hold no N^2 term (they are affine in N beyond one
   tile, and at N = 10^6, m = 1024 a thousandth of 8 N^2); tools/fitc_plan_check.cpp plain and under the address /
   undefined-behaviour sanitizers, as a stand-alone program.
5. The ABI pins: version 16, the new calls declared, bound, with the header's arities.
6. The front end over a numpy stand-in of the engine: refusals, ``GP.build_model(sparse=True)`` still raising, the k-means
   default's seed determinism and ``n_u`` bookkeeping, ``inducing_points=`` shapes, a fit, the refused queries.
"""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fitc_reference as F
from oracle import gp_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = {"gmb_fitc_set_inducing": 5, "gmb_fitc_evaluate": 5, "gmb_fitc_predict": 8, "gmb_debug_fitc_plan": 4}
NAMES = list(F.PROBLEMS) + ["seam"]


# ---- 1. the reference against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_float64_reference_against_longdouble(name):
    spec, theta, X, y, Z, Xs = F.problem(name)
    assert len(Z) == (F.SEAM if name == "seam" else F.PROBLEMS[name])[3]
    assert F.min_gap(spec, theta, X, y, Z) > 0.0  # no entry of lambda clips: the NLML is smooth around theta
    r = F.references(name)
    e_nlml = abs(r["h_nlml"] - r["nlml"]) / max(1.0, abs(r["nlml"]))
    e_mean = np.max(np.abs(r["h_mean"] - r["mean"])) / np.max(np.abs(r["mean"]))
    e_var = max(np.max(np.abs(r["h_var"] - r["var"])), np.max(np.abs(r["h_var_noise"] - r["var_noise"])))
    print(f"FITC-REF {name}: nlml {e_nlml:.2e} mean {e_mean:.2e} var {e_var:.2e}")
    # a backward-stable float64 computation on Kuu with cond ~ eta^2 / jitter = 1e6: cond x eps = 1e-10, the GPU tests' NLML floor
    assert e_nlml < 1e-10 and e_mean < 1e-10 and e_var < 1e-10
    assert np.all(r["var"] > 0) and np.allclose(r["var_noise"] - r["var"], theta[-1] ** 2, rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", NAMES)
def test_reverse_mode_gradient_against_extrapolated_differences(name):
    r = F.references(name)
    g, h = r["grad"], r["h_grad"]
    err = np.max(np.abs(h - g)) / np.max(np.abs(g))
    print(f"FITC-REF {name}: gradient {err:.2e} of max |grad| = {np.max(np.abs(g)):.3e}")
    # the differences: truncation O(h^4) after the Richardson step (h = 2e-3 theta: ~1e-11 relative) and the longdouble NLML's own
    # rounding over 2 h; the float64 adjoints: cond(Kuu) eps.  Both sit two decades below the GPU test's floor of 1e-8.
    assert err < 1e-9


# ---- 2. Z = X is the exact GP up to the two jitters ------------------------------------------------------------------------------
def test_inducing_points_on_the_data_give_the_exact_gp():
    rng = np.random.default_rng(5)
    N = 60
    X = (0.6 * np.arange(N) + 0.05 * rng.uniform(-1, 1, N))[:, None]  # at least half a lengthscale apart
    assert np.min(np.diff(X[:, 0])) >= 0.5
    y = np.sin(X[:, 0]) + 0.3 * rng.standard_normal(N)
    Xs = np.linspace(-1.0, 0.6 * N + 1.0, 97)[:, None]
    spec = O.make_spec(1, [0], kind="ExpQuad")
    theta = O.pack_theta(spec, [1.0], 1.0, 0.3)
    d_nlml = abs(F.nlml(spec, theta, X, y, X) - O.nlml(spec, theta, X, y, dist_mode="direct"))
    mu, var = F.predict(spec, theta, X, y, X, Xs, with_noise=True)
    mu_e, var_e = O.predict(spec, theta, X, y, Xs, with_noise=True, dist_mode="direct")
    d_mean, d_var = np.max(np.abs(mu - mu_e)), np.max(np.abs(var - var_e))
    print(f"FITC Z = X: nlml {d_nlml:.2e} mean {d_mean:.2e} var {d_var:.2e}")
    assert d_nlml <= 6.13e-4 and d_mean <= 7.60e-4 and d_var <= 7.04e-5  # 10 x the measured effect of the two jitters


# ---- 3. one inducing point ----------------------------------------------------------------------------------------------------------
def test_one_inducing_point_by_hand():
    spec, theta, X, y, Z, Xs = F.problem("exponential-m1")
    assert Z.shape == (1, 2)
    kzx = O.cov_full(spec, theta, Z, X, dist_mode="direct")[0]
    kuu = theta[2] ** 2 + spec["jitter"]  # eta^2 f(1e-6) differs from eta^2 by 5e-7: below the bar
    lam = theta[2] ** 2 - kzx**2 / kuu + theta[3] ** 2
    b = 1.0 + np.sum(kzx**2 / lam) / kuu
    c = (kzx / np.sqrt(kuu)) @ (y / lam) / np.sqrt(b)
    want = 0.5 * np.sum(np.log(lam)) + 0.5 * np.log(b) + 0.5 * (y @ (y / lam) - c * c) + 0.5 * len(y) * np.log(2 * np.pi)
    assert abs(F.nlml(spec, theta, X, y, Z) - want) < 1e-5 * abs(want)


# ---- 4. the plan --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, m", [(700, 130), (32768, 128), (32769, 1), (10**6, 1024)])
def test_plan_covers_every_column_once_and_holds_no_n_squared(N, m):
    from gumbi_amd import engine

    p = engine.fitc_plan(N, m)
    assert p == engine.Engine.fitc_plan(N, m)
    assert p["Np"] == -(-N // 128) * 128 and p["mp"] == -(-m // 128) * 128 and p["mr"] == -(-(m + 1) // 128) * 128
    assert len(p["tiles"]) == p["ntile"]
    covered = 0
    for first, count, tpad in p["tiles"]:
        assert first == covered and first % 128 == 0 and 1 <= count <= tpad < count + 128 and tpad % 128 == 0 and tpad <= p["tmax"]
        covered += count
    assert covered == N and p["tile_rows"] == F.TILE_ROWS_SMALL_M
    assert (N, m, p["ntile"]) in ((700, 130, 1), (32768, 128, 1), (32769, 1, 2), (10**6, 1024, 31))
    # the bytes: m x m and m x tile parts that do not depend on N beyond one tile, and a per-column part that is linear in it
    total = p["bytes_fixed"] + p["bytes_blocks"] + p["bytes_columns"]
    far, farther = engine.fitc_plan(N + 10 * p["tile_rows"], m), engine.fitc_plan(N + 20 * p["tile_rows"], m)
    assert far["bytes_fixed"] == p["bytes_fixed"] == farther["bytes_fixed"] and far["bytes_blocks"] == farther["bytes_blocks"]
    assert farther["bytes_columns"] - far["bytes_columns"] == far["bytes_columns"] - p["bytes_columns"] > 0
    assert p["bytes_columns"] <= 8 * 4 * p["Np"]  # lambda, alpha, d and the partial sums: a few doubles per column
    assert p["bytes_blocks"] <= 8 * 4.01 * p["mr"] * p["tmax"] + 8 * 17 * max(p["tmax"] * p["mp"], p["mp"] ** 2) / 128**2
    if N >= 32768:
        assert total < 8 * N * N / 4
    if N == 10**6:
        assert total < 8 * N * N / 1000


def test_plan_refusals():
    from gumbi_amd import engine

    for bad in ((0, 5), (10, 0), (10, 16385)):
        with pytest.raises(ValueError):
            engine.fitc_plan(*bad)


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_plan_program_builds_and_passes(tmp_path, flags):
    """tools/fitc_plan_check.cpp: the tiles and blocks ``gmb_fitc_evaluate`` computes before it launches anything, driven from a
    program of its own."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler on this machine"
    exe = tmp_path / "fitc_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", *flags, str(ROOT / "tools" / "fitc_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- 5. the ABI pins ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    for name, arity in NEW_CALLS.items():
        decl = re.search(rf"^(int|int64_t) {name}\(([^;]*)\);", header, re.M | re.S)
        assert decl, f"{name} is not declared in include/gumbi_hip.h"
        assert len(decl.group(2).split(",")) == arity
        assert name in engine.exported_symbols() and len(engine._SIGNATURES[name][1]) == arity
    ps = inspect.signature(engine.Engine.fitc_evaluate).parameters
    assert list(ps) == ["self", "theta", "grad"] and ps["grad"].default is True
    ps = inspect.signature(engine.Engine.fitc_predict).parameters
    assert list(ps) == ["self", "Xs", "with_noise"] and ps["with_noise"].default is True
    assert list(inspect.signature(engine.Engine.set_inducing).parameters) == ["self", "Z"]
    for hdr in ("fitc_plan.hpp",):
        text = (ROOT / "gumbi_amd" / "csrc" / hdr).read_text()
        assert "#include <hip" not in text and "hip_runtime" not in text and '#include "' not in text
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "fitc.hpp"' in source


# ---- 6. the front end without a device ----------------------------------------------------------------------------------------------
def table(n=120, seed=3, extra=None):
    import pandas as pd

    import gumbi_amd as gmb

    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 4.0, n), rng.uniform(10.0, 20.0, n)
    df = pd.DataFrame({"a": a, "b": b, "y": 3.0 + np.sin(a) * np.cos(0.3 * b) + 0.05 * rng.standard_normal(n)})
    outputs = ["y"]
    if extra == "category":
        df["lot"] = rng.choice(["p", "q"], n)
    if extra == "output":
        df["w"] = df["y"] * 0.5 + 0.05 * rng.standard_normal(n)
        outputs = ["y", "w"]
    return gmb.DataSet(df, outputs=outputs)


def test_sparse_gp_signatures_follow_gp():
    import gumbi_amd as gmb

    assert gmb.SparseGP is gmb.HipSparseGP and issubclass(gmb.SparseGP, gmb.GP)
    for method in ("fit", "build_model"):
        base = inspect.signature(getattr(gmb.GP, method)).parameters
        ours = inspect.signature(getattr(gmb.SparseGP, method)).parameters
        assert list(ours) == list(base) + ["inducing_points"]
        assert ours["sparse"].default is True and ours["n_u"].default == 100 and ours["inducing_points"].default is None


def test_unsupported_options_are_refused_before_anything_is_built(monkeypatch):
    import gumbi_amd as gmb

    F.use_fitc_oracle(monkeypatch)
    gp = gmb.SparseGP(table()).specify_model(continuous_dims=["a", "b"])
    with pytest.raises(ValueError, match="sparse=False"):
        gp.build_model(sparse=False)
    with pytest.raises(NotImplementedError, match="periodic"):
        gp.build_model(continuous_kernel="ExpQuad+Periodic", period=object())
    with pytest.raises(NotImplementedError, match="linear_dims"):
        gmb.SparseGP(table()).specify_model(continuous_dims=["a", "b"], linear_dims=["a"]).build_model()
    with pytest.raises(NotImplementedError, match="categorical"):
        gmb.SparseGP(table(extra="category")).specify_model(continuous_dims=["a", "b"], categorical_dims=["lot"]).build_model()
    with pytest.raises(NotImplementedError, match="additive"):
        gp_add = gmb.SparseGP(table()).specify_model(continuous_dims=["a", "b"])
        gp_add.additive = True
        gp_add.build_model()
    with pytest.raises(NotImplementedError, match="several outputs"):
        gmb.SparseGP(table(extra="output"), outputs=["y", "w"]).specify_model(continuous_dims=["a", "b"]).build_model()
    with pytest.raises(NotImplementedError):
        gmb.SparseGP(table(), distributed=True)
    assert gp.engine is None  # nothing was built by the refused calls
    # the exact class keeps its door shut
    with pytest.raises(NotImplementedError):
        gmb.GP(table()).specify_model(continuous_dims=["a", "b"]).build_model(sparse=True)


def test_kmeans_default_is_seeded_and_counts_its_centres(monkeypatch):
    import gumbi_amd as gmb
    from gumbi_amd.regression.sparse_gp import KMEANS_ROWS_PER_CENTRE, kmeans_inducing_points

    F.use_fitc_oracle(monkeypatch)
    gp = gmb.SparseGP(table(), seed=4).specify_model(continuous_dims=["a", "b"]).build_model(n_u=12)
    Z = gp.inducing_points.copy()
    assert Z.shape == (gp.n_u, 2) and 1 <= gp.n_u <= 12 and gp.sparse and gp.model_specs["sparse"] and gp.model_specs["n_u"] == 12
    assert np.array_equal(gp.engine.exact.Z, Z)
    X, _ = gp.get_shaped_data("mean")
    assert np.all(Z >= X.min(0)) and np.all(Z <= X.max(0))  # centres of clusters of rows
    again = gmb.SparseGP(table(), seed=4).specify_model(continuous_dims=["a", "b"]).build_model(n_u=12)
    other = gmb.SparseGP(table(), seed=5).specify_model(continuous_dims=["a", "b"]).build_model(n_u=12)
    assert np.array_equal(again.inducing_points, Z) and not np.array_equal(other.inducing_points[: len(Z)], Z[: other.n_u])
    # more centres than distinct rows: k-means returns what there is, and n_u says so
    dup = np.repeat(np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0]]), 5, axis=0)
    few = kmeans_inducing_points(dup, 8, seed=1)
    assert 1 <= len(few) <= 8 and few.shape[1] == 2
    # a long table is sub-sampled with the seed: the centres stay inside it and do not depend on rows that were not drawn
    rng = np.random.default_rng(0)
    long = rng.standard_normal((KMEANS_ROWS_PER_CENTRE * 3 + 500, 2))
    z1, z2 = kmeans_inducing_points(long, 3, seed=9), kmeans_inducing_points(long, 3, seed=9)
    assert np.array_equal(z1, z2) and len(z1) <= 3
    with pytest.raises(ValueError):
        gmb.SparseGP(table()).specify_model(continuous_dims=["a", "b"]).build_model(n_u=0)


def test_given_inducing_points(monkeypatch):
    import gumbi_amd as gmb

    F.use_fitc_oracle(monkeypatch)
    gp = gmb.SparseGP(table()).specify_model(continuous_dims=["a", "b"])
    pts = gp.parray(a=np.linspace(1.0, 3.5, 7), b=np.linspace(11.0, 19.0, 7))
    gp.build_model(inducing_points=pts, n_u=50)
    assert gp.n_u == 7 and gp.inducing_points.shape == (7, 2) and gp.model_specs["inducing_points"] is pts
    assert np.allclose(gp.inducing_points[:, 0], pts.z["a_z"].values()) and np.allclose(gp.inducing_points[:, 1], pts.z["b_z"].values())
    with pytest.raises(ValueError, match="one layer per model dimension"):
        gp.build_model(inducing_points=gp.parray(a=np.linspace(1.0, 3.5, 7)))
    with pytest.raises(ValueError, match="1-D"):
        gp.build_model(inducing_points=gp.parray(a=np.ones((2, 3)), b=np.ones((2, 3))))


def test_fit_predict_and_refused_queries(monkeypatch):
    import gumbi_amd as gmb

    F.use_fitc_oracle(monkeypatch)
    gp = gmb.SparseGP(table()).fit(continuous_dims=["a", "b"], n_u=15, MAP_kwargs={"maxeval": 30})
    assert gp.nlml_trace[-1] < gp.nlml_trace[0] and gp.MAP is not None and gp.engine.factor_is_current()
    gp.prepare_grid(resolution=6)
    pred = gp.predict_grid()
    assert pred.shape == gp.grid_parray.shape
    X, y = gp.get_shaped_data("mean")
    spec = gp.engine.exact.spec
    pa = gp._prepare_points_for_prediction(gp.grid_points, output=gp._parse_prediction_output(None))[0]
    mu, var = F.predict(spec, gp._theta_fitted, X, y, gp.inducing_points, pa)
    mu_g, var_g = gp.predict(pa)
    assert np.array_equal(mu_g, mu) and np.array_equal(var_g, var)
    for name in gmb.SparseGP.NOT_BUILT:
        with pytest.raises(NotImplementedError, match="is not built for the sparse approximation"):
            getattr(gp, name)()
