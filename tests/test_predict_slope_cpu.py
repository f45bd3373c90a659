"""The posterior of the slope ``d f / d x*`` on the CPU (``-m "not gpu"``: runs anywhere): tests/slope_reference.py -- the closed
form the HIP kernels implement, in numpy -- against independent yardsticks, and the layers above the engine on an oracle-backed
stand-in.

1. Header, binding, the plan header and its check program.
2. The pairwise derivative: ``B @ alpha`` against ``grad_reference.mean_grad`` on every problem.  The two are the same N products
   per entry summed in two orders (and the products associated differently): each side is within ``gamma`` of the exact sum with
   ``gamma <= (log2 N + 3) eps sum_n |b_n alpha_n|`` for numpy's blocked summation, N <= 700: bar ``16 eps sum |b_n| |alpha_n|``.
   Measured: 0.4 - 1.4 eps sum |b| |alpha| over the six problems.
3. The prior term.  ``P`` against the literals ``eta^2 / ls^2``, ``5 eta^2 / 3 ls^2``, ``3 eta^2 / ls^2``: ``f'(0)`` keeps
   ``r = sqrt(0 + 1e-12) = 1e-6``, so for Matern-5/2 ``f'(0) = -(5/6)(1 + sqrt5 r) exp(-sqrt5 r) = -(5/6)(1 - (5/2) r^2 + O(r^3))``:
   2.5e-12 relative; for Matern-3/2 ``f'(0) = -(3/2) exp(-sqrt3 r)``: ``sqrt3 r = 1.74e-6`` relative -- both below 1e-5; ExpQuad
   has no offset (a few eps).  And for the periodic forms ``P`` against ``2 (k(x, x) - k(x + h e_d, x)) / h^2`` from PyMC's own
   formulas (``periodic_reference.direct_cov``) over halving h (0.02 .. 0.0025), at the rate the kernel allows: the gap falls as
   h^2 for ``Periodic`` (ExpQuad: even and smooth) and for ``Matern52+Periodic`` -- the r^3 terms of (1 + sqrt5 r + 5 r^2 / 3)
   exp(-sqrt5 r) cancel, sqrt5 (-5/6 + 5/2 - 5/3) = 0, the first odd term is r^5 -- and as h for ``Matern32+Periodic``, whose
   (1 + sqrt3 r) exp(-sqrt3 r) = 1 - 3 r^2 / 2 + sqrt3 r^3 - ... has the |r|^3 term at the origin: by 4 +- 0.5 and 2 +- 0.25 per
   halving.  Measured ratios: 3.998 - 4.000, 3.82 - 3.98, 1.95 - 2.00.
4. The whole, coarsely and independently: ``P - B Sigma^-1 B^T`` against Richardson central differences (h = 0.02 and 0.01) of the
   ORACLE's joint posterior covariance, ExpQuad, N = 60, d = 2, six points.  Measured gap 6.0e-8 of max(1, max P) = 2.47 (1.5e-7
   absolute; 9e-9 absolute at half the step: the differences' h^4 error, not the formula's); bar 6e-7, ten times the measured gap
   for the choice of step.
5. The Kronecker combination against the stacked model's reference: 1e-8 relative, the bar of the Kronecker engine against the
   oracle (tests/test_predict_grad_cpu.py).
6. The front end over ``SlopeOracleEngine``: layer names, the sigma_y / sigma_x scalings, grid shape, ``joint=True``, multi-output
   row selection, the refusals.
"""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import grad_reference as GR
import periodic_reference as PR
import slope_reference as SR
from oracle import gp_oracle as O
from oracle_engine import OracleEngine
from test_gpu_parity import rel
from test_gpu_predict_grad import frontend_dataset

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_predict_slope", "gmb_predict_slope_terms", "gmb_debug_slope_tile_rows"]
EPS = np.finfo(float).eps


# ---- 1. header, binding, plan -------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^(int|int64_t) {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    ps = inspect.signature(engine.Engine.predict_slope).parameters
    assert list(ps) == ["self", "Xs", "cov", "terms"] and ps["cov"].default is False and ps["terms"].default is None
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "predict_slope.hpp"' in source
    plan = (ROOT / "gumbi_amd" / "csrc" / "slope_plan.hpp").read_text()
    assert "#include <hip" not in plan and "hip_runtime" not in plan and '#include "' not in plan


def test_tile_rows_follow_the_plan():
    from gumbi_amd import engine

    assert engine.slope_tile_rows(768, 3) == 10880          # 32768 / 3 rounded down to 128
    assert engine.slope_tile_rows(768, 1) == 32768
    assert engine.slope_tile_rows(10112, 4) == 8192        # a prediction's tile is capped at 32768 rows
    assert engine.slope_tile_rows(1_000_000, 2) == 512     # 8 GiB / 8 MB per row = 1073 rows -> 1024 / 2
    assert engine.slope_tile_rows(20_000_000, 16) == 128    # never below one tile
    for bad in ((0, 3), (768, 0), (768, 25)):
        with pytest.raises(ValueError):
            engine.slope_tile_rows(*bad)


def test_plan_program_builds_and_passes(tmp_path):
    """tools/slope_plan_check.cpp: the column list, the M-tile and the stacked layout ``gmb_predict_slope`` computes before it
    launches anything, driven from a program of its own (its head has the sanitizer build, run by hand)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "slope_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "slope_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- 2. the pairwise derivative ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SR.PROBLEMS)
def test_pairwise_derivative_sums_to_the_mean_gradient(name):
    spec, theta, X, y, periodic, periods = SR.problem(name)
    Xs = SR.points(name, 129)
    mdl = SR.Model(spec, theta, X, periodic, periods)
    alpha = GR._alpha(mdl.spec, mdl.theta, mdl.X, y)
    B, _ = mdl.B_P(Xs)
    G = GR.mean_grad(spec, theta, X, y, Xs, periodic=periodic, periods=periods)
    size = np.abs(B) @ np.abs(alpha)                          # (M, D): sum_n |b_n| |alpha_n|
    cols = SR.cont_columns(spec)
    gap = float(np.max(np.abs(B @ alpha - G)[:, cols] / size[:, cols]))
    print(f"SLOPE-CPU {name}: max |B alpha - mean_grad| / sum |b| |alpha| = {gap / EPS:.2f} eps")
    assert gap <= 16 * EPS
    flat = [c for c in range(X.shape[1]) if c not in cols]
    assert not np.any(B[:, flat, :])
    dmean = SR.reference(name, 129)[0]                        # ... and the solved form V v the engine uses
    assert rel(dmean, G) <= 1e-10


def test_a_selection_sums_its_terms():
    spec, theta, X, y, _, _ = SR.problem("three_term")
    Xs = SR.points("three_term", 129)
    parts = [SR.posterior(spec, theta, X, y, Xs, terms=1 << t) for t in range(3)]
    total = SR.reference("three_term", 129)
    assert rel(parts[0][0] + parts[1][0] + parts[2][0], total[0]) <= 1e-12
    both = SR.posterior(spec, theta, X, y, Xs, terms=0b101)
    assert rel(parts[0][0] + parts[2][0], both[0]) <= 1e-12
    assert not np.allclose(parts[0][2] + parts[2][2], both[2])  # covariances of a selection do NOT add: the cross term <V_t, V_u>


# ---- 3. the prior term ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,factor,offset", [("ExpQuad", 1.0, 0.0), ("Matern52", 5.0 / 3.0, 2.5e-12), ("Matern32", 3.0, np.sqrt(3.0) * 1e-6)])
def test_prior_curvature_equals_the_literals(kind, factor, offset):
    ls, eta = np.array([0.7, 1.3, 2.1]), 1.4
    spec = O.make_spec(3, range(3), kind=kind)
    theta = O.pack_theta(spec, ls, eta, 0.3)
    Xs = np.random.default_rng(0).standard_normal((5, 3))
    P = SR.prior_curvature(spec, theta, Xs, Xs)
    want = factor * eta**2 / ls**2
    idx = np.arange(3)
    gap = float(np.max(np.abs(P[:, idx, idx] / want - 1.0)))
    print(f"SLOPE-CPU {kind}: P against {factor:.4g} eta^2 / ls^2: {gap:.3e} relative (the 1e-12 offset: {offset:.3e})")
    assert gap <= offset * 1.001 + 4 * EPS and gap < 1e-5
    off_diag = P.copy()
    off_diag[:, idx, idx] = 0.0
    assert not np.any(off_diag)


@pytest.mark.parametrize("name,kind,rate", [("periodic", "ExpQuad", 2), ("matern52_periodic", "Matern52", 2), ("matern52_periodic", "Matern32", 1)])
def test_periodic_prior_curvature_is_the_limit_of_pymcs_kernel(name, kind, rate):
    spec, theta, X, _, mode, periods = SR.problem(name)
    spec = dict(spec, kind=O.KINDS[kind])
    p = O.unpack_theta(spec, theta)
    x = np.array([[0.37, -1.1]])
    P = SR.prior_curvature(spec, theta, X, x, None, mode, periods)[0]
    assert P[0, 1] == 0.0 and P[1, 0] == 0.0
    for d in range(2):
        gaps = []
        for h in (0.02, 0.01, 0.005, 0.0025):
            xh = x.copy()
            xh[0, d] += h
            k = PR.direct_cov(kind, mode, p["ls"], p["eta"], periods, x, np.vstack([x, xh]))[0]
            gaps.append(abs(2.0 * (k[0] - k[1]) / h**2 - P[d, d]) / P[d, d])
        ratios = [gaps[i] / gaps[i + 1] for i in range(3)]
        print(f"SLOPE-CPU {name} {kind} d = {d}: gaps {np.array2string(np.array(gaps), precision=3)}, ratios {np.array2string(np.array(ratios), precision=3)}")
        assert all(abs(r - 2.0**rate) <= 2.0**rate / 8 for r in ratios) and gaps[-1] < 0.05


# ---- 4. the whole against differences of the oracle's joint covariance ---------------------------------------------------------------
def test_covariance_matches_differences_of_the_joint_posterior():
    name = "expquad_small"
    spec, theta, X, y, _, _ = SR.problem(name)
    Xs = SR.points(name, 6)
    _, _, dcov = SR.posterior(spec, theta, X, y, Xs)
    fd = SR.fd_slope_cov(spec, theta, X, y, Xs, [0, 1], h=0.02)
    scale = max(1.0, float(np.max(SR.prior_curvature(spec, theta, X, Xs))))
    gap = float(np.max(np.abs(fd - dcov))) / scale
    print(f"SLOPE-CPU P - B Sigma^-1 B^T against Richardson differences of the joint covariance: {gap:.3e} of max(1, max P) = {scale:.3g}")
    assert gap <= 6e-7
    assert np.all(np.linalg.eigvalsh(dcov) > 0.0)


# ---- 5, 6. the layers above the engine ----------------------------------------------------------------------------------------------
class SlopeOracleEngine(OracleEngine):
    """``OracleEngine`` + ``predict_slope`` (and ``predict_grad``) answered from the reference (test infrastructure only)."""

    calls = 0

    def predict_slope(self, Xs, cov=False, terms=None):
        type(self).calls += 1
        if not self._factored:
            raise ValueError("no valid factorisation")
        dmean, dvar, dcov = SR.posterior(self.spec, self.theta, self.X, self.y, np.asarray(Xs, float), terms)
        return (dmean, dvar, dcov) if cov else (dmean, dvar)

    def predict_grad(self, Xs, terms=None):
        return self.predict_slope(Xs, terms=terms)[0]


def use_slope_oracle(monkeypatch):
    from gumbi_amd.regression import hip_gp, icm

    monkeypatch.setattr(hip_gp, "Engine", SlopeOracleEngine)
    monkeypatch.setattr(icm, "Engine", SlopeOracleEngine)


def fitted(monkeypatch, outputs, kronecker="auto", n=40, kernel="ExpQuad"):
    import gumbi_amd as gmb

    use_slope_oracle(monkeypatch)
    gp = gmb.GP(frontend_dataset(n, outputs), outputs=outputs if len(outputs) > 1 else outputs[0], kronecker=kronecker)
    gp.fit(continuous_dims=["a", "b"], continuous_kernel=kernel, MAP_kwargs={"maxeval": 10})
    return gp


def reference_at(gp, pa):
    return SR.posterior(gp.model.spec.as_dict(), gp._theta_fitted, gp.model.X, gp.model.y, pa)


def test_point_slopes_layers_and_scaling(monkeypatch):
    from gumbi_amd.arrays import UncertainArray

    gp = fitted(monkeypatch, ["y"])
    pts = gp.parray(a=np.linspace(0.8, 3.5, 9), b=np.linspace(11.0, 19.0, 9))
    slope = gp.predict_points_slope(pts)
    assert list(slope) == ["δ[y]/δ[a]", "δ[y]/δ[b]"] == gp.predict_points_grad(pts, norm=False).names
    assert gp.slope_cov is None
    pa, _, _ = gp._prepare_points_for_prediction(pts, output=["y"])
    dmean, dvar, dcov = reference_at(gp, pa)
    assert all(np.array_equal(a, b) for a, b in zip(gp.predict_slope(pa, cov=True), (dmean, dvar, dcov)))
    sy = np.sqrt(gp.stdzr["y"]["σ2"])
    sx = {x: np.sqrt(gp.stdzr[x]["σ2"]) for x in ("a", "b")}
    grad = gp.predict_points_grad(pts, norm=False)
    for x in ("a", "b"):
        ua = slope[f"δ[y]/δ[{x}]"]
        col = gp.dims.index(x)
        assert isinstance(ua, UncertainArray) and ua.shape == (9,) and ua.name == f"δ[y]/δ[{x}]"
        assert np.allclose(ua.μ, dmean[:, col] * sy / sx[x], rtol=1e-14, atol=0)
        assert np.allclose(ua.σ2, dvar[:, col] * (sy / sx[x]) ** 2, rtol=1e-14, atol=0) and np.all(ua.σ2 > 0)
        assert np.allclose(ua.μ, grad[f"δ[y]/δ[{x}]"].values(), rtol=1e-10, atol=0)
    joint = gp.predict_points_slope(pts, joint=True)
    cov = gp.slope_cov["y"]
    assert list(gp.slope_cov) == ["y"] and cov.shape == (9, 2, 2)
    cols = [gp.dims.index(x) for x in ("a", "b")]
    want = dcov[:, cols][:, :, cols] * sy**2 / np.outer([sx["a"], sx["b"]], [sx["a"], sx["b"]])
    assert np.allclose(cov, want, rtol=1e-14, atol=0)
    for k, x in enumerate(("a", "b")):  # its diagonal is the layers' variance, in the same units
        assert np.allclose(cov[:, k, k], joint[f"δ[y]/δ[{x}]"].σ2, rtol=1e-14, atol=0)
    assert "|∇|" in gp.predict_points_slope.__doc__ and "not Gaussian" in gp.predict_points_slope.__doc__


def test_grid_slopes_have_the_grid_shape(monkeypatch):
    gp = fitted(monkeypatch, ["y"])
    with pytest.raises(ValueError, match="prepare_grid"):
        gp.predict_grid_slope()
    gp.prepare_grid(resolution=6)
    slope = gp.predict_grid_slope(joint=True)
    assert list(slope) == ["δ[y]/δ[a]", "δ[y]/δ[b]"] and all(ua.shape == (6, 6) for ua in slope.values())
    grid_cov = gp.slope_cov["y"]
    assert grid_cov.shape == (6, 6, 2, 2)
    flat = gp.predict_points_slope(gp.grid_points, joint=True)
    assert np.array_equal(grid_cov.reshape(36, 2, 2), gp.slope_cov["y"])
    assert np.array_equal(slope["δ[y]/δ[a]"].μ.ravel(), flat["δ[y]/δ[a]"].μ)
    assert np.array_equal(slope["δ[y]/δ[b]"].σ2.ravel(), flat["δ[y]/δ[b]"].σ2)
    gp.predict_grid_slope()
    assert gp.slope_cov is None


def test_two_outputs_on_stacked_points(monkeypatch):
    gp = fitted(monkeypatch, ["y", "w"], kronecker=False)
    pts = gp.parray(a=np.linspace(0.8, 3.5, 7), b=np.linspace(11.0, 19.0, 7))
    slope = gp.predict_points_slope(pts, joint=True)
    assert list(slope) == ["δ[y]/δ[a]", "δ[y]/δ[b]", "δ[w]/δ[a]", "δ[w]/δ[b]"] and all(ua.shape == (7,) for ua in slope.values())
    pa, _, coords = gp._prepare_points_for_prediction(pts, output=["y", "w"])
    dmean, dvar, dcov = reference_at(gp, pa)
    out_col = gp.dims.index(gp.out_col)
    cols = [gp.dims.index(x) for x in ("a", "b")]
    sx = np.array([np.sqrt(gp.stdzr[x]["σ2"]) for x in ("a", "b")])
    for name, coord in zip(["y", "w"], coords):
        rows = pa[:, out_col] == coord
        sy = np.sqrt(gp.stdzr[name]["σ2"])
        ua = slope[f"δ[{name}]/δ[b]"]
        assert np.allclose(ua.μ, dmean[rows][:, cols[1]] * sy / sx[1], rtol=1e-14, atol=0)
        assert np.allclose(ua.σ2, dvar[rows][:, cols[1]] * (sy / sx[1]) ** 2, rtol=1e-14, atol=0)
        assert np.allclose(gp.slope_cov[name], dcov[rows][:, cols][:, :, cols] * sy**2 / np.outer(sx, sx), rtol=1e-14, atol=0)
    one = gp.predict_points_slope(pts, output="w")
    assert list(one) == ["δ[w]/δ[a]", "δ[w]/δ[b]"] and np.array_equal(one["δ[w]/δ[a]"].μ, slope["δ[w]/δ[a]"].μ)


def test_kronecker_combination_equals_the_stacked_model(monkeypatch):
    from gumbi_amd.regression import icm

    gk = fitted(monkeypatch, ["y", "w"], kronecker="auto")
    assert isinstance(gk.engine, icm.IcmEngine)
    pts = gk.parray(a=np.linspace(0.8, 3.5, 11), b=np.linspace(11.0, 19.0, 11))
    pa, _, _ = gk._prepare_points_for_prediction(pts, output=["y", "w"])
    dmean, dvar, dcov = gk.predict_slope(pa, cov=True)
    ref = reference_at(gk, pa)
    scale = max(1.0, float(np.max(np.abs(ref[2]))))
    gaps = rel(dmean, ref[0]), float(np.max(np.abs(dvar - ref[1]))) / scale, float(np.max(np.abs(dcov - ref[2]))) / scale
    print(f"SLOPE-CPU Kronecker against stacked: mean {gaps[0]:.2e}, var {gaps[1]:.2e}, cov {gaps[2]:.2e}")
    assert max(gaps) < 1e-8
    assert not np.any(dmean[:, -1]) and not np.any(dvar[:, -1]) and not np.any(dcov[:, -1, :]) and not np.any(dcov[:, :, -1])
    assert np.array_equal(gk.predict_slope(pa)[1], dvar)
    # the rule itself, restated by the reference
    st = gk.engine._decompose()
    task = pa[:, -1].astype(np.int64)
    per = [gk.engine._load(p, st).predict_slope(np.ascontiguousarray(pa[:, :-1]), cov=True) for p in range(gk.engine.P)]
    m2, c2 = SR.kron_combine(st["Q"], st["Dd"], [r[0] for r in per], [r[2] for r in per], task)
    assert np.allclose(m2, dmean[:, :-1], rtol=1e-13, atol=0) and np.allclose(c2, dcov[:, :-1, :-1], rtol=1e-13, atol=1e-300)


def test_unfitted_models_and_kernels_without_a_derivative_raise(monkeypatch):
    import gumbi_amd as gmb

    use_slope_oracle(monkeypatch)
    gp = gmb.GP(frontend_dataset(30, ["y"]), outputs="y")
    gp.specify_model(continuous_dims=["a", "b"])
    gp.build_model()
    with pytest.raises(ValueError, match="must be fit"):
        gp.predict_slope(np.zeros((3, 2)))
    with pytest.raises(ValueError, match="must be fit"):
        gp.predict_points_slope(gp.parray(a=np.array([1.0]), b=np.array([12.0])))
    with pytest.raises(NotImplementedError):
        gp.predict_slope(np.zeros((3, 2)), additive_level="Name")
    for kernel in ("Matern12", "Exponential"):
        gk = fitted(monkeypatch, ["y"], kernel=kernel)
        before = SlopeOracleEngine.calls
        with pytest.raises(ValueError, match=kernel):
            gk.predict_points_slope(gk.parray(a=np.array([1.0]), b=np.array([12.0])))
        assert SlopeOracleEngine.calls == before, "the engine was called for a kernel without a derivative"
    assert fitted(monkeypatch, ["y"], kernel="Matern32").predict_slope(np.zeros((3, 2)))[0].shape == (3, 2)


def test_distributed_engines_refuse():
    from gumbi_amd.distributed import DistributedEngine

    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.predict_slope(object(), np.zeros((1, 1)))
