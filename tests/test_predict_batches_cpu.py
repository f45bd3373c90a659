"""Joint batch proposals on the CPU (``-m "not gpu"``: runs anywhere): the definition ``gmb_predict_batches`` implements
(tests/batch_reference.py) against an independent route, the Monte-Carlo batch acquisition of ``gumbi_amd/acquisition.py``
against finite differences and the analytic EI, the front end over a numpy stand-in engine, and the plan program.

1. Header, binding, the plan header and its check program (plain and under the address / undefined-behaviour sanitizers, as a
   stand-alone program).
2. ``dcov`` against Richardson central differences (h = 1e-4 and h / 2) of a joint covariance formed in ``np.longdouble``
   (``batch_reference.joint_cov_precise``): bar ``1e-9 max|dcov|``.  The differences' own error is truncation ~ h^4 f^(5) --
   for the kinked kinds (Matern-1/2, Exponential), whose fifth derivative grows like r^-4 between close points, 1.5e-8 at
   h = 1e-3 and, falling as h^4, 1.5e-12 here -- plus rounding of the float64 kernel entries, 1e-16 / h = 1e-12: two decades
   below the bar.  ``dcov[j, j]`` and ``dmean`` against ``var_grad_reference``'s ``dvar`` and ``dmean`` (the same formulas by
   other calls): 1e-12.
3. The acquisition: value and both adjoints against central differences; ``cholesky_adjoint`` likewise; q = 1 against the analytic
   EI within 4 standard errors of the same samples; finite with a gradient where the plain EI underflows.
4. ``propose_batch`` / ``batch_acquisition_with_grad`` over ``BatchOracleEngine``.
"""
import functools
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy.special import ndtr

import batch_reference as BR
import var_grad_reference as VR
from oracle import gp_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_predict_batches", "gmb_debug_batch_plan"]


# ---- 1. header, binding, plan -------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import distributed, engine
    from gumbi_amd.regression import icm

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^(int|int64_t) {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    ps = inspect.signature(engine.Engine.predict_batches).parameters
    assert list(ps) == ["self", "Xs", "q", "jitter", "grad"] and ps["jitter"].default == 1e-6 and ps["grad"].default is True
    for stand_in in (icm.IcmEngine, distributed.DistributedEngine):
        assert list(inspect.signature(stand_in.predict_batches).parameters) == list(ps)
        with pytest.raises(NotImplementedError, match="predict_batches"):
            stand_in.predict_batches(None, np.zeros((2, 1)), 2)
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "predict_batches.hpp"' in source
    plan = (ROOT / "gumbi_amd" / "csrc" / "batch_plan.hpp").read_text()
    assert "#include <hip" not in plan and "hip_runtime" not in plan and '#include "' not in plan
    kernels = (ROOT / "gumbi_amd" / "csrc" / "predict_batches.hpp").read_text()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in kernels and "atomic" not in kernels.split("#pragma once")[1]


def test_plan_follows_the_header():
    from gumbi_amd import engine

    plan = engine.batch_plan(10000, 10112, 10, 8)  # ten restarts of eight points behind 10^4 observations
    assert plan["bt"] == 32768 // 8 and plan["ntile"] == 1 and plan["mt"] == 128 and plan["unit"] == 64 and plan["slots"] == 1034
    first, nb, mc, mpad, chunk, nchunk = plan["tiles"][0]
    assert (first, nb, mc, mpad) == (0, 10, 80, 128) and chunk % 64 == 0 and (nchunk - 1) * chunk < 10000 <= nchunk * chunk
    assert nchunk * nb <= plan["slots"] and nchunk * nb >= 512
    seam = engine.batch_plan(300, 384, 6556, 5)  # tiles are cut at whole batches: 6553 x 5 = 32765 points, then three batches
    assert seam["bt"] == 6553 and [t[:4] for t in seam["tiles"]] == [(0, 6553, 32765, 32768), (6553, 3, 15, 128)]
    assert seam["tiles"][0][5] == 1 and seam["tiles"][0][4] >= 300
    for bad in ((300, 384, 10, 0), (300, 384, 10, 17), (300, 384, 0, 8), (300, 300, 10, 8), (0, 128, 10, 8)):
        with pytest.raises(ValueError):
            engine.batch_plan(*bad)


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_plan_program_builds_and_passes(tmp_path, flags):
    """tools/batch_plan_check.cpp: the tiles, chunks, lanes and slots ``gmb_predict_batches`` computes before it launches anything,
    driven from a program of its own."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler on this machine"
    exe = tmp_path / "batch_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", *flags, str(ROOT / "tools" / "batch_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- 2. the reference against an independent route ----------------------------------------------------------------------------------
def table(N, d, kind):  # tests/test_gpu_predict_grad.py's table and points (that module is marked gpu as a whole)
    X, y, ls = O.synthetic_table(N, d, seed=1000 * d + N)
    spec = O.make_spec(d, range(d), kind=kind, ard=True)
    return spec, O.pack_theta(spec, ls, 1.1, 0.25), X, y


def points(X, M, cont, seed=1):
    rng = np.random.default_rng(seed)
    Xs = X[rng.integers(0, len(X), M)].copy()
    Xs[:, cont] += 0.3 * rng.standard_normal((M, len(cont)))
    return Xs


@functools.lru_cache(maxsize=None)
def precise_cov(kind):
    spec, theta, X, y = table(300, 3, kind)
    return BR.joint_cov_precise(spec, theta, X, y)


@pytest.mark.parametrize("q", [2, 5, 16])
@pytest.mark.parametrize("kind", O.KINDS)
def test_dcov_matches_differences_of_the_joint_covariance(kind, q):
    spec, theta, X, y = table(300, 3, kind)
    P = points(X, q, [0, 1, 2])
    mean, cov, dmean, dcov = BR.batch_posterior(spec, theta, X, y, P, q)
    C = precise_cov(kind)
    fd = np.asarray(BR.fd_cov_grad(C, P, [0, 1, 2], h=1e-4), dtype=float)
    scale = float(np.max(np.abs(fd)))
    err = float(np.max(np.abs(dcov[0] - fd)))
    low = float(np.min(np.linalg.eigvalsh(cov[0])))
    print(f"{kind} q={q}: max |dcov - fd| = {err:.3e}, max |fd| = {scale:.3e}, ratio {err / scale:.2e}; smallest eigenvalue {low:.3e}")
    assert err <= 1e-9 * scale
    assert np.max(np.abs(cov[0] - np.asarray(C(P), dtype=float))) <= 1e-12
    assert low > 0.0  # the block is positive definite without any jitter
    r_mean, r_var, r_dmean, r_dvar = VR.mean_var_grad(spec, theta, X, y, P, with_noise=False)
    idx = np.arange(q)
    assert np.max(np.abs(dcov[0][idx, idx] - r_dvar)) <= 1e-12 * np.max(np.abs(r_dvar))
    assert np.max(np.abs(dmean[0] - r_dmean)) <= 1e-12 * np.max(np.abs(r_dmean))
    assert np.max(np.abs(mean[0] - r_mean)) <= 1e-12 and np.max(np.abs(cov[0][idx, idx] - r_var)) <= 1e-12


def test_coincident_points_and_fixed_columns():
    """Two coincident points of a batch: the Matern-1/2 derivative of their pair is 0 (the same sqrt(r^2 + 1e-12) as
    predict_grad.hpp); a composite model's categorical and output columns carry no derivative."""
    spec, theta, X, y = table(300, 3, "Matern12")
    P = points(X, 4, [0, 1, 2])
    P[1] = P[0]
    dcov = BR.batch_posterior(spec, theta, X, y, P, 4)[3][0]
    assert np.all(np.isfinite(dcov))
    rest = BR.batch_posterior(spec, theta, X, y, P[[0, 2, 3]], 3)[3][0]
    assert np.allclose(dcov[0, 2:], rest[0, 1:], rtol=0, atol=1e-12)  # the twin adds nothing to the other pairs
    gold = np.load(ROOT / "tests" / "golden" / "gp_goldens.npz")
    spec = O.make_spec(4, [0, 1], idx_lin=[1], coreg=[(2, 3)], out_col=3, n_out=2, hetero_noise=True)
    Xc, yc, th = gold["composite_N140/X"], gold["composite_N140/y"], gold["composite_N140/theta"]
    Pc = points(Xc, 6, [0, 1], seed=4)
    _, cov, dmean, dcov = BR.batch_posterior(spec, th, Xc, yc, Pc, 3)
    assert not np.any(dmean[:, :, 2:]) and not np.any(dcov[:, :, :, 2:]) and np.any(dcov[:, :, :, :2])
    _, _, _, r_dvar = VR.mean_var_grad(spec, th, Xc, yc, Pc, with_noise=False)
    idx = np.arange(3)
    assert np.allclose(dcov[:, idx, idx].reshape(6, 4), r_dvar, rtol=0, atol=1e-12 * np.max(np.abs(r_dvar)))


# ---- 3. the acquisition --------------------------------------------------------------------------------------------------------------
def random_batches(B, q, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, q, q + 2))
    cov = 0.05 * A @ np.swapaxes(A, 1, 2) / (q + 2) + 1e-3 * np.eye(q)
    return 0.3 * rng.standard_normal((B, q)), cov


def test_cholesky_adjoint_matches_differences():
    from gumbi_amd import acquisition as acq

    _, cov = random_batches(3, 4, 0)
    R = np.tril(np.random.default_rng(1).standard_normal((3, 4, 4)))
    f = lambda C: np.sum(R * np.linalg.cholesky(C), axis=(1, 2))  # noqa: E731
    bar = acq.cholesky_adjoint(np.linalg.cholesky(cov), R)
    assert np.array_equal(bar, np.swapaxes(bar, 1, 2))
    h = 1e-6
    for j in range(4):
        for l in range(j + 1):
            E = np.zeros((4, 4))
            E[j, l] = E[l, j] = 1.0
            fd = (f(cov + h * E) - f(cov - h * E)) / (2 * h)
            want = bar[:, j, l] * (1.0 if j == l else 2.0)
            assert np.max(np.abs(fd - want)) <= 1e-7 * max(1.0, np.max(np.abs(want))), (j, l)


@pytest.mark.parametrize("maximize", [True, False])
@pytest.mark.parametrize("q", [1, 3, 6])
def test_batch_ei_adjoints_match_differences(q, maximize):
    """Central differences with h = 1e-6: the smoothing's temperatures (1e-3) bound the third derivatives by ~1e6 per unit of the
    first, so the differences' truncation is ~h^2 1e6 / 6 = 2e-7 of the gradient and their rounding 1e-16 |value| / h; bar 1e-5."""
    from gumbi_amd import acquisition as acq

    mean, cov = random_batches(4, q, 10 + q)
    Z = acq.sobol_normals(64, q, seed=3)
    best = 0.2 if maximize else -0.2
    f = lambda m, C: acq.batch_expected_improvement(m, C, Z, best, maximize=maximize)[0]  # noqa: E731
    value, d_mean, d_cov = acq.batch_expected_improvement(mean, cov, Z, best, maximize=maximize)
    assert value.shape == (4,) and d_mean.shape == (4, q) and d_cov.shape == (4, q, q) and np.array_equal(d_cov, np.swapaxes(d_cov, 1, 2))
    via_get = acq.get("qEI", best=best)(mean, cov, Z, maximize)
    assert all(np.array_equal(a, b) for a, b in zip(via_get, (value, d_mean, d_cov)))
    h = 1e-6
    worst = 0.0
    for j in range(q):
        e = np.zeros(q)
        e[j] = h
        fd = (f(mean + e, cov) - f(mean - e, cov)) / (2 * h)
        worst = max(worst, float(np.max(np.abs(fd - d_mean[:, j]) / np.max(np.abs(d_mean), axis=1))))
        for l in range(j + 1):
            E = np.zeros((q, q))
            E[j, l] = E[l, j] = h
            fd = (f(mean, cov + E) - f(mean, cov - E)) / (2 * h)
            want = d_cov[:, j, l] * (1.0 if j == l else 2.0)
            worst = max(worst, float(np.max(np.abs(fd - want) / np.max(np.abs(d_cov), axis=(1, 2)))))
    print(f"q={q} maximize={maximize}: worst difference / largest adjoint = {worst:.2e}")
    assert worst <= 1e-5


@pytest.mark.parametrize("maximize", [True, False])
def test_one_point_batches_are_the_analytic_ei(maximize):
    from gumbi_amd import acquisition as acq

    sign = 1.0 if maximize else -1.0
    z = np.array([-2.0, -1.0, 0.0, 0.7, 2.5])
    s = np.array([0.3, 1.0, 0.5, 2.0, 0.1])
    best = 0.4
    mean = (best + sign * z * s)[:, None]
    Z = acq.sobol_normals(1024, 1, seed=11)
    value, d_mean, d_cov = acq.batch_expected_improvement(mean, (s * s)[:, None, None], Z, best, maximize=maximize)
    ei = s * (z * ndtr(z) + np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi))
    draws = np.maximum(sign * (mean + s[:, None] * Z[:, 0][None, :] - best), 0.0)
    se = np.std(draws, axis=1, ddof=1) / np.sqrt(Z.shape[0])
    print("exp(value) - EI in standard errors:", ((np.exp(value) - ei) / se).round(3))
    assert np.all(np.abs(np.exp(value) - ei) <= 4.0 * se)
    assert np.all(acq.TAU_RELU ** 2 < 1e-2 * se)  # the smoothing's bias, O(tau^2 p(0)), is far below that
    assert np.all(sign * d_mean[:, 0] > 0) and np.all(d_cov[:, 0, 0] > 0)  # EI grows with the mean (towards the goal) and the variance


def test_flat_regions_keep_a_value_and_a_gradient():
    from gumbi_amd import acquisition as acq

    mean = np.array([[-50.0, -60.0]])
    cov = np.array([[[1.0, 0.2], [0.2, 1.5]]])
    plain = acq.expected_improvement(np.array([-50.0]), np.array([1.0]), 0.0)[0]
    assert np.exp(plain[0]) == 0.0  # EI itself underflows here
    value, d_mean, d_cov = acq.batch_expected_improvement(mean, cov, acq.sobol_normals(256, 2, seed=0), 0.0)
    assert np.all(np.isfinite(value)) and np.all(np.isfinite(d_mean)) and np.all(np.isfinite(d_cov))
    assert d_mean[0, 0] > 0 and np.any(d_cov != 0.0)
    with pytest.raises(np.linalg.LinAlgError):
        acq.batch_expected_improvement(mean, np.array([[[1.0, 2.0], [2.0, 1.0]]]), acq.sobol_normals(8, 2, seed=0), 0.0)
    a, b = acq.sobol_normals(256, 3, seed=5), acq.sobol_normals(256, 3, seed=5)
    assert a.shape == (256, 3) and np.array_equal(a, b) and np.all(np.isfinite(a)) and abs(float(np.mean(a))) < 0.05


# ---- 4. the front end on a numpy stand-in engine ------------------------------------------------------------------------------------
def fitted_1d(monkeypatch, n=40):
    import pandas as pd

    import gumbi_amd as gmb

    eng = BR.use_batch_oracle(monkeypatch)
    rng = np.random.default_rng(5)
    a = np.sort(rng.uniform(0.0, 6.0, n))
    y = 2.0 + np.sin(a) + 0.02 * rng.standard_normal(n)  # maximiser of the surface inside [0, 6]: a = pi / 2
    ds = gmb.DataSet(pd.DataFrame({"a": a, "y": y}), outputs=["y"])
    gp = gmb.GP(ds, outputs="y")
    gp.fit(continuous_dims=["a"], MAP_kwargs={"maxeval": 30})
    monkeypatch.setattr(eng, "calls", [])
    return gp, a, eng


def test_propose_batch_on_the_sine_table(monkeypatch):
    gp, a, eng = fitted_1d(monkeypatch)
    prop = gp.propose_batch(2, num_restarts=3, raw_samples=32, mc_samples=64, seed=3)
    assert prop is gp.proposal and prop.names == ["a"]
    values = prop["a"].values().ravel()
    assert values.shape == (2,) and np.all(values >= a.min() - 1e-9) and np.all(values <= a.max() + 1e-9)
    lo, hi = gp.optimization_bounds
    assert lo.shape == hi.shape == (1,) and lo[0] < hi[0]
    assert gp.proposal_raw_acquisition.shape == (32,) and gp.proposal_acquisition >= np.max(gp.proposal_raw_acquisition)
    # one values-only call for the raw batches, ONE call at B = num_restarts per objective evaluation, one for the final choice
    assert eng.calls[0] == (32, 2, False) and eng.calls[-1] == (6, 2, False)
    assert set(eng.calls[1:-1]) == {(3, 2, True)} and len(eng.calls) - 2 == gp.proposal_result.nfev
    again = gp.propose_batch(2, num_restarts=3, raw_samples=32, mc_samples=64, seed=3)
    assert np.array_equal(again["a"].values().ravel(), values)  # seeded: the same proposal
    with pytest.raises(NotImplementedError, match="q > 1"):  # the single-point entry is unchanged
        gp.propose_continuous(q=2)
    with pytest.raises(ValueError):
        gp.propose_batch(17)
    with pytest.raises(ValueError, match="qEI"):
        gp.propose_batch(2, acquisition="EI")


def test_chained_gradient_matches_differences_of_the_acquisition(monkeypatch):
    gp, a, eng = fitted_1d(monkeypatch)
    Zb = np.random.default_rng(2).uniform(-1.0, 1.0, (2, 3, 1))
    value, grad = gp.batch_acquisition_with_grad(Zb, mc_samples=64, seed=1)
    assert value.shape == (2,) and grad.shape == (2, 3, 1) and eng.calls == [(2, 3, True)]
    h = 1e-6
    for b in range(2):
        for j in range(3):
            up, dn = Zb.copy(), Zb.copy()
            up[b, j, 0] += h
            dn[b, j, 0] -= h
            fd = (gp.batch_acquisition_with_grad(up, mc_samples=64, seed=1)[0][b] - gp.batch_acquisition_with_grad(dn, mc_samples=64, seed=1)[0][b]) / (2 * h)
            assert abs(fd - grad[b, j, 0]) <= 1e-4 * max(1.0, float(np.max(np.abs(grad[b])))), (b, j, fd, grad[b, j, 0])


def test_sparse_and_classification_models_refuse():
    import gumbi_amd as gmb

    for cls, words in ((gmb.SparseGP, "sparse approximation"), (gmb.GPC, "classification")):
        for name in ("propose_batch", "batch_acquisition_with_grad"):
            assert name in cls.NOT_BUILT
            with pytest.raises(NotImplementedError, match=words):
                getattr(cls, name)(None)
