"""GP classification by the Laplace approximation, the parts that need no device: the numpy restatements (tests/laplace_reference.py)
against each other and against central differences, the caps of the Newton iteration, the averaged probability, the plan
(csrc/laplace_plan.hpp: its export and its sanitized check program), the ABI pins and the front end's refusals."""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import laplace_reference as L

ROOT = Path(__file__).resolve().parent.parent
NAMES = list(L.PROBLEMS)
NEW_CALLS = {"gmb_laplace_evaluate": 5, "gmb_laplace_predict": 7, "gmb_laplace_info": 2, "gmb_laplace_copy_mode": 3,
             "gmb_laplace_set_options": 3, "gmb_debug_laplace_plan": 3, "gmb_debug_laplace_symv": 3}


# ---- 1. the two restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_host_restatement_against_the_longdouble_reference(name):
    """float64 on LAPACK loses to rounding what cond(B) allows -- nothing near the floors the engine is held to"""
    r = L.references(name)
    rel = lambda k: np.max(np.abs(r["h_" + k] - r[k])) / np.max(np.abs(r[k]))  # noqa: E731
    assert abs(r["h_nlq"] - r["nlq"]) <= 1e-12 * max(1.0, abs(r["nlq"]))
    assert rel("grad") <= 1e-10 and rel("f") <= 1e-11 and rel("a") <= 1e-9 and rel("mean") <= 1e-10
    assert np.max(np.abs(r["h_var"] - r["var"])) <= 1e-8
    assert np.all(r["var"] > -1e-9) and np.all(np.isfinite(r["grad"]))


@pytest.mark.parametrize("name", NAMES)
def test_newton_iteration_stays_far_from_its_caps(name):
    """40 iterations and 20 halvings are conditions, not measurements: with the engine's stop rule every problem needs at most 14
    iterations and at most one halving, so a cap cannot be what a failure hides behind"""
    r = L.references(name)
    assert 1 <= r["h_iterations"] <= 14 and r["h_halvings"] <= 1
    assert r["iterations"] <= 20 and r["halvings"] <= 1  # (the reference goes on to a step of 1e-17)


def test_the_hard_problems_are_hard():
    sep, sat = L.references("separated"), L.references("saturated")
    assert np.max(np.abs(sep["f"])) > 20 and sep["W"].min() < 1e-10
    assert np.max(np.abs(sat["f"])) > 50 and sat["W"].min() < 1e-25


def test_a_cap_is_an_error():
    spec, theta, X, y, _ = L.problem("separated")
    with pytest.raises(L.NoConvergence):
        L.host(spec, theta, X, y, max_iter=2)


@pytest.mark.parametrize("name", ["N100", "eq-shared", "m12-lin", "coreg", "separated"])
def test_gradient_against_central_differences_of_the_objective(name):
    """step 1e-5, agreement 1e-7 of the largest entry; this is what decides the sign of s2 (the opposite of the printed line 10 of
    Algorithm 5.1: W = -dd log p): the printed sign is off by order 1"""
    spec, theta, X, y, _ = L.problem(name)
    g = L.references(name)["grad"]
    fd = np.zeros_like(g)
    for j in range(theta.size):
        if theta[j] == 0.0:  # sigma = 0: d sigma^2 / d sigma = 0, and the objective is even in sigma
            continue
        tp, tm = theta.copy(), theta.copy()
        tp[j] += 1e-5
        tm[j] -= 1e-5
        fd[j] = float((L.objective(spec, tp, X, y) - L.objective(spec, tm, X, y)) / np.longdouble(2e-5))
    print(name, np.max(np.abs(fd - g)) / np.max(np.abs(g)))
    assert np.max(np.abs(fd - g)) <= 1e-7 * np.max(np.abs(g))
    assert g[np.flatnonzero(theta == 0.0)[0]] == 0.0


# ---- 2. the averaged probability ------------------------------------------------------------------------------------------------------
def test_averaged_sigmoid_against_adaptive_quadrature():
    from scipy.integrate import quad
    from scipy.special import expit

    from gumbi_amd.regression.gpc import averaged_sigmoid

    def ref(mu, v):
        if v == 0:
            return expit(mu)
        s = np.sqrt(v)
        f = lambda z: expit(mu + s * z) * np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)  # noqa: E731
        brk = sorted({-12.0, 12.0, *(min(12.0, max(-12.0, (k - mu) / s)) for k in (-40, -10, -3, 0, 3, 10, 40))})
        return sum(quad(f, a, b, epsabs=1e-15, epsrel=1e-14, limit=200)[0] for a, b in zip(brk[:-1], brk[1:]))

    mus = np.array([-30, -10, -3, -0.5, 0, 0.7, 4, 12, 30], dtype=float)
    vs = np.array([0, 0.01, 0.5, 1, 4, 25, 100], dtype=float)
    MU, V = np.meshgrid(mus, vs, indexing="ij")
    got = averaged_sigmoid(MU, V)
    want = np.array([[ref(m, v) for v in vs] for m in mus])
    assert got.shape == MU.shape and np.max(np.abs(got - want)) <= 1e-10
    assert np.all((got > 0) & (got < 1))
    # one small variance beside a large one in the same call, and an empty call
    assert abs(averaged_sigmoid([0.3, 0.3], [0.04, 100.0])[0] - ref(0.3, 0.04)) <= 1e-10
    assert averaged_sigmoid(np.zeros(0), np.zeros(0)).shape == (0,)


# ---- 3. the plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 100, 128, 129, 300, 1000])
def test_plan_export(N):
    from gumbi_amd import build, engine

    build.build_library()
    p = engine.laplace_plan(N)
    nt = -(-N // 128)
    assert p["Np"] == nt * 128 and p["Nr"] == -(-(N + 1) // 128) * 128 and p["nt"] == nt and p["slots"] == nt * (nt + 1) // 2
    assert p["slot_doubles"] == 256 and p["lik_blocks"] == -(-p["Np"] // 256)
    # the state's own buffers: Sigma, 16 vectors, the slots, the partial sets and their fold
    assert p["bytes_state"] == 8 * (p["Nr"] * p["Np"] + 16 * p["Np"] + 256 * p["slots"] + p["lik_sums"] * (p["lik_blocks"] + 1))
    seen = set()
    for R, terms in enumerate(p["row_terms"]):
        assert len(terms) == nt + 1
        for q, off in enumerate(terms):
            tile = (R, q) if q <= R else (q - 1, R)
            assert off == 256 * (tile[0] * (tile[0] + 1) // 2 + tile[1]) + (0 if q <= R else 128)
            seen.add(off)
    assert len(seen) == 2 * p["slots"]  # every half of every slot, once


def test_plan_refusals():
    from gumbi_amd import engine

    for bad in (0, -3, 2**22 + 1):
        with pytest.raises(ValueError):
            engine.laplace_plan(bad)


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_plan_program_builds_and_passes(tmp_path, flags):
    """tools/laplace_plan_check.cpp: the slots and the order of the sums, driven from a program of its own"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler on this machine"
    exe = tmp_path / "laplace_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", *flags, str(ROOT / "tools" / "laplace_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- 4. the ABI pins --------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name, arity in NEW_CALLS.items():
        decl = re.search(rf"^(int|int64_t) {name}\(([^;]*)\);", header, re.M | re.S)
        assert decl, f"{name} is not declared in include/gumbi_hip.h"
        assert len(decl.group(2).split(",")) == arity
        assert name in engine.exported_symbols() and len(engine._SIGNATURES[name][1]) == arity
    assert re.search(r"GMB_ENOCONV = -6\b", header) and engine.GMB_ENOCONV == -6
    body = re.search(r"typedef struct gmb_laplace_stats \{(.*?)\} gmb_laplace_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(?:double|int32_t)\s+([a-z_0-9]+)\s*;", body) == [n for n, _ in engine.LaplaceStats._fields_]
    assert engine.C.sizeof(engine.LaplaceStats) == 24
    ps = inspect.signature(engine.Engine.laplace_evaluate).parameters
    assert list(ps) == ["self", "theta", "grad"] and ps["grad"].default is True
    assert list(inspect.signature(engine.Engine.laplace_predict).parameters) == ["self", "Xs"]
    assert issubclass(engine.LaplaceConvergenceError, RuntimeError) and not issubclass(engine.LaplaceConvergenceError, ValueError)
    text = (ROOT / "gumbi_amd" / "csrc" / "laplace_plan.hpp").read_text()
    assert "#include <hip" not in text and "hip_runtime" not in text and '#include "' not in text


# ---- 5. the front end without a device --------------------------------------------------------------------------------------------------
def _dataset(values, extra=None):
    import pandas as pd

    import gumbi_amd as gmb

    rng = np.random.default_rng(0)
    cols = {"x0": rng.standard_normal(len(values)), "x1": rng.standard_normal(len(values)), "y": np.asarray(values, dtype=float)}
    cols.update(extra or {})
    return gmb.DataSet(pd.DataFrame(cols), outputs=[c for c in cols if c.startswith("y")])


def test_front_end_checks_labels_and_scope_before_any_device_is_touched():
    import gumbi_amd as gmb

    assert gmb.GPC is gmb.HipGPC and issubclass(gmb.GPC, gmb.HipGP)
    good = [0.0, 1.0] * 20
    for bad in ([0.0, 0.5] * 20, [0.0, 2.0] * 20, [-1.0, 1.0] * 20):
        with pytest.raises(ValueError, match="labels 0 and 1"):
            gmb.GPC(_dataset(bad), outputs=["y"])
    gp = gmb.GPC(_dataset(good), outputs=["y"])
    # the labels are not standardized: what the engine will get is what the table holds
    gp.specify_model(continuous_dims=["x0", "x1"])
    X, y = gp.get_shaped_data("mean")
    assert y.tolist() == good and X.shape == (40, 2) and abs(X.mean()) < 1.0
    assert gp.stdzr["y"] == {"μ": 0.0, "σ2": 1.0} and gp.data.stdzr["y"]["μ"] == 0.5  # (the data set's own standardizer is untouched)
    with pytest.raises(NotImplementedError, match="distributed"):
        gmb.GPC(_dataset(good), outputs=["y"], distributed=True)
    with pytest.raises(NotImplementedError, match="Kronecker"):
        gmb.GPC(_dataset(good), outputs=["y"], kronecker=True)
    with pytest.raises(NotImplementedError, match="one output"):
        gmb.GPC(_dataset(good, extra={"y2": good}), outputs=["y", "y2"])
    with pytest.raises(NotImplementedError, match="sparse"):
        gp.build_model(sparse=True)
    with pytest.raises(NotImplementedError, match="periodic"):
        gp.build_model(continuous_kernel="Matern52+Periodic")
    cat = _dataset(good, extra={"c": ["a", "b"] * 20})
    with pytest.raises(NotImplementedError, match="additive"):
        gmb.GPC(cat, outputs=["y"]).specify_model(continuous_dims=["x0"], categorical_dims=["c"], additive=True)
    for name in gmb.GPC.NOT_BUILT:
        with pytest.raises(NotImplementedError, match="classification"):
            getattr(gp, name)()
    assert "cross_validate" in gmb.GPC.NOT_BUILT and "predict_joint" in gmb.GPC.NOT_BUILT
