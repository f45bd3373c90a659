"""A batch of experiments by greedy integrated variance reduction on the CPU (``-m "not gpu"``: runs anywhere):
tests/design_reference.py -- the definition ``gmb_design_batch`` implements, in numpy -- against an independent route, the
conditions the GPU tests rely on, and the layers above the engine on an oracle-backed stand-in.

1. Header, binding, the plan header and its check program (plain and under the address / undefined-behaviour sanitizers, as a
   stand-alone program).
2. The yardstick against an independent route.  The rows ``D0`` are the first M rows of ``group_average_reference.joint_posterior``
   (the same products; 1e-12 relative for the different matrix shapes BLAS sees; the variances, which are the prediction's
   ``k** - |V|^2``, 2e-11: see the test).  After the reference's picks,
   ``sum_r w_r var(r)`` of an oracle GP with those points ADDED to the training set equals ``ivar0 - sum gains``: bar 1e-10
   relative to ivar0 -- both sides are O(N^3) double-precision routes on matrices with cond <= 4.5e5, where the sibling files
   measure 2e-12.  Measured: 0 .. 5e-15 with noise, 1.0e-11 .. 1.5e-11 without (there the route is the joint posterior of the
   picks and the reference points, whose diagonal differs from the prediction's variance as above).
3. The gap condition: for every problem and step the GPU tests use, the reference's best gain exceeds its runner-up by more than
   100 x the gain bar, so the picks are decided far above the engine's rounding and no step is left out there.
4. The front end over ``DesignOracleEngine``: seeded default candidates, categorical levels, repeats, the attributes, refusals.
"""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import design_reference as DR
import group_average_reference as GA

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_design_batch", "gmb_debug_design_plan"]


# ---- 1. header, binding, plan -------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^(int|int64_t) {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    ps = inspect.signature(engine.Engine.design_batch).parameters
    assert list(ps) == ["self", "Xc", "Xr", "q", "weights", "with_noise", "allow_repeats"]
    assert ps["weights"].default is None and ps["with_noise"].default is True and ps["allow_repeats"].default is True
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "design_batch.hpp"' in source
    plan = (ROOT / "gumbi_amd" / "csrc" / "design_plan.hpp").read_text()
    assert "#include <hip" not in plan and "hip_runtime" not in plan and '#include "' not in plan


def test_plan_follows_the_header():
    from gumbi_amd import engine

    plan = engine.design_plan(768, 130, 2 * DR.DESIGN_CHUNK + 1)
    assert plan["chunk"] == DR.DESIGN_CHUNK and plan["Mc"] == 256 and plan["ld"] == 256 + 4224 and plan["nchunk"] == 3
    assert plan["tiles"] == [(0, 130, 256, 0), (130, 4097, 4224, 256)] and plan["mt"] == 4224
    assert plan["chunks"] == [(0, 2048), (2048, 4096), (4096, 4480)]
    far = engine.design_plan(10112, 1024, 100000)  # reference points in tiles of a prediction's 32768 rows
    assert [t[1] for t in far["tiles"]] == [1024, 32768, 32768, 32768, 1696] and far["tiles"][2][3] == 1024 + 32768
    assert far["own_bytes"] >= 8 * 1024 * (10112 + far["ld"])
    for bad in ((768, 0, 5), (768, 5, 0), (700, 5, 5), (768, 32769, 5), (1000064, 1025, 5)):
        with pytest.raises(ValueError):
            engine.design_plan(*bad)


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_plan_program_builds_and_passes(tmp_path, flags):
    """tools/design_plan_check.cpp: the tiles, columns, chunks and slots ``gmb_design_batch`` computes before it launches anything,
    driven from a program of its own."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler on this machine"
    exe = tmp_path / "design_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", *flags, str(ROOT / "tools" / "design_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- 2. the yardstick against an independent route ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GA.PROBLEMS)
def test_rows_are_the_joint_posteriors(name):
    spec, theta, X, y = GA.problem(name)
    rng = np.random.default_rng(5)
    Xc, Xr = DR.jittered_rows(name, 9, rng), DR.jittered_rows(name, 40, rng)
    D0, var_r = DR.posterior_rows(spec, theta, X, y, Xc, Xr)
    _, C = GA.joint_posterior(spec, theta, X, y, np.vstack([Xc, Xr]))
    scale = float(np.max(np.abs(C)))
    gap = float(np.max(np.abs(D0 - C[:9]))) / scale, float(np.max(np.abs(var_r - np.diag(C)[9:]))) / scale
    print(f"DESIGN-CPU {name}: rows against the joint posterior {gap[0]:.2e}, variances {gap[1]:.2e}")
    # (the variances are the PREDICTION's k** - |V|^2 with k** = eta^2 exactly, as pm.gp.cov.Stationary.diag; the joint posterior's
    # diagonal goes through sqrt(r^2 + 1e-12) at r = 0, which for a Matern-5/2 kernel is eta^2 (1 - 5/6 1e-12): 1e-12 eta^2 apart
    # by definition, eta^2 up to ~6 max|C| on these problems)
    assert gap[0] <= 1e-12 and gap[1] <= 2e-11


@pytest.mark.parametrize("with_noise,allow_repeats", [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize("name", GA.PROBLEMS)
def test_gains_are_what_conditioning_on_the_picks_removes(name, with_noise, allow_repeats):
    """(without noise a repeat has gain 0 up to rounding and conditioning twice on a noiseless point is singular: that
    combination is left to the definition)"""
    spec, theta, X, y = GA.problem(name)
    rng = np.random.default_rng(8)
    Xc, Xr = DR.jittered_rows(name, 40, rng), DR.jittered_rows(name, 150, rng)
    w = rng.uniform(0.0, 2.0, len(Xr)) / len(Xr)
    D0, var_r = DR.posterior_rows(spec, theta, X, y, Xc, Xr)
    noise = np.asarray(DR.O.noise_diag(spec, np.asarray(theta, float), Xc)) if with_noise else np.zeros(len(Xc))
    res = DR.greedy(D0, noise, w, 6, allow_repeats)
    assert np.all(res["picks"] >= 0)
    ivar0 = float(w @ var_r)
    if not with_noise:  # a measurement without noise: the oracle's Sigma needs the point's noise to be the model's, so condition by hand
        left = ivar0 - float(np.sum(res["gains"]))
        P = np.vstack([Xc[res["picks"]], Xr])
        _, C = GA.joint_posterior(spec, theta, X, y, P)
        k = len(res["picks"])
        cond = C[k:, k:] - C[k:, :k] @ np.linalg.solve(C[:k, :k], C[:k, k:])
        other = float(w @ np.diag(cond))
    else:
        left = ivar0 - float(np.sum(res["gains"]))
        other = DR.by_conditioning(spec, theta, X, y, Xc, Xr, res["picks"], w)
    gap = abs(left - other) / ivar0
    print(f"DESIGN-CPU {name} noise {with_noise} repeats {allow_repeats}: picks {res['picks'].tolist()}, ivar0 {ivar0:.6e}, "
          f"left {left:.6e}, by conditioning {other:.6e}, gap {gap:.2e} of ivar0")
    assert gap <= 1e-10


# ---- 3. the gap condition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_every_pick_of_the_gpu_cases_is_decided_far_above_the_bar(name):
    worst = np.inf
    for M in DR.M_SIZES:
        for R in DR.R_SIZES:
            for with_noise, allow_repeats in ((True, True), (True, False), (False, False)):
                ref, _ = DR.reference(name, M, R, with_noise, allow_repeats)
                for t in range(DR.Q_MAX):
                    if ref["picks"][t] < 0 or not np.isfinite(ref["gaps"][t]):
                        continue  # (M = 1: nobody to confuse the pick with)
                    ratio = ref["gaps"][t] / ref["bars"][t]
                    worst = min(worst, ratio)
                    assert ratio > 100.0, f"{name} M = {M} R = {R} noise {with_noise} repeats {allow_repeats} step {t}: gap / bar = {ratio:.1f}"
    print(f"DESIGN-CPU {name}: smallest (best gain - runner-up) / bar over the GPU cases = {worst:.3g}")


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_the_duplicates_case_ties_only_between_the_copies(name, with_noise):
    _, _, ref, _, (lo, hi) = DR.duplicates_case(name, with_noise)
    picks = ref["picks"].tolist()
    assert np.all(ref["picks"] >= 0) and len(set(picks)) == len(picks)
    assert lo < hi and picks[0] == lo  # the best candidate and its copy tie: the lower index goes first
    ratios = ref["gaps"] / ref["bars"]
    print(f"DESIGN-CPU {name} duplicates noise {with_noise}: picks {picks}, smallest gap / bar {ratios.min():.3g}")
    assert np.all(ratios > 100.0)


def test_run_off_case_ends_in_minus_ones():
    ref, _ = DR.reference("matern", 5, 129, True, False, 7)
    assert np.all(ref["picks"][:5] >= 0) and sorted(ref["picks"][:5]) == [0, 1, 2, 3, 4]
    assert ref["picks"][5:].tolist() == [-1, -1] and ref["gains"][5:].tolist() == [0.0, 0.0]
    assert np.all(ref["gaps"][:4] / ref["bars"][:4] > 100.0)


# ---- 4. the front end ------------------------------------------------------------------------------------------------------------------
def fitted(monkeypatch, outputs=("y",), kronecker="auto", n=40):
    import gumbi_amd as gmb
    from test_gpu_predict_grad import frontend_dataset

    DR.use_design_oracle(monkeypatch)
    outputs = list(outputs)
    gp = gmb.GP(frontend_dataset(n, outputs), outputs=outputs if len(outputs) > 1 else outputs[0], kronecker=kronecker)
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 10})
    return gp


def test_default_design_is_seeded_and_sets_the_attributes(monkeypatch):
    gp = fitted(monkeypatch)
    picked = gp.design_batch(5, n_candidates=64, n_reference=200, seed=7)
    assert isinstance(gp.engine, DR.DesignOracleEngine)
    assert picked.names == ["a", "b"] and picked.shape == (5,)
    picks, gains, scores = gp.design_picks.copy(), gp.design_gains.copy(), gp.design_scores.copy()
    assert picks.shape == (5,) and gains.shape == (5,) and scores.shape == (64,) and gp.design_candidates.shape == (64,)
    assert np.all(gains > 0) and np.all(np.diff(gains) <= 0) and 0 < gains.sum() < gp.design_ivar0
    assert gains[0] == scores.max() and picks[0] == int(np.argmax(scores))
    cand = np.column_stack([gp.design_candidates.z["a_z"].values(), gp.design_candidates.z["b_z"].values()])
    lo, hi = np.asarray(gp.model.X, float).min(0), np.asarray(gp.model.X, float).max(0)
    assert np.all(cand >= lo - 1e-12) and np.all(cand <= hi + 1e-12)  # inside the data's limits
    assert np.array_equal(np.column_stack([picked.z["a_z"].values(), picked.z["b_z"].values()]), cand[picks])
    again = gp.design_batch(5, n_candidates=64, n_reference=200, seed=7)
    assert np.array_equal(gp.design_picks, picks) and np.array_equal(gp.design_gains, gains)
    assert np.array_equal(again.z["a_z"].values(), picked.z["a_z"].values())
    gp.design_batch(5, n_candidates=64, n_reference=200, seed=8)
    assert not np.array_equal(gp.design_scores, scores)
    # the q = 0 form on given points: the step-0 scores
    ref = gp.design_candidates
    vr = gp.variance_reduction(gp.parray(a=np.array([1.0, 2.0, 3.0]), b=np.array([12.0, 15.0, 18.0])), ref)
    assert vr.shape == (3,) and np.all(vr > 0)
    with pytest.raises(ValueError, match="q must be"):
        gp.design_batch(-1)


def test_bounds_confine_the_default_points(monkeypatch):
    gp = fitted(monkeypatch)
    bounds = gp.parray(a=np.array([1.0, 2.0]), b=np.array([12.0, 13.0]))
    gp.design_batch(2, n_candidates=32, n_reference=50, bounds=bounds, seed=1)
    a, b = gp.design_candidates["a"].values(), gp.design_candidates["b"].values()
    assert np.all((a >= 1.0 - 1e-9) & (a <= 2.0 + 1e-9) & (b >= 12.0 - 1e-9) & (b <= 13.0 + 1e-9))


def test_replicates_are_returned_twice(monkeypatch):
    gp = fitted(monkeypatch)
    one = gp.parray(a=np.array([2.0]), b=np.array([15.0]))
    ref = gp.parray(a=np.linspace(1.0, 3.5, 30), b=np.linspace(11.0, 19.0, 30))
    picked = gp.design_batch(3, candidates=one, reference=ref)
    assert picked.shape == (3,) and gp.design_picks.tolist() == [0, 0, 0] and np.all(np.diff(gp.design_gains) < 0)
    assert np.allclose(picked["a"].values(), 2.0) and np.allclose(picked["b"].values(), 15.0)
    once = gp.design_batch(3, candidates=one, reference=ref, allow_repeats=False)
    assert once.shape == (1,) and gp.design_picks.tolist() == [0, -1, -1] and gp.design_gains[1:].tolist() == [0.0, 0.0]


def test_categorical_levels_are_appended(monkeypatch):
    from test_joint_cpu import model_2d_categorical

    DR.use_design_oracle(monkeypatch)
    gp = model_2d_categorical()
    levels = gp.categorical_levels["Name"]
    with pytest.raises(AttributeError, match="every categorical dimension"):
        gp.design_batch(2, n_candidates=8, n_reference=8)
    scores = []
    for level in levels[:2]:
        picked = gp.design_batch(2, n_candidates=16, n_reference=40, categorical_levels={"Name": level}, seed=3)
        assert set(picked.names) == {"X", "Y"} and picked.shape == (2,)
        scores.append(gp.design_scores.copy())
    assert not np.array_equal(scores[0], scores[1])  # the same coordinates at another level: another posterior


def test_kronecker_and_distributed_refuse(monkeypatch):
    from gumbi_amd.distributed import DistributedEngine
    from gumbi_amd.regression import icm

    gk = fitted(monkeypatch, ("y", "w"))
    assert isinstance(gk.engine, icm.IcmEngine)
    with pytest.raises(NotImplementedError, match="single-device"):
        gk.design_batch(2, n_candidates=8, n_reference=8)
    with pytest.raises(NotImplementedError, match="single-device"):
        gk.engine.design_batch(np.zeros((1, 3)), np.zeros((1, 3)), 1)
    with pytest.raises(NotImplementedError, match="single-device"):
        DistributedEngine.design_batch(object(), np.zeros((1, 1)), np.zeros((1, 1)), 1)
    stacked = fitted(monkeypatch, ("y", "w"), kronecker=False)
    with pytest.raises(ValueError, match="ONE output"):
        stacked.design_batch(2, n_candidates=8, n_reference=8)
    assert stacked.design_batch(2, n_candidates=8, n_reference=8, output="w").shape == (2,)
