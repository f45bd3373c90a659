"""Averages of the posterior over groups of points without a GPU: the numpy yardstick (tests/group_average_reference.py: the
definition ``W mu``, ``W C W^T`` on the full joint posterior) held against the algebra the engine computes (G right-hand sides,
nothing M x M), and the layers above the kernels -- header, binding, the task list, refusals, the front end over an oracle engine.

Bar of the identity: 1e-11 max(1, max|ref|).  Both sides are direct solves in f64 against matrices of cond <= 4.5e5; measured,
printed below: <= 2e-12 (mean, cond 4.5e5) and <= 4e-14 (cov) -- three orders inside the GPU tests' 1e-8 / 1e-9."""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import group_average_reference as GA
from oracle import gp_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_predict_groups", "gmb_predict_groups_terms", "gmb_debug_group_tasks"]


def gap(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), max(1.0, float(np.max(np.abs(ref))))
    print(f"GROUP-AVERAGE {what}: max |diff| = {err:.3e}, scale {scale:.3g}")
    return err / scale


# ---- header, binding, task list ---------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^(int|int64_t) {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    pg = inspect.signature(engine.Engine.predict_groups).parameters
    assert list(pg) == ["self", "Xs", "offsets", "weights", "cov", "terms"]
    assert pg["weights"].default is None and pg["cov"].default is False and pg["terms"].default is None
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "group_average.hpp"' in source
    tasks_header = (ROOT / "gumbi_amd" / "csrc" / "group_tasks.hpp").read_text()
    assert f"GROUP_CHUNK = {engine.GROUP_CHUNK};" in tasks_header and engine.GROUP_CHUNK == GA.GROUP_CHUNK
    assert "hip_runtime" not in tasks_header


@pytest.mark.parametrize("chunk", [None, 1, 7, 128])
def test_task_list_covers_every_point_once(chunk):
    from gumbi_amd import engine

    offsets = GA.offsets_of(GA.SIZES)
    tasks = engine.group_tasks(offsets, chunk)
    limit = engine.GROUP_CHUNK if chunk is None else chunk
    seen = np.zeros(int(offsets[-1]), dtype=int)
    for g, m0, cnt in tasks:
        assert 1 <= cnt <= limit and offsets[g] <= m0 and m0 + cnt <= offsets[g + 1]
        seen[m0:m0 + cnt] += 1
    assert np.all(seen == 1)
    assert tasks == sorted(tasks) and len(set(tasks)) == len(tasks)
    assert len(tasks) == sum(-(-n // limit) for n in GA.SIZES)
    if chunk is None:  # the longest group: two full tasks and a point
        g = GA.SIZES.index(2 * GA.GROUP_CHUNK + 1)
        assert [cnt for gg, _, cnt in tasks if gg == g] == [GA.GROUP_CHUNK, GA.GROUP_CHUNK, 1]


@pytest.mark.parametrize("bad", [[0, 2, 2, 5], [1, 3], [0, 4, 3], [0], []])
def test_task_list_refuses_malformed_offsets(bad):
    from gumbi_amd import engine

    with pytest.raises(ValueError):
        engine.group_tasks(bad)


def test_task_program_builds_and_passes(tmp_path):
    """tools/group_tasks_check.cpp: the offsets check and the task list that ``gmb_predict_groups`` runs before it launches
    anything, driven from a program of its own (its head has the sanitizer build, run by hand)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "group_tasks_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "group_tasks_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- the yardstick against itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", GA.WEIGHTS)
@pytest.mark.parametrize("name", GA.PROBLEMS)
def test_definition_is_the_engines_algebra(name, kind):
    Xs, offsets = GA.points(name, "sizes")
    w = GA.weights_of(name, "sizes", kind)
    mean_r, cov_r = GA.reference(name, "sizes", kind)
    mean, cov = GA.a_form(*GA.problem(name), Xs, offsets, w)
    assert gap(mean, mean_r, f"{name} {kind} mean") <= 1e-11
    assert gap(cov, cov_r, f"{name} {kind} cov") <= 1e-11
    assert np.max(np.abs(cov_r - cov_r.T)) <= 1e-13


def test_definition_of_a_term_selection():
    name = "three_term"
    Xs, offsets = GA.points(name, "many")
    total = GA.reference(name, "many", "mean")
    parts = [GA.reference(name, "many", "mean", 1 << t) for t in range(3)]
    assert gap(sum(p[0] for p in parts), total[0], "single-term means sum to the total's") <= 1e-11
    mean, cov = GA.a_form(*GA.problem(name), Xs, offsets, None, terms=0b101)
    assert gap(mean, GA.reference(name, "many", "mean", 0b101)[0], "terms 0b101 mean") <= 1e-11
    assert gap(cov, GA.reference(name, "many", "mean", 0b101)[1], "terms 0b101 cov") <= 1e-11


@pytest.mark.parametrize("name", GA.PROBLEMS)
def test_one_point_group_is_the_latent_prediction(name):
    spec, theta, X, y = GA.problem(name)
    Xs, offsets = GA.points(name, "sizes")
    mean_r, cov_r = GA.reference(name, "sizes", "mean")
    assert GA.SIZES[0] == 1
    mu, var = O.predict(spec, theta, X, y, Xs[:1], with_noise=False, dist_mode="direct")
    assert abs(mean_r[0] - mu[0]) <= 1e-11 * max(1.0, abs(mu[0])) and abs(cov_r[0, 0] - var[0]) <= 1e-11


def test_variance_of_an_average_is_not_the_mean_of_the_variances():
    name = "matern"
    spec, theta, X, y = GA.problem(name)
    Xs, offsets = GA.points(name, "sizes")
    _, cov_r = GA.reference(name, "sizes", "mean")
    _, var = O.predict(spec, theta, X, y, Xs, with_noise=False, dist_mode="direct")
    naive = np.array([var[offsets[g]:offsets[g + 1]].mean() for g in range(len(GA.SIZES))])
    ratio = naive / np.diag(cov_r)
    print("GROUP-AVERAGE mean of variances / variance of the mean, per group:", np.array2string(ratio, precision=3))
    assert abs(ratio[0] - 1.0) <= 1e-9  # one point: the same thing
    assert np.all(ratio[2:] > 1.5)      # an average over many points is known better than its points


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_kronecker_and_distributed_engines_refuse():
    from gumbi_amd.distributed import DistributedEngine
    from gumbi_amd.regression.icm import IcmEngine

    with pytest.raises(NotImplementedError, match="Kronecker.*kronecker=False"):
        IcmEngine.predict_groups(object(), np.zeros((2, 2)), [0, 2])
    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.predict_groups(object(), np.zeros((2, 2)), [0, 2], cov=True)


# ---- the front end over an oracle engine ---------------------------------------------------------------------------------------------
def fitted(monkeypatch, outputs=None, **fit_kwargs):
    from test_gpu_frontend import example_gp

    GA.use_group_oracle(monkeypatch)
    gp = example_gp()
    gp.kronecker = False
    kwargs = {"outputs": outputs} if outputs else {}
    gp.fit(**kwargs, **{"continuous_dims": ["X", "Y"], **fit_kwargs}, MAP_kwargs={"maxeval": 8})
    return gp


def joint_of(gp, points_array, offsets, weights, terms=None):
    return GA.by_joint(gp.model.spec.as_dict(), gp._theta_fitted, gp.model.X, gp.model.y, points_array, offsets, weights, terms)


def test_predict_average_sorts_labels(monkeypatch):
    gp = fitted(monkeypatch)
    rng = np.random.default_rng(2)
    M = 23
    pts = gp.parray(X=rng.normal(0.0, 1.0, M), Y=rng.normal(0.0, 1.0, M), stdzd=True)
    labels = rng.permutation(np.repeat([7, -2, 40, 3], [5, 9, 1, 8]))
    avg, cov = gp.predict_average(pts, groups=labels, joint=True)
    assert avg.shape == (4,) and cov.shape == (4, 4) and list(gp.average_labels) == [-2, 3, 7, 40]
    pa, _, _ = gp._prepare_points_for_prediction(pts, output=["d"])
    for k, label in enumerate(gp.average_labels):
        rows = np.flatnonzero(labels == label)
        m, c = joint_of(gp, pa[rows], [0, len(rows)], None)
        assert abs(float(avg.z.μ[k]) - m[0]) <= 1e-11 and abs(float(avg.z.σ2[k]) - c[0, 0]) <= 1e-11 and abs(cov[k, k] - c[0, 0]) <= 1e-11
    one = gp.predict_average(pts)
    m, c = joint_of(gp, pa, [0, M], None)
    assert one.shape == (1,) and abs(float(one.z.μ[0]) - m[0]) <= 1e-11 and abs(float(one.z.σ2[0]) - c[0, 0]) <= 1e-11
    w = rng.normal(0.0, 1.0, M)
    signed = gp.predict_average(pts, weights=w)
    m, c = joint_of(gp, pa, [0, M], w)
    assert abs(float(signed.z.μ[0]) - m[0]) <= 1e-11 and abs(float(signed.z.σ2[0]) - c[0, 0]) <= 1e-11
    with pytest.raises(ValueError, match="one integer label per point"):
        gp.predict_average(pts, groups=labels[:-1])
    with pytest.raises(ValueError, match="weights for"):
        gp.predict_average(pts, weights=w[:-1])


def test_predict_marginal_of_the_example(monkeypatch):
    gp = fitted(monkeypatch)
    n = len(gp.model.y)
    pred = gp.predict_marginal("X", resolution=7, joint=True)
    assert pred.shape == (7,) and gp.marginal_points.shape == (7,) and gp.marginal_points.names == ["X"]
    assert gp.marginal_cov.shape == (7, 7) and np.max(np.abs(gp.marginal_cov - gp.marginal_cov.T)) <= 1e-13
    design = gp.marginal_design("X", resolution=7)
    assert design["points_array"].shape == (7 * n, len(gp.dims)) and np.array_equal(design["offsets"], np.arange(8) * n)
    limits = gp._default_grid_limits({"X"}).z["X_z"].values()
    assert np.allclose(design["grid"].z["X_z"].values(), np.linspace(limits[0], limits[1], 7), rtol=0, atol=1e-12)
    xc, yc = gp.dims.index("X"), gp.dims.index("Y")
    block = design["points_array"][2 * n:3 * n]
    assert np.all(block[:, xc] == block[0, xc]) and np.array_equal(block[:, yc], np.asarray(gp.model.X)[:, yc])
    mean_r, cov_r = joint_of(gp, design["points_array"], design["offsets"], design["weights"])
    assert gap(np.asarray(pred.z.μ), mean_r, "marginal mean") <= 1e-11
    assert gap(np.asarray(pred.z.σ2), np.diag(cov_r), "marginal var") <= 1e-11
    assert gap(gp.marginal_cov, cov_r, "marginal cov") <= 1e-11
    plain = gp.predict_marginal("X", resolution=7)
    assert gp.marginal_cov is None and np.array_equal(np.asarray(plain.z.μ), np.asarray(pred.z.μ))
    # two dimensions: the grid's shape, axes in the model's order
    both = gp.predict_marginal(["Y", "X"], resolution={"X": 3, "Y": 4}, n_background=9, seed=1)
    assert both.shape == (3, 4) and gp.marginal_points.names == ["X", "Y"]
    # a seeded subset of the background is reproducible, another seed another subset
    a = gp.predict_marginal("Y", resolution=5, n_background=11, seed=4)
    b = gp.predict_marginal("Y", resolution=5, n_background=11, seed=4)
    c = gp.predict_marginal("Y", resolution=5, n_background=11, seed=5)
    assert np.array_equal(np.asarray(a.z.μ), np.asarray(b.z.μ)) and not np.array_equal(np.asarray(a.z.μ), np.asarray(c.z.μ))
    assert gp.marginal_design("Y", resolution=5, n_background=11, seed=4)["points_array"].shape == (55, len(gp.dims))
    # a parray background
    back = gp.parray(Y=np.array([-0.5, 0.25, 1.0]), stdzd=True)
    over = gp.predict_marginal("X", resolution=4, over=back)
    design = gp.marginal_design("X", resolution=4, over=back)
    assert design["points_array"].shape == (12, len(gp.dims)) and np.allclose(design["points_array"][:3, yc], [-0.5, 0.25, 1.0])
    assert gap(np.asarray(over.z.μ), joint_of(gp, design["points_array"], design["offsets"], design["weights"])[0], "parray background") <= 1e-11
    with pytest.raises(ValueError, match="one or two of the continuous"):
        gp.predict_marginal("Code")
    with pytest.raises(ValueError, match="n_background"):
        gp.predict_marginal("X", n_background=n + 1)


def test_compare_levels_is_antisymmetric(monkeypatch):
    gp = fitted(monkeypatch, categorical_dims="Name")
    levels = gp.categorical_levels["Name"]
    ab = gp.compare_levels("Name", levels[0], levels[1])
    ba = gp.compare_levels("Name", levels[1], levels[0])
    assert sorted(ab) == ["levels", "mean", "n_background", "var", "z_score"] and ab["levels"] == (levels[0], levels[1])
    assert abs(ab["mean"] + ba["mean"]) <= 1e-12 * max(1.0, abs(ab["mean"])) and abs(ab["var"] - ba["var"]) <= 1e-12 * max(1.0, ab["var"])
    assert ab["z_score"] == ab["mean"] / np.sqrt(ab["var"]) and ab["var"] > 0.0
    assert ab["n_background"] == len(gp.model.y)
    same = gp.compare_levels("Name", levels[0], levels[0])
    assert abs(same["mean"]) <= 1e-12 and abs(same["var"]) <= 1e-11
    with pytest.raises(ValueError, match="not a categorical dimension"):
        gp.compare_levels("X", levels[0], levels[1])
    with pytest.raises(ValueError, match="not a level"):
        gp.compare_levels("Name", levels[0], "nope")


def test_front_end_refusals(monkeypatch):
    from gumbi_amd.regression.hip_gp import UnknownAdditiveLevel
    from test_gpu_frontend import example_gp

    GA.use_group_oracle(monkeypatch)
    gp = example_gp()
    gp.specify_model(continuous_dims=["X", "Y"])
    gp.build_model()
    with pytest.raises(ValueError, match="must be fit"):
        gp.predict_groups(np.zeros((2, 2)), [0, 2])
    gp = fitted(monkeypatch)
    pts = gp.parray(X=np.zeros(3), Y=np.zeros(3), stdzd=True)
    for call in (lambda: gp.predict_average(pts, additive_level="nope"), lambda: gp.predict_marginal("X", additive_level="nope"),
                 lambda: gp.predict_groups(np.zeros((2, 2)), [0, 2], additive_level="nope")):
        with pytest.raises(UnknownAdditiveLevel):
            call()
    gp.distributed = True
    with pytest.raises(NotImplementedError, match="distributed"):
        gp.predict_average(pts)
    two = fitted(monkeypatch, outputs=["d", "c"])
    pts2 = two.parray(X=np.zeros(3), Y=np.zeros(3), stdzd=True)
    with pytest.raises(ValueError, match="ONE output"):
        two.predict_average(pts2)
    with pytest.raises(ValueError, match="ONE output"):
        two.predict_marginal("X")
    one = two.predict_marginal("X", resolution=3, output="c")
    assert one.shape == (3,) and one.name == "c"
    design = two.marginal_design("X", resolution=3, output="c")
    oc = two.dims.index(two.out_col)
    assert np.all(design["points_array"][:, oc] == two.coords[two.out_col]["c"]) and design["points_array"].shape[0] == 3 * (len(two.model.y) // 2)
