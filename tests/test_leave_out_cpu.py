"""Leave-one-out and leave-group-out predictions without a GPU: the numpy yardstick (tests/leave_out_reference.py: the rows
literally deleted) held against the closed form the engine computes from one factor, and the layers above the kernels -- header,
binding, refusals, the index check, the front end over an oracle engine.

Bar of the identity: 1e-10 max(1, max|ref|).  Both sides are direct solves in f64 against matrices of cond <= 4.5e5; measured,
printed below: <= 1e-12 at cond 3e3 and <= 9e-12 at cond 4.5e5 -- three orders inside the GPU tests' 1e-8 / 1e-9."""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import leave_out_reference as LR
from oracle import gp_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_loo", "gmb_leave_out"]
PROBLEMS = ["three_term", "matern", "matern_illcond"]


def groups_of(name):
    return LR.three_term_groups() if name == "three_term" else LR.matern_groups()


def gap(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), max(1.0, float(np.max(np.abs(ref))))
    print(f"LEAVE-OUT {what}: max |closed - deleted| = {err:.3e}, scale {scale:.3g}")
    return err / scale


# ---- the identity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PROBLEMS)
def test_closed_form_leave_one_out_is_deletion(name):
    p = LR.problem(name)
    print(f"{name}: N = {p.N}, cond(Sigma) = {p.cond():.3g}")
    for with_noise in (True, False):
        mean, var = p.loo_closed_form(with_noise)
        mean_r, var_r = LR.loo_reference(name, with_noise)
        assert gap(mean, mean_r, f"{name} loo mean noise={with_noise}") <= 1e-10
        assert gap(var, var_r, f"{name} loo var noise={with_noise}") <= 1e-10


@pytest.mark.parametrize("name", PROBLEMS)
def test_closed_form_groups_are_deletion(name):
    p = LR.problem(name)
    for label, rows in groups_of(name).items():
        for with_noise in (True, False):
            mean, cov = p.closed_form(rows, with_noise)
            mean_r, cov_r = p.by_deletion(rows, with_noise)
            assert gap(mean, mean_r, f"{name} {label} (m = {len(rows)}) mean noise={with_noise}") <= 1e-10
            assert gap(cov, cov_r, f"{name} {label} cov noise={with_noise}") <= 1e-10
            assert np.array_equal(cov_r, cov_r.T) or np.max(np.abs(cov_r - cov_r.T)) <= 1e-12


def test_one_row_group_is_leave_one_out():
    p = LR.problem("matern")
    mean, cov = p.by_deletion([699])
    mean_r, var_r = LR.loo_reference("matern")
    assert mean[0] == mean_r[699] and cov[0, 0] == var_r[699]
    scr = np.array([5, 699, 17, 300])
    m1, c1 = p.by_deletion(scr)
    m2, c2 = p.by_deletion(np.sort(scr))
    order = np.argsort(scr)
    assert np.max(np.abs(m1[order] - m2)) <= 1e-12 and np.max(np.abs(c1[np.ix_(order, order)] - c2)) <= 1e-12


@pytest.mark.parametrize("name", PROBLEMS)
def test_noise_and_jitter_conventions(name):
    """with_noise changes the variance by the model's noise at the row; 1 / d exceeds the deletion variance (with noise) by the
    jitter: Sigma holds it, ``O.predict(with_noise=True)`` does not add it."""
    p = LR.problem(name)
    rows = groups_of(name)[list(groups_of(name))[0]]
    _, var1 = p.loo_closed_form(True)
    _, var0 = p.loo_closed_form(False)
    noise = O.noise_diag(p.spec, p.theta, p.X)
    assert np.max(np.abs((var1 - var0) - noise)) <= 1e-12 * max(1.0, float(np.max(var1)))
    _, c1 = p.by_deletion(rows, True)
    _, c0 = p.by_deletion(rows, False)
    assert np.max(np.abs((c1 - c0) - np.diag(noise[rows]))) <= 1e-12 * max(1.0, float(np.max(np.abs(c1))))
    Sinv, _ = p._inverse()
    _, var_r = LR.loo_reference(name, True)
    excess = 1.0 / np.diag(Sinv) - var_r
    print(f"{name}: 1 / d - deletion variance in [{excess.min():.12e}, {excess.max():.12e}] (jitter {p.jitter:g})")
    assert p.jitter == 1e-6 and np.max(np.abs(excess - p.jitter)) <= 1e-11 * max(1.0, float(np.max(var_r)))


def test_deletion_is_the_oracle_prediction_without_the_rows():
    p = LR.problem("three_term")
    rows = LR.three_term_groups()["random37"]
    keep = np.setdiff1d(np.arange(p.N), rows)
    for with_noise in (True, False):
        mu, var = O.predict(p.spec, p.theta, p.X[keep], p.y[keep], p.X[rows], with_noise=with_noise, dist_mode="direct")
        mean, cov = p.by_deletion(rows, with_noise)
        assert np.max(np.abs(mean - mu)) <= 1e-11 * max(1.0, float(np.max(np.abs(mu))))
        assert np.max(np.abs(np.diag(cov) - var)) <= 1e-11 * max(1.0, float(np.max(var)))


# ---- header, binding, refusals ------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import engine

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^int {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    loo = inspect.signature(engine.Engine.loo).parameters
    assert loo["rows"].default is None and loo["with_noise"].default is True
    lo = inspect.signature(engine.Engine.leave_out).parameters
    assert lo["with_noise"].default is True and lo["cov"].default is False
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "leave_out.hpp"' in source


def test_kronecker_and_distributed_engines_refuse():
    from gumbi_amd.distributed import DistributedEngine
    from gumbi_amd.regression.icm import IcmEngine

    with pytest.raises(NotImplementedError, match="Kronecker"):
        IcmEngine.loo(object())
    with pytest.raises(NotImplementedError, match="Kronecker"):
        IcmEngine.leave_out(object(), [0, 1])
    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.loo(object())
    with pytest.raises(NotImplementedError, match="distributed"):
        DistributedEngine.leave_out(object(), [0, 1], cov=True)


def test_index_check_program_builds_and_passes(tmp_path):
    """tools/leave_out_check.cpp: the host-side check of ``idx`` (distinct, in range) that ``gmb_leave_out`` runs before it launches
    anything, driven from a program of its own (its head has the sanitizer build, run by hand)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    exe = tmp_path / "leave_out_check"
    subprocess.run([cxx, "-std=c++17", "-O1", str(ROOT / "tools" / "leave_out_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- the front end over an oracle engine ---------------------------------------------------------------------------------------------
def fitted(monkeypatch, outputs=None, **gp_kwargs):
    from test_gpu_frontend import example_gp

    LR.use_leave_out_oracle(monkeypatch)
    gp = example_gp()
    for key, value in gp_kwargs.items():
        setattr(gp, key, value)
    kwargs = {"outputs": outputs} if outputs else {}
    gp.fit(**kwargs, continuous_dims=["X", "Y"], MAP_kwargs={"maxeval": 8})
    return gp


def test_leave_one_out_of_the_example(monkeypatch):
    gp = fitted(monkeypatch)
    n = len(gp.model.y)
    res = gp.leave_one_out()
    assert sorted(res) == ["mean", "nlpd", "predictions", "var", "z_score"]
    assert res["mean"].shape == res["var"].shape == res["z_score"].shape == res["nlpd"].shape == (n,)
    y = np.asarray(gp.model.y, float)
    assert np.allclose(res["z_score"], (y - res["mean"]) / np.sqrt(res["var"]), rtol=1e-14, atol=0)
    assert np.allclose(res["nlpd"], 0.5 * np.log(2 * np.pi * res["var"]) + 0.5 * res["z_score"] ** 2, rtol=1e-13, atol=1e-13)
    assert list(res["predictions"]) == ["d"]
    want = gp.uparray("d", res["mean"], res["var"], stdzd=True)
    got = res["predictions"]["d"]
    assert np.array_equal(np.asarray(got.z.μ), np.asarray(want.z.μ)) and np.array_equal(np.asarray(got.z.σ2), np.asarray(want.z.σ2))
    # the numbers are the oracle's prediction of each row from the others
    p = LR.LeaveOut(gp.model.spec.as_dict(), gp._theta_fitted, gp.model.X, gp.model.y)
    for i in (0, n // 2, n - 1):
        keep = np.delete(np.arange(n), i)
        mu, var = O.predict(p.spec, p.theta, p.X[keep], p.y[keep], p.X[i:i + 1], with_noise=True, dist_mode="direct")
        assert abs(res["mean"][i] - mu[0]) <= 1e-11 and abs(res["var"][i] - var[0]) <= 1e-11
    latent = gp.leave_one_out(with_noise=False)
    assert np.allclose(res["var"] - latent["var"], O.noise_diag(p.spec, p.theta, p.X), rtol=0, atol=1e-12)


def test_leave_one_out_splits_a_stacked_table_by_output(monkeypatch):
    gp = fitted(monkeypatch, outputs=["d", "c"], kronecker=False)
    res = gp.leave_one_out()
    n = len(gp.model.y)
    assert sorted(res["predictions"]) == ["c", "d"] and res["mean"].shape == (n,)
    oc = gp.dims.index(gp.out_col)
    col = np.asarray(gp.model.X)[:, oc]
    for name in ("d", "c"):
        rows = np.flatnonzero(col == gp.coords[gp.out_col][name])
        assert len(rows) == n // 2
        want = gp.uparray(name, res["mean"][rows], res["var"][rows], stdzd=True)
        assert np.array_equal(np.asarray(res["predictions"][name].z.μ), np.asarray(want.z.μ))


@pytest.mark.parametrize("outputs", [None, ["d", "c"]])
def test_leave_group_out_by_unit(monkeypatch, outputs):
    gp = fitted(monkeypatch, outputs=outputs, kronecker=False)
    n = len(gp.model.y)
    res = gp.leave_group_out(unit="Name", joint=True)
    wide = gp.data.wide
    assert [r["unit"] for r in res] == list(dict.fromkeys(wide["Name"]))
    covered = np.concatenate([r["rows"] for r in res])
    assert sorted(covered.tolist()) == list(range(n))
    # the rows of a unit: every output's block holds the table's rows in the table's order
    n_out = 2 if outputs else 1
    block = n // n_out
    names = wide["Name"].to_numpy()
    assert len(names) == block
    for r in res:
        in_table = np.flatnonzero(names == r["unit"])
        assert np.array_equal(np.sort(r["rows"]), np.sort(np.concatenate([in_table + k * block for k in range(n_out)])))
        m = len(r["rows"])
        assert r["mean"].shape == r["var"].shape == (m,) and r["cov"].shape == (m, m) and np.isscalar(r["nlpd"])
        assert np.allclose(np.diag(r["cov"]), r["var"], rtol=1e-12, atol=0)
    one = res[1]
    resid = np.asarray(gp.model.y)[one["rows"]] - one["mean"]
    _, logdet = np.linalg.slogdet(one["cov"])
    want = 0.5 * resid @ np.linalg.solve(one["cov"], resid) + 0.5 * logdet + 0.5 * len(resid) * np.log(2 * np.pi)
    assert abs(one["nlpd"] - want) <= 1e-9 * max(1.0, abs(want))
    plain = gp.leave_group_out(unit="Name")
    assert "cov" not in plain[1] and plain[1]["nlpd"].shape == (len(one["rows"]),)
    assert np.array_equal(plain[1]["mean"], one["mean"])


def test_leave_group_out_folds_and_groups(monkeypatch):
    gp = fitted(monkeypatch)
    n = len(gp.model.y)
    folds = gp.leave_group_out(n_folds=5, seed=3)
    again = gp.leave_group_out(n_folds=5, seed=3)
    other = gp.leave_group_out(n_folds=5, seed=4)
    assert len(folds) == 5 and sorted(np.concatenate([f["rows"] for f in folds]).tolist()) == list(range(n))
    assert all(np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["mean"], b["mean"]) for a, b in zip(folds, again))
    assert any(not np.array_equal(a["rows"], b["rows"]) for a, b in zip(folds, other))
    default = gp.leave_group_out(n_folds=5)
    seeded = gp.leave_group_out(n_folds=5, seed=gp.seed)
    assert all(np.array_equal(a["rows"], b["rows"]) for a, b in zip(default, seeded))
    res = gp.leave_group_out(groups=[[3, 1, 7], np.array([0])])
    assert [r["rows"].tolist() for r in res] == [[3, 1, 7], [0]] and "unit" not in res[0]
    loo = gp.leave_one_out()
    assert abs(res[1]["mean"][0] - loo["mean"][0]) <= 1e-12 and abs(res[1]["var"][0] - loo["var"][0]) <= 1e-12
    for bad in ({"unit": "Name", "n_folds": 3}, {"groups": [[0]], "n_folds": 3}, {"unit": "Name", "groups": [[0]]}, {}):
        with pytest.raises(ValueError, match="exactly one"):
            gp.leave_group_out(**bad)
    with pytest.raises(ValueError, match="not a column"):
        gp.leave_group_out(unit="nope")
    with pytest.raises(ValueError, match="n_folds"):
        gp.leave_group_out(n_folds=0)


def test_front_end_refusals(monkeypatch):
    from test_gpu_frontend import example_gp

    LR.use_leave_out_oracle(monkeypatch)
    gp = example_gp()
    gp.specify_model(continuous_dims=["X", "Y"])
    gp.build_model()
    with pytest.raises(ValueError, match="must be fit"):
        gp.leave_one_out()
    with pytest.raises(ValueError, match="must be fit"):
        gp.leave_group_out(n_folds=2)
    fit = fitted(monkeypatch)
    fit.distributed = True
    with pytest.raises(NotImplementedError, match="distributed"):
        fit.leave_one_out()
    with pytest.raises(NotImplementedError, match="distributed"):
        fit.leave_group_out(n_folds=2)
    kron = fitted(monkeypatch, outputs=["d", "c"], kronecker=True)
    from gumbi_amd.regression.icm import IcmEngine

    assert isinstance(kron.engine, IcmEngine)
    with pytest.raises(NotImplementedError, match="kronecker=False"):
        kron.leave_one_out()
    with pytest.raises(NotImplementedError, match="kronecker=False"):
        kron.leave_group_out(unit="Name")
