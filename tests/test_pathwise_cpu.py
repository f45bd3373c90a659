"""Pathwise posterior draws on the CPU (``-m "not gpu"``: runs anywhere): the host side ``gumbi_amd/pathwise.py``, the numpy
reference ``tests/pathwise_reference.py`` the GPU tests hold the engine to, and the plan program.

1. Header, binding, the plan header and its check program (plain and under the address / undefined-behaviour sanitizers, as a
   stand-alone program).
2. Spectral sampling, all five kinds: ``max |Phi Phi^T - K|`` over 24 points uniform in [-2, 2]^D at F = 4096, D in {1, 2, 4, 8},
   20 seeds.  Bar ``6 sqrt(1.5 / F) eta^2``: one feature product ``2 cos(a) cos(b) = cos(a - b) + cos(a + b)`` has variance
   <= 1 (the difference) + 1/2 (the sum, uniform phase) = 1.5, so the bar is six standard deviations of the mean of F of them.
3. The antithetic identity: the pair mean of the reference paths equals ``k(x*, X) Sigma^-1 y`` to 1e-11 relative.
4. The gradient formula against Richardson central differences (h = 1e-4 and h / 2) of the reference value evaluated in
   ``np.longdouble``: bar ``1e-9 max|grad|``, the bar tests/test_predict_batches_cpu.py uses for its derivative check (there with
   the error budget of the differences: truncation ~ h^4 f^(5), 1.5e-12 for the kinked kinds; rounding 1e-19 / h).
5. ``path_inputs``: reproducible from the seed, shapes, the antithetic sign pattern.
6. The pointwise variance of 4096 reference draws against the exact posterior variance: PRINTED, not bounded (the random-feature
   prior is an approximation; DESIGN §3.20 records the ratio).
"""
import functools
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pathwise_reference as PR
from gumbi_amd import pathwise
from oracle import gp_oracle as O

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ["gmb_paths_prepare", "gmb_paths_eval", "gmb_paths_eval_own", "gmb_paths_clear", "gmb_paths_count", "gmb_debug_paths_plan"]


# ---- 1. header, binding, plan -------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_calls():
    from gumbi_amd import distributed, engine
    from gumbi_amd.regression import icm

    header = (ROOT / "include" / "gumbi_hip.h").read_text()
    for name in NEW_CALLS:
        assert re.search(rf"^(int|int32_t|int64_t) {name}\(", header, re.M), f"{name} is not declared in include/gumbi_hip.h"
        assert name in engine.exported_symbols(), f"{name} is not bound"
    assert engine.ABI_VERSION == 16 and "#define GMB_ABI_VERSION 16" in header
    for method in ("paths_prepare", "paths_eval", "paths_eval_own", "paths_clear"):
        ps = inspect.signature(getattr(engine.Engine, method)).parameters
        for stand_in in (icm.IcmEngine, distributed.DistributedEngine):
            assert list(inspect.signature(getattr(stand_in, method)).parameters) == list(ps)
            with pytest.raises(NotImplementedError, match=method):
                getattr(stand_in, method)(None, *[None] * (len(ps) - 1))
    source = (ROOT / "gumbi_amd" / "csrc" / "engine.hip").read_text()
    assert '#include "pathwise.hpp"' in source
    plan = (ROOT / "gumbi_amd" / "csrc" / "paths_plan.hpp").read_text()
    assert "#include <hip" not in plan and "hip_runtime" not in plan and '#include "' not in plan
    kernels = (ROOT / "gumbi_amd" / "csrc" / "pathwise.hpp").read_text()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in kernels and "atomic" not in kernels.split("#pragma once")[1]
    for helper in ("paths_lane_row", "paths_lane_k", "paths_result_row", "paths_range", "paths_draw_tiles", "paths_part_at", "paths_own_part_at"):
        assert f"{helper}(" in kernels, f"the kernels do not index through the plan header's {helper}"  # (what the plan program checks)
    module = (ROOT / "gumbi_amd" / "pathwise.py").read_text()
    assert "engine" not in [ln.split()[-1] for ln in module.splitlines() if ln.startswith(("import ", "from "))]


def test_plan_follows_the_header():
    from gumbi_amd import engine

    plan = engine.paths_plan(10000, 2048, 10**6, 64, nacc=5)  # a 10^6-point grid under 64 draws
    assert plan["Sp"] == 64 and plan["draw_blocks"] == 1 and plan["N4"] == 10000 and plan["F4"] == 2048
    assert plan["mt"] == 65536 and plan["ntile"] == 16
    assert plan["tiles"][0][:4] == (0, 65536, 65536, 4096) and plan["tiles"][0][5] == 1  # a full tile fills the machine: one chunk
    first, mc, mpad, pt, chunk, nchunk, own_chunk, own_nchunk = plan["tiles"][-1]
    assert (first, mc, mpad, pt, nchunk) == (15 * 65536, 16960, 17024, 1060, 2)  # the last tile: 1060 waves per chunk, two chunks
    assert plan["part_doubles"] == 2 * 64 * 17024  # ... whose partials are the only ones the call needs
    assert sum(t[1] for t in plan["tiles"]) == 10**6
    small = engine.paths_plan(300, 1000, 333, 17, nacc=5)  # S crosses a 16-seam: Sp = 32; few point tiles: chunked
    first, mc, mpad, pt, chunk, nchunk, own_chunk, own_nchunk = small["tiles"][0]
    assert small["Sp"] == 32 and (first, mc, mpad, pt) == (0, 333, 384, 21) and chunk % 64 == 0 and nchunk > 1
    assert (nchunk - 1) * chunk < 300 + 1000 <= nchunk * chunk and small["part_doubles"] == nchunk * 32 * 384
    assert small["own_part_doubles"] == own_nchunk * 5 * 384
    for bad in ((300, 64, 10, 0), (300, 64, 10, 513), (300, 0, 10, 4), (300, 16385, 10, 4), (300, 64, 0, 4), (0, 64, 10, 4)):
        with pytest.raises(ValueError):
            engine.paths_plan(*bad)


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_plan_program_builds_and_passes(tmp_path, flags):
    """tools/paths_plan_check.cpp: the point tiles, draw blocks, chunks over N + F, the lane-to-pair map, the partial slots and the
    Sp padding the pathwise calls compute before they launch anything, driven from a program of its own."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler on this machine"
    exe = tmp_path / "paths_plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", *flags, str(ROOT / "tools" / "paths_plan_check.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr


# ---- 2. spectral sampling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", O.KINDS)
def test_feature_products_average_to_the_kernel(kind, D):
    F, eta = 4096, 1.3
    spec = O.make_spec(D, range(D), kind=kind, ard=True)
    bar = 6.0 * np.sqrt(1.5 / F) * eta ** 2
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(100 * D + seed)
        ls = rng.uniform(0.7, 1.8, D)
        theta = O.pack_theta(spec, ls, eta, 0.2)
        X = rng.uniform(-2.0, 2.0, (24, D))
        omega = pathwise.spectral_frequencies(kind, F, D, rng)
        phase = rng.uniform(0.0, 2.0 * np.pi, F)
        Phi = PR.features(spec, theta, omega, phase, X)
        worst = max(worst, float(np.max(np.abs(Phi @ Phi.T - PR.cross_kernel(spec, theta, X, X)))))
    print(f"{kind} D={D}: max |Phi Phi^T - K| = {worst:.3e} = {worst / (np.sqrt(1.5 / F) * eta ** 2):.2f} sqrt(1.5 / F) eta^2 (bar 6)")
    assert worst <= bar
    assert pathwise.spectral_frequencies(O.KINDS[kind], 8, D, np.random.default_rng(1)).tobytes() == \
        pathwise.spectral_frequencies(kind, 8, D, np.random.default_rng(1)).tobytes()


# ---- 3., 4. the reference ------------------------------------------------------------------------------------------------------------
def table(N, d, kind, ard=True):  # tests/test_gpu_predict_grad.py's table and points (that module is marked gpu as a whole)
    X, y, ls = O.synthetic_table(N, d, seed=1000 * d + N)
    spec = O.make_spec(d, range(d), kind=kind, ard=ard)
    return spec, O.pack_theta(spec, ls if ard else [float(np.mean(ls))], 1.1, 0.25), X, y


def points(X, M, cont, seed=1, on_train=0):
    rng = np.random.default_rng(seed)
    Xs = X[rng.integers(0, len(X), M)].copy()
    Xs[on_train:, cont] += 0.3 * rng.standard_normal((M - on_train, len(cont)))
    return Xs


@pytest.mark.parametrize("kind", O.KINDS)
def test_antithetic_pairs_average_to_the_posterior_mean(kind):
    spec, theta, X, y = table(200, 3, kind)
    omega, phase, w, eps = pathwise.path_inputs(kind, 6, 256, 3, len(y), seed=5, antithetic=True)
    Xs = points(X, 50, [0, 1, 2], on_train=10)
    A = PR.coefficients(spec, theta, X, y, omega, phase, w, eps)
    Y = PR.all_draws(spec, theta, X, Xs, omega, phase, w, A)
    mean = PR.posterior_mean(spec, theta, X, y, Xs)
    err = max(float(np.max(np.abs(0.5 * (Y[2 * i] + Y[2 * i + 1]) - mean))) for i in range(3)) / float(np.max(np.abs(mean)))
    print(f"{kind}: pair mean vs k(x*, X) Sigma^-1 y: {err:.2e} relative; spread of the draws {float(np.std(Y - mean)):.3f}")
    assert err <= 1e-11
    assert float(np.std(Y - mean)) > 1e-3  # (the draws themselves are not the mean)


@pytest.mark.parametrize("ard", [True, False], ids=["ard", "shared"])
@pytest.mark.parametrize("kind", O.KINDS)
def test_gradient_formula_against_longdouble_differences(kind, ard):
    spec, theta, X, y = table(120, 3, kind, ard=ard)
    S = 4
    omega, phase, w, eps = pathwise.path_inputs(kind, S, 128, 3, len(y), seed=9)
    A = PR.coefficients(spec, theta, X, y, omega, phase, w, eps)
    Xs = points(X, 12, [0, 1, 2], seed=3)
    draw = np.arange(12) % S
    val, G = PR.own_draws(spec, theta, X, Xs, draw, omega, phase, w, A)
    Y = PR.all_draws(spec, theta, X, Xs, omega, phase, w, A)
    assert np.max(np.abs(val - Y[draw, np.arange(12)])) <= 1e-12 * np.max(np.abs(Y))

    def value(P):
        return PR.own_draws(spec, theta, X, P, draw, omega, phase, w, A, grad=False, dtype=np.longdouble)[0]

    h = np.longdouble(1e-4)
    num = np.zeros_like(G)
    for c in range(3):
        def diff(step):
            E = np.zeros(Xs.shape, np.longdouble)
            E[:, c] = step
            P = np.asarray(Xs, np.longdouble)
            return (value(P + E) - value(P - E)) / (2 * step)
        num[:, c] = np.asarray((4 * diff(h / 2) - diff(h)) / 3, float)
    err, scale = float(np.max(np.abs(G - num))), float(np.max(np.abs(G)))
    print(f"{kind} {'ARD' if ard else 'shared'}: max |G - Richardson| = {err:.3e}, max |G| = {scale:.3e}, ratio {err / scale:.2e}")
    assert err <= 1e-9 * scale


# ---- 5. path_inputs -------------------------------------------------------------------------------------------------------------------
def test_path_inputs_shapes_seed_and_antithetic_signs():
    a = pathwise.path_inputs("Matern52", 7, 33, 3, 50, seed=4)
    b = pathwise.path_inputs("Matern52", 7, 33, 3, 50, seed=4)
    c = pathwise.path_inputs("Matern52", 7, 33, 3, 50, seed=5)
    assert [x.shape for x in a] == [(33, 3), (33,), (7, 33), (7, 50)]
    assert all(x.tobytes() == z.tobytes() for x, z in zip(a, b)) and a[2].tobytes() != c[2].tobytes()
    assert np.all((a[1] >= 0.0) & (a[1] < 2.0 * np.pi))
    omega, phase, w, eps = pathwise.path_inputs("ExpQuad", 7, 33, 2, 50, seed=4, antithetic=True)
    assert w.shape == (7, 33) and eps.shape == (7, 50)
    for i in range(3):
        assert np.array_equal(w[2 * i + 1], -w[2 * i]) and np.array_equal(eps[2 * i + 1], -eps[2 * i])
    assert not np.array_equal(w[6], w[4]) and not np.array_equal(w[2], w[0])
    assert all(x.flags["C_CONTIGUOUS"] for x in (omega, phase, w, eps))
    with pytest.raises(ValueError):
        pathwise.path_inputs("Cubic", 2, 8, 1, 5, seed=0)
    with pytest.raises(ValueError):
        pathwise.path_inputs("ExpQuad", 0, 8, 1, 5, seed=0)


def test_a_set_of_paths_knows_when_it_is_no_longer_the_engines():
    """``PosteriorPaths`` over a stand-in GP: the engine holds ONE set, and an older handle raises instead of evaluating another set."""
    from types import SimpleNamespace

    from gumbi_amd.regression.hip_gp import PosteriorPaths

    calls = []
    eng = SimpleNamespace(paths_generation=3, paths_eval_own=lambda P, draw, grad=True: (calls.append(len(P)) or np.zeros(len(P)), np.zeros((len(P), 2))))
    gp = SimpleNamespace(engine=eng)
    paths = PosteriorPaths(gp, ["y"], ["a", "b"], [0, 1], lambda Z: Z, 4, 3)
    val, grad = paths.value_and_grad(np.zeros((5, 2)), np.zeros(5, int))
    assert val.shape == (5,) and grad.shape == (5, 2) and calls == [5]
    eng.paths_generation = 4  # another draw_paths, a propose_thompson or paths_clear
    for call in (lambda: paths.value_and_grad(np.zeros((5, 2)), np.zeros(5, int)), lambda: paths.at_points(None), paths.on_grid):
        with pytest.raises(ValueError, match="stale"):
            call()
    eng.paths_generation = 3
    gp.engine = SimpleNamespace(paths_generation=3)  # a rebuilt engine, whatever its counter says
    with pytest.raises(ValueError, match="stale"):
        paths.value_and_grad(np.zeros((5, 2)), np.zeros(5, int))
    assert calls == [5]


# ---- 6. recorded, not bounded ----------------------------------------------------------------------------------------------------------
def test_variance_of_the_draws_is_printed_not_bounded():
    spec, theta, X, y = table(100, 2, "Matern52")
    S, F = 4096, 4096
    omega, phase, w, eps = pathwise.path_inputs("Matern52", S, F, 2, len(y), seed=11)
    A = PR.coefficients(spec, theta, X, y, omega, phase, w, eps)
    Xs = points(X, 8, [0, 1], seed=2)
    Y = PR.all_draws(spec, theta, X, Xs, omega, phase, w, A)
    var = O.predict(spec, theta, X, y, Xs, with_noise=False, dist_mode="direct")[1]
    ratio = np.var(Y, axis=0) / var
    print(f"variance of {S} reference draws / exact posterior variance at 8 points (F = {F}): {ratio.min():.3f} .. {ratio.max():.3f}")
    assert Y.shape == (S, 8) and np.all(np.isfinite(ratio))
