"""The walk over an additive model's covariance terms (csrc/term_walk.hpp, engine.hip: walk_terms) on the MI355X: every entry point
that re-prepares the resident training points term by term, run behind every other.  A walk that returns with a later term's
preparation in place -- or a term prepared from the wrong copy of its parameters -- shows in the NEXT call, so each call is run
twice, in two orders, and compared bit for bit with itself and against the oracle.  Needs a GPU (``-m gpu``).

Shapes: the two-term additive model of tests/test_oracle.py at N = 300 (three block columns, the last ragged; categorical table,
output table, linear part and hetero noise all live) with M = 75 test points (one ragged tile); the single-term control is
Matern52, d = 3, at the same N and M.  ``additive_periodic`` is the additive model as ``<kind>+Periodic`` (mode 1: twice the prepared
columns), against tests/periodic_reference.py.

Bars, each copied from the existing additive test of that call:

* ``predict``: mean 1e-8 relative, variance 1e-9 absolute (test_gpu_parity.py::test_additive_model_matches_oracle);
* ``predict_grad``, and ``predict_with_grad``'s ``dmean`` / ``dvar``: ``1e-8 max|G_ref|`` absolute; ``predict_with_grad``'s mean
  and variance against ``predict``: 1e-10 relative (test_gpu_predict_grad.py, test_gpu_var_grad.py);
* ``predict_joint``: covariance 1e-9 absolute, mean 1e-8 relative; ``draw_joint`` (``with_noise=True``, ``jitter=0``: the
  well-conditioned form): 1e-8 of max|Y_ref| (test_gpu_joint.py);
* NLML 1e-10 relative, its gradient ``1e-8 max(1, |g|_inf)`` (test_gpu_parity.py, test_gpu_append.py);
* a repeated call: bit-identical.
"""
import functools

import numpy as np
import pytest

import grad_reference as GR
import var_grad_reference as VR
from oracle import gp_oracle as O
from test_gpu_parity import make_engine, rel

pytestmark = pytest.mark.gpu

K_APPEND = 30
PERIODS = {"additive_periodic": (3.0, 2.6)}  # case -> periods of its two continuous dimensions (mode 1)


@functools.lru_cache(maxsize=None)
def problem(case):
    """(spec, theta, X, y, Xs, Z): N = 300 observations, M = 75 test points off every fourth of them, three rows of normals."""
    if case.startswith("additive"):
        from test_oracle import additive_problem

        spec, theta, X, y = additive_problem(n=150, two_outputs=True, lin=True, hetero=True)
    else:
        from test_gpu_predict_grad import table

        spec, theta, X, y = table(300, 3, "Matern52")
    Xs = X[::4].copy()
    Xs[:, 0] += 0.17
    return spec, theta, X, y, Xs, np.random.default_rng(6).standard_normal((3, len(Xs)))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The oracle's result of every call of ``prediction_calls``, and the NLML with its gradient."""
    from test_joint_cpu import JointOracleEngine

    spec, theta, X, y, Xs, Z = problem(case)
    if case in PERIODS:
        from periodic_reference import Warped

        w, per = Warped(spec, 1, PERIODS[case]), dict(periodic=1, periods=PERIODS[case])
        ref = {"predict": w.predict(theta, X, y, Xs), "evaluate": w.nlml_and_grad(theta, X, y),
               "predict_joint": w.predict_joint(theta, X, y, Xs, with_noise=True, jitter=0.0)}
    else:
        per = {}
        joint = JointOracleEngine()
        joint.set_data(X, y)
        joint.spec = spec
        joint.set_theta(theta)
        ref = {"predict": O.predict(spec, theta, X, y, Xs, with_noise=True, dist_mode="direct"),
               "evaluate": O.nlml_and_grad(spec, theta, X, y, dist_mode="direct"),
               "predict_joint": joint.predict_joint(Xs, with_noise=True, jitter=0.0)}
    ref["predict_grad"] = GR.mean_grad(spec, theta, X, y, Xs, **per)
    ref["predict_with_grad"] = VR.mean_var_grad(spec, theta, X, y, Xs, **per)
    mean, cov = ref["predict_joint"]
    ref["draw_joint"] = mean[None, :] + Z @ O.cholesky_lower(cov).T
    return ref


def engine_for(case, X, y):
    spec, theta = problem(case)[:2]
    if case in PERIODS:
        from test_gpu_periodic import make_engine as periodic_engine

        return periodic_engine(spec, 1, PERIODS[case], theta, X, y)
    return make_engine(spec, theta, X, y)


def prediction_calls(eng, Xs, Z):
    """The five prediction-type calls: none of them changes the factor, each walks the terms."""
    return [("predict", lambda: eng.predict(Xs)),
            ("predict_grad", lambda: (eng.predict_grad(Xs),)),
            ("predict_with_grad", lambda: eng.predict_with_grad(Xs)),
            ("predict_joint", lambda: eng.predict_joint(Xs, with_noise=True, jitter=0.0)),
            ("draw_joint", lambda: (eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0),))]


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def close_to(got, ref, what):
    scale, err = float(np.max(np.abs(ref))), float(np.max(np.abs(got - ref)))
    print(f"TERMWALK {what}: max |got - ref| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert got.shape == ref.shape
    return err / scale


def check_predictions(first, ref, what):
    mu, var = first["predict"]
    assert close_to(mu, ref["predict"][0], f"{what} predict mean") < 1e-8
    assert float(np.max(np.abs(var - ref["predict"][1]))) < 1e-9
    assert close_to(first["predict_grad"][0], ref["predict_grad"], f"{what} predict_grad") <= 1e-8
    mean, v, dmean, dvar = first["predict_with_grad"]
    assert close_to(dmean, ref["predict_with_grad"][2], f"{what} dmean") <= 1e-8
    assert close_to(dvar, ref["predict_with_grad"][3], f"{what} dvar") <= 1e-8
    assert rel(mean, mu) < 1e-10 and rel(v, var) < 1e-10
    jmean, cov = first["predict_joint"]
    assert float(np.max(np.abs(cov - ref["predict_joint"][1]))) <= 1e-9
    assert close_to(jmean, ref["predict_joint"][0], f"{what} joint mean") <= 1e-8
    assert close_to(first["draw_joint"][0], ref["draw_joint"], f"{what} draws") <= 1e-8


def check_evaluation(val, g, ref, what):
    val_r, g_r = ref
    err = float(np.max(np.abs(g - g_r)))
    print(f"TERMWALK {what}: nlml rel {abs(val - val_r) / abs(val_r):.2e}, max |g - g_ref| = {err:.3e}, |g_ref|_inf = {np.max(np.abs(g_r)):.3e}")
    assert abs(val - val_r) <= 1e-10 * abs(val_r)
    assert err < 1e-8 * max(1.0, float(np.max(np.abs(g_r))))


def forward_and_back(case):
    """(a): behind ``factorize`` the five calls once in order, then once more in the reverse order.  Returns both rounds."""
    spec, theta, X, y, Xs, Z = problem(case)
    with engine_for(case, X, y) as eng:
        eng.factorize()
        calls = prediction_calls(eng, Xs, Z)
        first = {name: call() for name, call in calls}
        second = {name: call() for name, call in reversed(calls)}
    return first, second


def every_entry_point(case):
    """(b): evaluations around a prediction, the separate gradient call behind a fresh factorisation, and an append of the last
    ``K_APPEND`` rows followed by a prediction and an evaluation.  Returns the named results in the order they were made."""
    spec, theta, X, y, Xs, _ = problem(case)
    out = {}
    with engine_for(case, X, y) as eng:
        out["evaluate 1"] = eng.evaluate(theta, grad=True)
        out["predict between"] = eng.predict(Xs)
        out["evaluate 2"] = eng.evaluate(theta, grad=True)
        eng.factorize()
        out["nlml"] = eng.nlml(grad=True)
    n = len(y) - K_APPEND
    with engine_for(case, X[:n], y[:n]) as eng:
        eng.factorize()
        eng.append(X[n:], y[n:])
        assert eng.N == len(y) and eng.factor_is_current()
        out["predict appended"] = eng.predict(Xs)
        out["evaluate appended"] = eng.evaluate(theta, grad=True)
    return out


@pytest.mark.parametrize("case", ["additive", "additive_periodic", "single_term"])  # (c): the single-term model is the control
def test_prediction_calls_do_not_disturb_each_other(gpu, case):
    first, second = forward_and_back(case)
    for name in first:
        assert same_bits(first[name], second[name]), f"{case}: {name} differs between its two runs"
    check_predictions(first, reference(case), case)


@pytest.mark.parametrize("case", ["additive", "additive_periodic"])
def test_every_entry_point_behind_every_other(gpu, case):
    out, ref = every_entry_point(case), reference(case)

    def check_predict(got, what):
        assert close_to(got[0], ref["predict"][0], f"{what} mean") < 1e-8
        assert float(np.max(np.abs(got[1] - ref["predict"][1]))) < 1e-9

    assert same_bits(out["evaluate 1"], out["evaluate 2"])
    check_evaluation(*out["evaluate 1"], ref["evaluate"], "evaluate")
    check_predict(out["predict between"], "predict between evaluations")
    check_evaluation(*out["nlml"], ref["evaluate"], "nlml(grad) behind factorize")
    check_predict(out["predict appended"], "predict behind append")
    check_evaluation(*out["evaluate appended"], ref["evaluate"], "evaluate behind append")
