"""gmb_evaluate keeps nothing from one call to the next (csrc/eval_plan.hpp), on the MI355X: one case per branch of
an evaluation's plan.  Needs a GPU (``-m gpu``).

Per case two engines on the same problem.  A is fresh and evaluates ``theta`` with the gradient.  B first builds a history that
takes every other way through gmb_evaluate and its neighbours -- ``set_theta(theta2)``, ``factorize``, ``nlml(grad)``,
``predict``; an ``evaluate`` that fails as not positive definite (a NaN coordinate, as in
``test_gpu_parity.test_not_positive_definite_raises_linalgerror``); an ``evaluate`` that is refused (a theta of the wrong
length); ``evaluate(theta, grad=False)`` -- and then evaluates ``theta`` with the gradient as well.  Whatever a call left behind
must not reach the next one:

* value and gradient of the two engines are equal in their bytes, and so are the means and variances of a ``predict`` at 64 points
  behind them;
* B's ``evaluate(theta, grad=False)`` returns A's value in its bytes;
* ``factor_is_current()`` after every step of B is what ``B_VALID`` lists, after every step of A what ``A_VALID`` lists, and the
  two agree behind the steps both take (the evaluation with the gradient, the prediction).

Only calls that exist since ABI version 16 are used and nothing new is assumed: the file pins what the engine did before the plan
became an argument as well.

    case  shape                              branch of the plan
    a     N = 100, d = 2, ARD                one block: inline prep, the tail merged into grad_finish_kernel
    b     N = 100, d = 2, one lengthscale    lands through eval_land_kernel
    c     N = 300, d = 3                     three block columns, the last ragged
    d     N = 200, additive, two terms       prezero through prep_points, no inline prep
    e     N = 4200, d = 2                    more than 4096 rows: no inline prep; 4096 columns or more: phase events
    f     case a with set_profiling(True)    phase events recorded on the light path
"""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

A_VALID = [("fresh", False), ("evaluate(theta)", True), ("predict", True)]
B_VALID = [("set_theta(theta2)", False), ("factorize", True), ("nlml(grad)", True), ("predict (theta2)", True),
           ("set_data(NaN)", False), ("evaluate: not positive definite", False), ("set_data", False),
           ("evaluate: refused", False), ("evaluate(theta, grad=False)", True), ("evaluate(theta)", True), ("predict", True)]


def plain(N, d, ard=True, seed=31):
    X, y, ls = O.synthetic_table(N, d, seed=seed)
    spec = O.make_spec(d, range(d), ard=ard)
    return spec, O.pack_theta(spec, ls if ard else [1.2], 1.0, 0.2), X, y


def additive(n):
    from test_oracle import additive_problem

    return additive_problem(n=n, two_outputs=False, lin=False, hetero=False)


CASES = {
    "a": (lambda: plain(100, 2), False),
    "b": (lambda: plain(100, 2, ard=False), False),
    "c": (lambda: plain(300, 3), False),
    "d": (lambda: additive(200), False),
    "e": (lambda: plain(4200, 2), False),
    "f": (lambda: plain(100, 2), True),
}


@functools.lru_cache(maxsize=None)
def run(case):
    """(A's steps, B's steps, results): [name, factor_is_current()] per step of either engine, and what the steps returned."""
    make, profiling = CASES[case]
    spec, theta, X, y = make()
    theta2 = theta * np.linspace(1.15, 0.9, len(theta))
    Xs = X[:64].copy()
    Xs[:, 0] += 0.17
    Xbad = X.copy()
    Xbad[len(X) // 2, 0] = np.nan
    out = {}

    def walk(eng, steps):
        seen = []
        for name, call in steps:
            res = call(eng)
            if res is not None:
                out[name] = res
            seen.append((name.split(": ", 1)[1], eng.factor_is_current()))
        return seen

    def raises(kind, call):
        def step(eng):
            with pytest.raises(kind):
                call(eng)
        return step

    with make_engine(spec, theta, X, y) as a, make_engine(spec, theta, X, y) as b:
        a.set_profiling(profiling)
        b.set_profiling(profiling)
        seen_a = walk(a, [("A: fresh", lambda e: None),
                          ("A: evaluate(theta)", lambda e: e.evaluate(theta)),
                          ("A: predict", lambda e: e.predict(Xs))])
        out["A: timings"] = a.timings()
        seen_b = walk(b, [("B: set_theta(theta2)", lambda e: e.set_theta(theta2)),
                          ("B: factorize", lambda e: e.factorize()),
                          ("B: nlml(grad)", lambda e: e.nlml(grad=True)),
                          ("B: predict (theta2)", lambda e: e.predict(Xs)),
                          ("B: set_data(NaN)", lambda e: e.set_data(Xbad, y)),
                          ("B: evaluate: not positive definite", raises(np.linalg.LinAlgError, lambda e: e.evaluate(theta))),
                          ("B: set_data", lambda e: e.set_data(X, y)),
                          ("B: evaluate: refused", raises(ValueError, lambda e: e.evaluate(theta[:-1]))),
                          ("B: evaluate(theta, grad=False)", lambda e: (e.evaluate(theta, grad=False),)),
                          ("B: evaluate(theta)", lambda e: e.evaluate(theta)),
                          ("B: predict", lambda e: e.predict(Xs))])
        out["B: timings"] = b.timings()
    return seen_a, seen_b, out


def same_bytes(x, y):
    return np.asarray(x, dtype=np.float64).tobytes() == np.asarray(y, dtype=np.float64).tobytes()


@pytest.mark.parametrize("case", sorted(CASES))
def test_an_evaluation_does_not_depend_on_the_calls_before_it(gpu, case):
    seen_a, seen_b, out = run(case)
    for who, seen in (("A", seen_a), ("B", seen_b)):
        for name, valid in seen:
            print(f"EVALPLAN {case} {who} {name:36s} current {valid}")
    assert seen_a == A_VALID
    assert seen_b == B_VALID
    assert dict(seen_a)["evaluate(theta)"] == dict(seen_b)["evaluate(theta)"] and dict(seen_a)["predict"] == dict(seen_b)["predict"]
    (val_a, g_a), (val_b, g_b) = out["A: evaluate(theta)"], out["B: evaluate(theta)"]
    print(f"EVALPLAN {case} nlml A {val_a!r} B {val_b!r} max |g_A - g_B| {np.max(np.abs(g_a - g_b)):.3e}")
    assert np.all(np.isfinite(g_a)) and np.isfinite(val_a)
    assert same_bytes(val_a, val_b) and same_bytes(g_a, g_b)
    assert same_bytes(out["B: evaluate(theta, grad=False)"][0], val_a)
    (mu_a, var_a), (mu_b, var_b) = out["A: predict"], out["B: predict"]
    assert mu_a.shape == (64,) and np.all(np.isfinite(mu_a)) and np.all(var_a > 0)
    assert same_bytes(mu_a, mu_b) and same_bytes(var_a, var_b)


@pytest.mark.parametrize("case,recorded", [("a", False), ("e", True), ("f", True)])
def test_phase_events_follow_the_plan(gpu, case, recorded):
    """Small light evaluations record no phase events (their timings read 0) unless profiling is on; from 4096 columns on they do --
    behind a fresh engine as behind a history (test_gpu_parity pins the same at N = 300)."""
    _, _, out = run(case)
    for who in ("A", "B"):
        tm = out[f"{who}: timings"]
        print(f"EVALPLAN {case} {who} kbuild_ms {tm['kbuild_ms']:.4f} chol_ms {tm['chol_ms']:.4f} grad_ms {tm['grad_ms']:.4f}")
        if recorded:
            assert tm["kbuild_ms"] > 0 and tm["chol_ms"] > 0 and tm["grad_ms"] > 0
        else:
            assert tm["kbuild_ms"] == 0 and tm["chol_ms"] == 0 and tm["grad_ms"] == 0
