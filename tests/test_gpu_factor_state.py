"""What the engine says about its resident factorisation (csrc/factor_state.hpp) along one fixed walk through the ABI, on the MI355X:
the tie between the hand-transcribed model of tools/factor_state_check.cpp and the engine itself.  Needs a GPU (``-m gpu``).

One engine -- Matern52, d = 3, N = 300 (three block columns, the last ragged: ``test_gpu_predict_grad.table``), M = 75 test points
-- is walked through every call that invalidates, consumes or restores something.  After EVERY step the walk records
``factor_is_current()`` and what ``copy_alpha()`` does (its error text, or which of the alphas seen so far it returned, compared
by their bytes); a step that predicts records ``timings()["predict_gemm_form"]``, a step that is refused its error text.
``EXPECTED`` holds those observations as literals, read off the engine's code: the walk must reproduce them line for line.  Only
calls of ABI version 16 are used, so the file runs unchanged on a build from before the header existed.

Two things the walk records on purpose although they look wrong (kept until a behaviour change says otherwise):
``copy_alpha`` hands back the PREVIOUS alpha after an invalidating call (``set_theta``, ``set_y``, ``set_dist_mode``); nothing
else does -- every other reader asks for a valid factorisation first.

Values against the oracle, each bar copied from the existing test of that call on this very problem
(tests/test_gpu_term_walk.py, ``single_term``, which cites their sources):

* ``predict``: mean 1e-8 relative, variance 1e-9 absolute (test_gpu_parity.py, test_gpu_append.py:61);
* ``predict_grad``: ``1e-8 max|G_ref|`` absolute (test_gpu_predict_grad.py);
* ``predict_joint``: covariance 1e-9 absolute, mean 1e-8 relative (test_gpu_joint.py);
* NLML 1e-10 relative, its gradient ``1e-8 max(1, |g|_inf)`` (test_gpu_parity.py, test_gpu_append.py:132);
* alpha against ``Sigma^-1 y``: 1e-8 relative (test_gpu_append.py:134);
* a repeated call, and a call whose inputs the steps in between left untouched: bit-identical.

``FACTORSTATE sha256`` in the output is the digest of every recorded array in walk order: equal before and after a change that
claims to leave the engine's results alone.
"""
import functools
import hashlib

import numpy as np
import pytest

import grad_reference as GR
from oracle import gp_oracle as O
from test_gpu_parity import make_engine, rel

pytestmark = pytest.mark.gpu

K_APPEND = 30
PERIODS = (3.0, 2.6, 3.4)

NO_FACTOR = "no valid factorisation: call gmb_factorize first"
NO_THETA = "gmb_set_theta has not been called"
NO_ALPHA = "gmb_copy_alpha: alpha exists only after a gradient evaluation (gmb_nlml with grad)"
DISTRIBUTED = " is not available on distributed engines (gmb_dist_*, capacity mode)"
ONE_DEVICE = DISTRIBUTED + ": factorise with gmb_factorize on one device"

# [step, factor_is_current() behind it, copy_alpha() behind it, what the step itself showed]
#   copy_alpha: its error text, or "alpha k" = the k-th distinct alpha of the walk;   a predicting step: "form 0" the triangular
#   solve, "form 1" the product with the resident inverse;   a refused step: its error text;   anything else: None
EXPECTED = [
    # ---- the default schedule: gmb_evaluate fuses the gradient into the factorisation's launch and leaves U and alpha --------
    ["ready", False, NO_ALPHA, None],
    ["predict refused", False, NO_ALPHA, "gmb_predict: " + NO_FACTOR],
    ["evaluate(theta, grad)", True, "alpha 1", None],
    ["predict", True, "alpha 1", "form 1"],
    ["predict again", True, "alpha 1", "form 1"],
    ["predict_joint", True, "alpha 1", "form 1"],
    ["set_theta(theta2)", False, "alpha 1", None],                      # (the previous theta's alpha)
    ["predict refused (theta2)", False, "alpha 1", "gmb_predict: " + NO_FACTOR],
    ["predict_joint refused (theta2)", False, "alpha 1", "gmb_predict_joint: " + NO_FACTOR],
    ["predict_grad refused (theta2)", False, "alpha 1", "gmb_predict_grad: " + NO_FACTOR],
    ["append K=0 (theta2)", False, "alpha 1", None],                    # (nothing to refuse: without a factor only the data grows)
    ["factorize", True, NO_ALPHA, None],
    ["predict (theta2)", True, NO_ALPHA, "form 0"],
    ["predict_grad (theta2)", True, NO_ALPHA, None],                     # (alpha by back substitution: not the gradient's)
    ["predict_grad again (theta2)", True, NO_ALPHA, None],
    ["nlml(grad)", True, "alpha 2", None],                               # (three block columns: the launch tree -- consume, restore)
    ["predict behind nlml(grad)", True, "alpha 2", "form 0"],
    ["predict_grad behind nlml(grad)", True, "alpha 2", None],
    # ---- the launch tree throughout -----------------------------------------------------------------------------------------
    ["tree: evaluate(theta, grad)", True, "alpha 3", None],
    ["tree: predict", True, "alpha 3", "form 0"],
    ["tree: predict again", True, "alpha 3", "form 0"],
    ["tree: set_theta(theta2)", False, "alpha 3", None],
    ["tree: predict refused", False, "alpha 3", "gmb_predict: " + NO_FACTOR],
    ["tree: factorize", True, NO_ALPHA, None],
    ["tree: predict (theta2)", True, NO_ALPHA, "form 0"],
    ["tree: predict_grad (theta2)", True, NO_ALPHA, None],
    ["tree: nlml(grad)", True, "alpha 2", None],                         # (the same factor, the same tree: the same bits as above)
    ["tree: predict behind nlml(grad)", True, "alpha 2", "form 0"],
    # ---- the tile tasks behind a finished factorisation: U and alpha stay, as behind the fused launch ------------------------
    ["tiles: evaluate(theta, grad)", True, "alpha 1", None],            # (the fused launch's tasks in two launches: the same bits)
    ["tiles: predict", True, "alpha 1", "form 1"],
    ["tiles: factorize", True, NO_ALPHA, None],
    ["tiles: predict behind factorize", True, NO_ALPHA, "form 0"],
    ["tiles: nlml(grad)", True, "alpha 1", None],
    ["tiles: predict behind nlml(grad)", True, "alpha 1", "form 1"],
    # ---- new observations ---------------------------------------------------------------------------------------------------
    ["set_y(y2)", False, "alpha 1", None],
    ["predict refused (y2)", False, "alpha 1", "gmb_predict: " + NO_FACTOR],
    ["factorize (y2)", True, NO_ALPHA, None],
    ["predict (y2)", True, NO_ALPHA, "form 0"],
    # ---- the periodic feature map on and off: theta goes with it ---------------------------------------------------------------
    ["evaluate(theta, grad) (y2)", True, "alpha 4", None],
    ["set_periodic on", False, "gmb_copy_alpha: " + NO_THETA, None],
    ["predict refused (periodic, no theta)", False, "gmb_copy_alpha: " + NO_THETA, "gmb_predict: " + NO_THETA],
    ["set_theta (periodic)", False, "alpha 4", None],
    ["predict refused (periodic)", False, "alpha 4", "gmb_predict: " + NO_FACTOR],
    ["evaluate(theta, grad) (periodic)", True, "alpha 5", None],
    ["predict (periodic)", True, "alpha 5", "form 1"],
    ["set_periodic off", False, "gmb_copy_alpha: " + NO_THETA, None],
    ["set_theta (periodic off)", False, "alpha 5", None],
    ["factorize (periodic off)", True, NO_ALPHA, None],
    ["predict (periodic off)", True, NO_ALPHA, "form 0"],
    # ---- append and truncate, behind a live factor and behind none -------------------------------------------------------------
    ["evaluate(theta, grad) before append", True, "alpha 4", None],     # (y2, theta, no period: as four steps above "set_periodic on")
    ["append(30) behind a live factor", True, NO_ALPHA, None],
    ["predict (330)", True, NO_ALPHA, "form 0"],
    ["truncate(300) behind a live factor", True, NO_ALPHA, None],
    ["predict (300 again)", True, NO_ALPHA, "form 0"],
    ["set_theta(theta2) before append", False, NO_ALPHA, None],
    ["append(30) behind no factor", False, NO_ALPHA, None],
    ["predict refused (330, no factor)", False, NO_ALPHA, "gmb_predict: " + NO_FACTOR],
    ["factorize (330, theta2)", True, NO_ALPHA, None],
    ["predict (330, theta2)", True, NO_ALPHA, "form 0"],
    ["set_theta(theta) before truncate", False, NO_ALPHA, None],
    ["truncate(300) behind no factor", False, NO_ALPHA, None],
    ["evaluate(theta, grad) (300 again)", True, "alpha 4", None],
    # ---- the multi-GPU driver's capacity mode and back: no communicator needed ----------------------------------------------------
    ["set_dist_mode(1)", False, "alpha 4", None],
    ["predict refused (capacity mode)", False, "alpha 4", "gmb_predict: " + NO_FACTOR],
    ["append refused (capacity mode)", False, "alpha 4", "gmb_append: gmb_append" + DISTRIBUTED],
    ["factorize (capacity mode)", True, NO_ALPHA, None],
    ["predict (capacity mode)", True, NO_ALPHA, "form 0"],
    ["predict_grad refused (capacity mode)", True, NO_ALPHA, "gmb_predict_grad: gmb_predict_grad" + ONE_DEVICE],
    ["predict_joint refused (capacity mode)", True, NO_ALPHA, "gmb_predict_joint: gmb_predict_joint" + ONE_DEVICE],
    ["set_dist_mode(0)", False, NO_ALPHA, None],
    ["predict refused (replicated mode)", False, NO_ALPHA, "gmb_predict: " + NO_FACTOR],
    ["factorize (replicated mode)", True, NO_ALPHA, None],
    ["predict_grad (replicated mode)", True, NO_ALPHA, None],
    # ---- the debug door stays shut --------------------------------------------------------------------------------------------
    ["debug door refused", True, NO_ALPHA,
     "gmb_debug_assume_factored: gmb_debug_assume_factored needs GUMBI_HIP_DEBUG_DOORS=1 in the environment"],
]


@functools.lru_cache(maxsize=None)
def problem():
    from test_gpu_predict_grad import table

    spec, theta, X, y = table(300, 3, "Matern52")
    _, _, Xmore, ymore = table(300 + K_APPEND, 3, "Matern52")
    theta2 = theta * np.linspace(1.15, 0.9, len(theta))
    y2 = y[::-1].copy()
    Xs = X[::4].copy()
    Xs[:, 0] += 0.17
    return dict(spec=spec, theta=theta, theta2=theta2, X=X, y=y, y2=y2, Xa=Xmore[300:], ya=ymore[300:], Xs=Xs)


@functools.lru_cache(maxsize=None)
def walk():
    """(observations, arrays): the rows of ``EXPECTED`` as the engine produced them, and every array a step returned, by step."""
    import os

    p = problem()
    theta, theta2, Xs = p["theta"], p["theta2"], p["Xs"]
    obs, arrays, alphas = [], {}, []
    door = os.environ.pop("GUMBI_HIP_DEBUG_DOORS", None)  # (the engine reads the environment at the call)

    with make_engine(p["spec"], theta, p["X"], p["y"]) as eng:
        def alpha_behind():
            try:
                a = eng.copy_alpha()
            except ValueError as err:
                return str(err)
            if a.tobytes() not in alphas:
                alphas.append(a.tobytes())
                arrays[f"alpha {len(alphas)}"] = (a,)
            return f"alpha {alphas.index(a.tobytes()) + 1}"

        def step(name, call=None, predicts=False):
            seen = None
            if call is not None:
                try:
                    res = call()
                except ValueError as err:
                    seen = str(err)
                else:
                    if predicts:
                        seen = f"form {eng.timings()['predict_gemm_form']}"
                    if res is not None:
                        arrays[name] = tuple(np.asarray(r) for r in res) if isinstance(res, tuple) else (np.asarray(res),)
            obs.append([name, eng.factor_is_current(), alpha_behind(), seen])

        def predict(name):
            step(name, lambda: eng.predict(Xs), predicts=True)

        step("ready")
        predict("predict refused")
        step("evaluate(theta, grad)", lambda: eng.evaluate(theta, grad=True))
        predict("predict")
        predict("predict again")
        step("predict_joint", lambda: eng.predict_joint(Xs, with_noise=True, jitter=0.0), predicts=True)
        step("set_theta(theta2)", lambda: eng.set_theta(theta2))
        predict("predict refused (theta2)")
        step("predict_joint refused (theta2)", lambda: eng.predict_joint(Xs))
        step("predict_grad refused (theta2)", lambda: eng.predict_grad(Xs))
        step("append K=0 (theta2)", lambda: eng.append(np.empty((0, 3)), np.empty(0)))
        step("factorize", eng.factorize)
        predict("predict (theta2)")
        step("predict_grad (theta2)", lambda: eng.predict_grad(Xs))
        step("predict_grad again (theta2)", lambda: eng.predict_grad(Xs))
        step("nlml(grad)", lambda: eng.nlml(grad=True))
        predict("predict behind nlml(grad)")
        step("predict_grad behind nlml(grad)", lambda: eng.predict_grad(Xs))

        assert eng.set_grad_scheme(eng.GRAD_LAUNCH_TREE) == eng.GRAD_BY_SIZE
        step("tree: evaluate(theta, grad)", lambda: eng.evaluate(theta, grad=True))
        predict("tree: predict")
        predict("tree: predict again")
        step("tree: set_theta(theta2)", lambda: eng.set_theta(theta2))
        predict("tree: predict refused")
        step("tree: factorize", eng.factorize)
        predict("tree: predict (theta2)")
        step("tree: predict_grad (theta2)", lambda: eng.predict_grad(Xs))
        step("tree: nlml(grad)", lambda: eng.nlml(grad=True))
        predict("tree: predict behind nlml(grad)")

        eng.set_grad_scheme(eng.GRAD_TILES)
        step("tiles: evaluate(theta, grad)", lambda: eng.evaluate(theta, grad=True))
        predict("tiles: predict")
        step("tiles: factorize", eng.factorize)
        predict("tiles: predict behind factorize")
        step("tiles: nlml(grad)", lambda: eng.nlml(grad=True))
        predict("tiles: predict behind nlml(grad)")
        eng.set_grad_scheme(eng.GRAD_BY_SIZE)

        step("set_y(y2)", lambda: eng.set_y(p["y2"]))
        predict("predict refused (y2)")
        step("factorize (y2)", eng.factorize)
        predict("predict (y2)")

        step("evaluate(theta, grad) (y2)", lambda: eng.evaluate(theta, grad=True))
        step("set_periodic on", lambda: eng.set_periodic(1, PERIODS))
        predict("predict refused (periodic, no theta)")
        step("set_theta (periodic)", lambda: eng.set_theta(theta))
        predict("predict refused (periodic)")
        step("evaluate(theta, grad) (periodic)", lambda: eng.evaluate(theta, grad=True))
        predict("predict (periodic)")
        step("set_periodic off", lambda: eng.set_periodic(0, np.zeros(3)))
        step("set_theta (periodic off)", lambda: eng.set_theta(theta))
        step("factorize (periodic off)", eng.factorize)
        predict("predict (periodic off)")

        step("evaluate(theta, grad) before append", lambda: eng.evaluate(theta, grad=True))
        step("append(30) behind a live factor", lambda: eng.append(p["Xa"], p["ya"]))
        predict("predict (330)")
        step("truncate(300) behind a live factor", lambda: eng.truncate(300))
        predict("predict (300 again)")
        step("set_theta(theta2) before append", lambda: eng.set_theta(theta2))
        step("append(30) behind no factor", lambda: eng.append(p["Xa"], p["ya"]))
        predict("predict refused (330, no factor)")
        step("factorize (330, theta2)", eng.factorize)
        predict("predict (330, theta2)")
        step("set_theta(theta) before truncate", lambda: eng.set_theta(theta))
        step("truncate(300) behind no factor", lambda: eng.truncate(300))
        step("evaluate(theta, grad) (300 again)", lambda: eng.evaluate(theta, grad=True))

        def dist_mode(mode):
            assert eng.set_dist_mode(mode) == 1 - mode  # (the previous mode)

        step("set_dist_mode(1)", lambda: dist_mode(1))
        predict("predict refused (capacity mode)")
        step("append refused (capacity mode)", lambda: eng.append(np.empty((0, 3)), np.empty(0)))
        step("factorize (capacity mode)", eng.factorize)
        predict("predict (capacity mode)")
        step("predict_grad refused (capacity mode)", lambda: eng.predict_grad(Xs))
        step("predict_joint refused (capacity mode)", lambda: eng.predict_joint(Xs))
        step("set_dist_mode(0)", lambda: dist_mode(0))
        predict("predict refused (replicated mode)")
        step("factorize (replicated mode)", eng.factorize)
        step("predict_grad (replicated mode)", lambda: eng.predict_grad(Xs))

        step("debug door refused", eng.debug_assume_factored)
    if door is not None:
        os.environ["GUMBI_HIP_DEBUG_DOORS"] = door

    digest = hashlib.sha256()
    for name, arrs in arrays.items():
        for a in arrs:
            digest.update(np.ascontiguousarray(a).tobytes())
    print(f"FACTORSTATE sha256 of {sum(len(a) for a in arrays.values())} arrays: {digest.hexdigest()}")
    return obs, arrays


@functools.lru_cache(maxsize=None)
def reference():
    """The oracle at every (rows, observations, theta, feature map) the walk predicts or evaluates at."""
    from periodic_reference import Warped
    from test_joint_cpu import JointOracleEngine

    p = problem()
    spec, theta, theta2, X, y, y2, Xs = (p[k] for k in ("spec", "theta", "theta2", "X", "y", "y2", "Xs"))
    X330, y330 = np.vstack([X, p["Xa"]]), np.concatenate([y2, p["ya"]])

    def predict(th, Xt, yt):
        return O.predict(spec, th, Xt, yt, Xs, with_noise=True, dist_mode="direct")

    def evaluate(th, yt):
        return O.nlml_and_grad(spec, th, X, yt, dist_mode="direct")

    def alpha(th, yt):
        return np.linalg.solve(O.sigma_matrix(spec, th, X, dist_mode="direct"), yt)

    joint = JointOracleEngine()
    joint.set_data(X, y)
    joint.spec = spec
    joint.set_theta(theta)
    w = Warped(spec, 1, PERIODS)
    return {
        "predict": {"theta": predict(theta, X, y), "theta2": predict(theta2, X, y), "y2": predict(theta, X, y2),
                    "330": predict(theta, X330, y330), "330 theta2": predict(theta2, X330, y330),
                    "periodic": w.predict(theta, X, y2, Xs)},
        "evaluate": {"theta": evaluate(theta, y), "theta2": evaluate(theta2, y), "y2": evaluate(theta, y2),
                     "periodic": w.nlml_and_grad(theta, X, y2)},
        "alpha": {"theta": alpha(theta, y), "theta2": alpha(theta2, y), "y2": alpha(theta, y2)},
        "predict_grad": {"theta2": GR.mean_grad(spec, theta2, X, y, Xs), "y2": GR.mean_grad(spec, theta, X, y2, Xs)},
        "predict_joint": joint.predict_joint(Xs, with_noise=True, jitter=0.0),
    }


# which reference every value-returning step answers to
PREDICTS = {
    "theta": ["predict", "predict again", "tree: predict", "tree: predict again", "tiles: predict", "tiles: predict behind factorize",
              "tiles: predict behind nlml(grad)"],
    "theta2": ["predict (theta2)", "predict behind nlml(grad)", "tree: predict (theta2)", "tree: predict behind nlml(grad)"],
    "y2": ["predict (y2)", "predict (periodic off)", "predict (300 again)", "predict (capacity mode)"],
    "330": ["predict (330)"],
    "330 theta2": ["predict (330, theta2)"],
    "periodic": ["predict (periodic)"],
}
EVALUATES = {
    "theta": ["evaluate(theta, grad)", "tree: evaluate(theta, grad)", "tiles: evaluate(theta, grad)", "tiles: nlml(grad)"],
    "theta2": ["nlml(grad)", "tree: nlml(grad)"],
    "y2": ["evaluate(theta, grad) (y2)", "evaluate(theta, grad) before append", "evaluate(theta, grad) (300 again)"],
    "periodic": ["evaluate(theta, grad) (periodic)"],
}
PREDICT_GRADS = {
    "theta2": ["predict_grad (theta2)", "predict_grad again (theta2)", "predict_grad behind nlml(grad)", "tree: predict_grad (theta2)"],
    "y2": ["predict_grad (replicated mode)"],
}
ALPHAS = {"alpha 1": "theta", "alpha 2": "theta2", "alpha 3": "theta", "alpha 4": "y2"}  # (alpha 5: the periodic model's)
# steps that must return the very bits of an earlier step: the calls in between touched nothing these read
SAME_BITS = [
    ("predict", "predict again"),                                        # L^-1 was transposed by the first, reused by the second
    ("predict_grad (theta2)", "predict_grad again (theta2)"),            # alpha back-substituted by the first, reused by the second
    ("predict (theta2)", "predict behind nlml(grad)"),                   # the launch tree put the factor's diagonal blocks back
    ("tree: predict", "tree: predict again"),
    ("predict (theta2)", "tree: predict (theta2)"),                      # gmb_factorize does not depend on the gradient's schedule
    ("predict_grad (theta2)", "tree: predict_grad (theta2)"),
    ("nlml(grad)", "tree: nlml(grad)"),                                  # three block columns: the launch tree either way
    ("predict (theta2)", "tree: predict behind nlml(grad)"),
    ("tree: predict", "tiles: predict behind factorize"),                # gmb_factorize and the unfused gmb_evaluate: one Cholesky
    ("predict", "tiles: predict"),                                       # the fused launch's tasks in two launches: the same bits
    ("predict", "tiles: predict behind nlml(grad)"),
    ("evaluate(theta, grad) (y2)", "evaluate(theta, grad) before append"),
    ("evaluate(theta, grad) (y2)", "evaluate(theta, grad) (300 again)"),  # append, truncate and two factorisations later
    ("predict (y2)", "predict (periodic off)"),
    ("predict (y2)", "predict (capacity mode)"),
]


def test_walk_shows_what_the_code_says(gpu):
    obs, _ = walk()
    for got, want in zip(obs, EXPECTED):
        print(f"FACTORSTATE {got[0]:40s} current {got[1]!s:5s} {got[2][:40]:40s} {got[3]}")
    assert [o[0] for o in obs] == [w[0] for w in EXPECTED]
    wrong = [(got, want) for got, want in zip(obs, EXPECTED) if got != want]
    assert not wrong, wrong


def test_walk_values_match_the_oracle(gpu):
    _, arrays = walk()
    ref = reference()
    for key, steps in PREDICTS.items():
        mu_r, var_r = ref["predict"][key]
        for s in steps:
            mu, var = arrays[s]
            e_m, e_v = rel(mu, mu_r), float(np.max(np.abs(var - var_r)))
            print(f"FACTORSTATE {s}: mean rel {e_m:.2e} var abs {e_v:.2e}")
            assert e_m < 1e-8 and e_v < 1e-9, s
    for key, steps in EVALUATES.items():
        val_r, g_r = ref["evaluate"][key]
        for s in steps:
            val, g = float(arrays[s][0]), arrays[s][1]
            e_g = float(np.max(np.abs(g - g_r)))
            print(f"FACTORSTATE {s}: nlml rel {abs(val - val_r) / abs(val_r):.2e} max |g - g_ref| {e_g:.2e} of {np.max(np.abs(g_r)):.2e}")
            assert abs(val - val_r) <= 1e-10 * abs(val_r), s
            assert e_g <= 1e-8 * max(1.0, float(np.max(np.abs(g_r)))), s
    for key, steps in PREDICT_GRADS.items():
        G_r = ref["predict_grad"][key]
        for s in steps:
            e = float(np.max(np.abs(arrays[s][0] - G_r)))
            print(f"FACTORSTATE {s}: max |G - G_ref| {e:.2e} of {np.max(np.abs(G_r)):.2e}")
            assert e <= 1e-8 * float(np.max(np.abs(G_r))), s
    for name, key in ALPHAS.items():
        e = rel(arrays[name][0], ref["alpha"][key])
        print(f"FACTORSTATE {name} ({key}): rel {e:.2e}")
        assert e <= 1e-8, name
    mean, cov = arrays["predict_joint"]
    mean_r, cov_r = ref["predict_joint"]
    assert float(np.max(np.abs(cov - cov_r))) <= 1e-9 and rel(mean, mean_r) <= 1e-8


def test_untouched_inputs_give_the_same_bits(gpu):
    _, arrays = walk()
    for a, b in SAME_BITS:
        assert len(arrays[a]) == len(arrays[b])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(arrays[a], arrays[b])), f"{b!r} differs from {a!r}"
