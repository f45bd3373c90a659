"""GP classification by the Laplace approximation (csrc/laplace.hpp) against an extended-precision reference -- runs on the MI355X
box only (``-m gpu``).

The problems are tests/laplace_reference.py's, test points M in {1, 129, 200}.  The engine and the float64 host restatement
(LAPACK, the engine's stop rule) are each compared with the longdouble reference; for every problem and quantity the engine's
error may be at most

    max(8 x the host's error, floor)

(the standing rule of tests/test_gpu_fitc.py) with the floors: the objective 1e-10 of max(1, |nlq|), every gradient entry 1e-8 of
max |grad|, the mode and the latent mean 1e-8 of their maximum, the latent variance 1e-9 absolute.  Every comparison prints
``LAPLACE <problem> <quantity> <engine error> <host error> <ratio>``; tests/golden/make_laplace_ratios.py turns a log of them into
tests/golden/laplace_ratios.json, the record behind DESIGN 3.18's table (the bars do not read it).

Then: the Newton iteration's length against the host's, the same bits call after call and around exact calls on the same engine,
the state rules of ``gmb_laplace_predict`` and of the exact path behind a Laplace call, the errors, the padding rows, and the front
end (``gumbi_amd.GPC``).
"""
import numpy as np
import pytest

import laplace_reference as L
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NAMES = list(L.PROBLEMS)
K = 8.0
FLOOR = {"nlq": 1e-10, "grad": 1e-8, "f": 1e-8, "mean": 1e-8, "var": 1e-9}


def kernel_spec(spec, **over):
    from gumbi_amd.engine import KernelSpec

    kw = dict(D=spec["D"], idx_cont=spec["idx_cont"], kind=spec["kind"], ard=spec["ard"], idx_lin=spec["idx_lin"], coreg=spec["coreg"],
              jitter=spec["jitter"])
    kw.update(over)
    return KernelSpec(**kw)


def make_engine(name, y=None):
    from gumbi_amd.engine import Engine

    spec, theta, X, y0, _ = L.problem(name)
    eng = Engine(0)
    eng.set_data(X, y0 if y is None else y)
    eng.set_kernel(kernel_spec(spec))
    return eng


def scaled_errors(key, got, want):
    """the errors of one quantity in the units of its bar"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    scale = {"nlq": max(1.0, abs(float(want))) if key == "nlq" else 1.0, "grad": np.max(np.abs(want)), "f": np.max(np.abs(want)),
             "mean": np.max(np.abs(want))}.get(key, 1.0)
    return np.atleast_1d(np.abs(got - want)) / scale


class Bars:
    def __init__(self, name):
        self.name, self.ref, self.bad = name, L.references(name), []

    def check(self, key, got, rows=None, label=None):
        ref = self.ref[key] if rows is None else self.ref[key][:rows]
        host = self.ref["h_" + key] if rows is None else self.ref["h_" + key][:rows]
        err, e64 = scaled_errors(key, got, ref), scaled_errors(key, host, ref)
        if key != "grad":  # (the gradient entry by entry; every other quantity by its worst element, host and engine alike)
            err, e64 = np.array([err.max()]), np.array([e64.max()])
        bound = np.maximum(K * e64, FLOOR[key])
        label = label or key
        for j in range(err.size):
            tag = f"{label}[{j}]" if key == "grad" else label
            print(f"LAPLACE {self.name} {tag} {err[j]:.3e} {e64[j]:.3e} {err[j] / max(e64[j], 1e-300):.4g}")
            if not err[j] <= bound[j]:
                self.bad.append(f"{tag}: {err[j]:.3e} > {bound[j]:.3e} = max(8 x host {e64[j]:.2e}, floor {FLOOR[key]:.0e})")

    def done(self):
        assert not self.bad, f"{self.name}: " + "; ".join(self.bad)


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_engine_within_8x_of_the_float64_host(gpu, name):
    spec, theta, X, y, Xs = L.problem(name)
    bars = Bars(name)
    with make_engine(name) as eng:
        nlq, grad = eng.laplace_evaluate(theta, grad=True)
        info = eng.laplace_info()
        bars.check("nlq", nlq)
        bars.check("grad", grad)
        bars.check("f", eng.laplace_mode()[0])
        for M in L.TEST_POINTS:
            mean, var = eng.laplace_predict(Xs[:M])
            bars.check("mean", mean, rows=M, label=f"mean(M={M})")
            bars.check("var", var, rows=M, label=f"var(M={M})")
        assert eng.notpd_index() == -1
    print(f"LAPLACE-ITER {name} {info['iterations']} {bars.ref['h_iterations']} {info['halvings']} {bars.ref['h_halvings']}")
    # the Newton iteration is the host restatement's: the same count, give or take one, and as far from the caps
    assert abs(info["iterations"] - bars.ref["h_iterations"]) <= 1 and info["halvings"] <= 1
    bars.done()


# ---- the same bits, and the two paths on one engine -------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["N129", "coreg"])
def test_repeated_calls_give_the_same_bits_also_around_exact_calls(gpu, name):
    spec, theta, X, y, Xs = L.problem(name)
    th_exact = theta.copy()
    th_exact[np.flatnonzero(theta == 0.0)[0]] = 0.3  # (sigma, for the exact path)
    with make_engine(name) as eng, make_engine(name) as fresh:
        v0, g0 = eng.laplace_evaluate(theta, grad=True)
        p0 = eng.laplace_predict(Xs)
        m0 = eng.laplace_mode()
        v1 = eng.laplace_evaluate(theta, grad=False)  # grad = NULL: the objective of the call with a gradient
        p1 = eng.laplace_predict(Xs)
        v2, g2 = eng.laplace_evaluate(theta * 1.01, grad=True)  # (no warm start: what came before does not matter)
        # an exact evaluation and prediction behind the Laplace calls: the bits of an engine that never saw them
        ex = eng.evaluate(th_exact)
        ex_p = eng.predict(Xs)
        fx = fresh.evaluate(th_exact)
        fx_p = fresh.predict(Xs)
        v3, g3 = eng.laplace_evaluate(theta, grad=True)
        p3 = eng.laplace_predict(Xs)
        m3 = eng.laplace_mode()
    assert bits(v0) == bits(v1) == bits(v3) and v2 != v0
    assert np.array_equal(bits(g0), bits(g3)) and not np.array_equal(g0, g2)
    for a, b, c in zip(p0 + m0, p1 + m0, p3 + m3):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    assert bits(ex[0]) == bits(fx[0]) and np.array_equal(bits(ex[1]), bits(fx[1]))
    assert np.array_equal(bits(ex_p[0]), bits(fx_p[0])) and np.array_equal(bits(ex_p[1]), bits(fx_p[1]))


def test_state_rules_between_the_laplace_and_the_exact_path(gpu):
    name = "N129"
    spec, theta, X, y, Xs = L.problem(name)
    th_exact = theta.copy()
    th_exact[np.flatnonzero(theta == 0.0)[0]] = 0.3  # (sigma, for the exact path)
    with make_engine(name) as eng, make_engine(name) as fresh:
        with pytest.raises(ValueError, match="no gmb_laplace_evaluate"):
            eng.laplace_predict(Xs)
        eng.laplace_evaluate(theta, grad=True)
        want = eng.laplace_predict(Xs)
        # B's factor sits in the factor buffer: the exact path is "not factored" and refuses instead of reading it as Sigma's
        assert not eng.factor_is_current()
        with pytest.raises(ValueError, match="factor"):
            eng.predict(Xs)
        with pytest.raises(ValueError):
            eng.nlml()
        eng.factorize()  # (theta is the Laplace call's: sigma = 0, Sigma = K + jitter I)
        fresh.set_theta(theta)
        fresh.factorize()
        for a, b in zip(eng.predict(Xs), fresh.predict(Xs)):
            assert np.array_equal(bits(a), bits(b))
        with pytest.raises(ValueError, match="factorisation of Sigma"):
            eng.laplace_predict(Xs)
        # everything that changes theta, the labels or the data takes the Laplace state away, and says so
        for change, text in ((lambda: eng.set_theta(theta), "theta was set"), (lambda: eng.set_y(y), "gmb_set_y"),
                             (lambda: eng.append(X[:3] + 0.01, y[:3]), "gmb_append"), (lambda: eng.evaluate(th_exact), "theta was set|factorisation")):
            eng.truncate(len(X)) if eng.N != len(X) else None
            eng.laplace_evaluate(theta, grad=False)
            got = eng.laplace_predict(Xs)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
            change()
            with pytest.raises(ValueError, match=text):
                eng.laplace_predict(Xs)
            with pytest.raises(ValueError):
                eng.laplace_mode()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", [0.5, 2.0])
def test_labels_other_than_0_and_1_are_refused(gpu, label):
    spec, theta, X, y, Xs = L.problem("N129")
    bad = y.copy()
    bad[128] = label  # (the one live row of the second tile)
    with make_engine("N129", y=bad) as eng:
        with pytest.raises(ValueError, match="exactly 0 or 1; 1 of 129"):
            eng.laplace_evaluate(theta)
        with pytest.raises(ValueError):
            eng.laplace_predict(Xs)
        eng.set_y(y)
        assert abs(eng.laplace_evaluate(theta, grad=False) - L.references("N129")["nlq"]) < 1e-8


def test_an_iteration_cap_is_an_error_of_its_own_and_the_engine_stays_usable(gpu):
    from gumbi_amd.engine import LaplaceConvergenceError

    spec, theta, X, y, Xs = L.problem("separated")
    with make_engine("separated") as eng:
        eng.set_laplace_options(max_iter=2)
        with pytest.raises(LaplaceConvergenceError, match="no convergence in 2 Newton iterations"):
            eng.laplace_evaluate(theta)
        assert eng.laplace_info()["iterations"] == 2
        with pytest.raises(ValueError, match="failed"):
            eng.laplace_predict(Xs)
        for bad in (dict(tol=0.0), dict(max_iter=0), dict(max_iter=41)):
            with pytest.raises(ValueError):
                eng.set_laplace_options(**bad)
        eng.set_laplace_options()
        nlq = eng.laplace_evaluate(theta, grad=False)
        assert abs(nlq - L.references("separated")["nlq"]) < 1e-8
        th = theta.copy()
        th[2] = 0.2
        assert np.isfinite(eng.evaluate(th)[0])  # ... by the exact path too


def test_models_outside_the_scope_are_refused(gpu):
    from gumbi_amd.engine import Engine

    spec, theta, X, y, Xs = L.problem("coreg")
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(kernel_spec(spec, additive=True))
        add = np.concatenate([theta, [1.0, 1.5, 1.0]])  # (+ ls | eta of the categorical dimension's own kernel)
        with pytest.raises(ValueError, match="additive"):
            eng.laplace_evaluate(add)
    spec, theta, X, y, Xs = L.problem("N100")
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(kernel_spec(spec, kind="ExpQuad", periodic=2, periods=[3.0, 3.0]))
        with pytest.raises(ValueError, match="periodic"):
            eng.laplace_evaluate(theta)
    Xo = np.column_stack([X, np.arange(len(X)) % 2]).astype(float)
    with Engine(0) as eng:
        eng.set_data(Xo, y)
        eng.set_kernel(kernel_spec(spec, D=3, out_col=2, n_out=2))
        with pytest.raises(ValueError, match="one output"):
            eng.laplace_evaluate(np.ones(eng.spec.theta_size()))


# ---- padding ----------------------------------------------------------------------------------------------------------------------------
def test_padding_rows_are_exactly_zero(gpu):
    """N = 129: 127 padding rows in the second tile.  The mode, a^ and every output of the symmetric product are 0 there, and the
    product is Sigma v on the live rows."""
    spec, theta, X, y, Xs = L.problem("N129")
    S = O.sigma_matrix(spec, theta, X, dist_mode="direct")
    with make_engine("N129") as eng:
        eng.laplace_evaluate(theta)
        f, a = eng.laplace_mode(padded=True)
        assert f.shape == a.shape == (256,)
        assert np.all(bits(f[129:]) == 0) and np.all(bits(a[129:]) == 0) and np.all(f[:129] != 0)
        rng = np.random.default_rng(5)
        for v in (np.ones(129), rng.standard_normal(129), np.eye(129)[128]):
            out = eng.debug_laplace_symv(v)
            assert out.shape == (256,) and np.all(bits(out[129:]) == 0)
            assert np.max(np.abs(out[:129] - S @ v)) <= 1e-12 * np.max(np.abs(S)) * np.sum(np.abs(v))
        assert np.max(np.abs(eng.debug_laplace_symv(a[:129])[:129] - f[:129])) <= 1e-12 * np.max(np.abs(f))


# ---- the front end -----------------------------------------------------------------------------------------------------------------------
def _table(N=300, seed=4):
    import pandas as pd

    rng = np.random.default_rng(seed)
    x0, x1 = rng.uniform(-2, 2, N), rng.uniform(0, 5, N)
    p = 1.0 / (1.0 + np.exp(-(1.5 * np.sin(1.5 * x0) + 0.6 * (x1 - 2.5))))
    return pd.DataFrame({"x0": x0, "x1": x1, "y": (rng.random(N) < p).astype(float)})


def test_front_end_fit_and_predictions(gpu):
    import gumbi_amd as gmb
    from gumbi_amd.regression.gpc import averaged_sigmoid

    df = _table()
    ds = gmb.DataSet(df, outputs=["y"])
    gp = gmb.GPC(ds, outputs=["y"]).fit(continuous_dims=["x0", "x1"])
    assert gp.MAP["σ"] == 0.0 and gp.model.y.tolist() == df["y"].tolist()  # the labels went to the engine as they are
    # the objective at the MAP is below the objective at the start
    pos = gp._positive_mask()
    to_u = lambda th: np.where(pos, np.log(np.where(pos, np.maximum(th, 1e-300), 1.0)), th)  # noqa: E731
    start = gp._initial_theta()
    f_start = gp._objective(to_u(start), pos)[0]
    th = gp._theta_fitted.copy()
    u_map = to_u(np.where(np.arange(th.size) == gp._sigma_slice().start, 1.0, th))
    f_map = gp._objective(u_map, pos)[0]
    assert f_map < f_start - 1.0
    info = gp.laplace_info
    assert 1 <= info["iterations"] <= 14 and info["halvings"] <= 1
    # at the fitted theta: the latent predictions and the probabilities are the float64 host restatement's
    pts = gp.parray(x0=df["x0"].to_numpy()[:150], x1=df["x1"].to_numpy()[:150])
    latent = gp.predict_points(pts)
    proba = gp.predict_points_proba(pts)
    Xz = gp._prepare_points_for_prediction(pts, output=["y"])[0]
    ks = gp.model.spec
    spec = O.make_spec(ks.D, ks.idx_cont, kind=ks.kind, ard=ks.ard)
    host = L.host(spec, gp._theta_fitted, gp.model.X, gp.model.y, Xz)
    assert latent.name == "y" and np.max(np.abs(latent.μ - host["mean"])) <= 1e-8 * np.max(np.abs(host["mean"]))
    assert np.max(np.abs(latent.σ2 - host["var"])) <= 1e-9
    p = np.asarray(proba.values(), dtype=float).ravel()
    assert proba.names == ["y"] and np.max(np.abs(p - averaged_sigmoid(host["mean"], host["var"]))) <= 1e-8
    assert np.array_equal(p, gp.predict_proba(Xz))
    # the fit separates the classes better than a coin
    assert np.mean((p > 0.5) == (df["y"].to_numpy()[:150] > 0.5)) > 0.6
    gp.prepare_grid(resolution=9)
    grid = gp.predict_grid_proba()
    g = np.asarray(grid.values(), dtype=float)
    assert grid.names == ["y"] and g.shape == gp.grid_parray.shape == (9, 9) and np.all((g > 0) & (g < 1))
    # what reads the exact factor is refused
    for call in (lambda: gp.predict_joint(Xz), lambda: gp.leave_one_out(), lambda: gp.cross_validate(), lambda: gp.predict_grad(Xz),
                 lambda: gp.build_model(sparse=True), lambda: gp.build_model(continuous_kernel="Periodic"),
                 lambda: gmb.GPC(ds, outputs=["y"], distributed=True)):
        with pytest.raises(NotImplementedError):
            call()
