"""The sparse (FITC) path of the engine against an extended-precision reference -- runs on the MI355X box only (``-m gpu``).

The problems are tests/fitc_reference.py's (``PROBLEMS``; ``seam``: two column tiles of X behind m = 16; ``DISPATCH``: every kind
at every padded width of the derivative kernel, N = 200, m = 16), Z from seeded k-means of X, test points M in {1, 129, 200}.  The engine and the float64 host restatement (LAPACK) are each compared with the longdouble
reference; for every problem and quantity the engine's error may be at most

    max(8 x the host's error, floor)

with the suite's own bars as floors: NLML 1e-10 (relative to max(1, |NLML|), as tests/test_gpu_periodic.py states it), every
gradient entry 1e-8 of max |grad|, the mean 1e-8 of max |mean|, the variances 1e-9 absolute.  8 x is the allowance
tests/test_gpu_conditioning.py gives a different summation order.  The problems are ill-conditioned in G_uu (k_ii - q_i down to
5e-8: cond(Kuu) ~ 1e6), so the gradient's bar comes from the host's measured error and not from a guess.  Every comparison
prints ``FITC <problem> <quantity> <engine error> <host error> <ratio>``; tests/golden/make_fitc_ratios.py turns a log of them
into tests/golden/fitc_ratios.json, the record behind DESIGN 3.17's table.

Then: the same bits call after call and form after form, the state rules of ``gmb_fitc_predict``, an exact fit on the same
engine untouched by the sparse calls, the memory bound, and the front end (``gumbi_amd.SparseGP``).
"""
import functools

import numpy as np
import pytest

import fitc_reference as F
from oracle import gp_oracle as O

pytestmark = pytest.mark.gpu

NAMES = list(F.PROBLEMS) + ["seam"]
K = 8.0
FLOOR = {"nlml": 1e-10, "grad": 1e-8, "mean": 1e-8, "var": 1e-9, "var_noise": 1e-9}


def kernel_spec(spec):
    from gumbi_amd.engine import KernelSpec

    return KernelSpec(D=spec["D"], idx_cont=spec["idx_cont"], kind=spec["kind"], ard=spec["ard"], jitter=spec["jitter"])


def make_engine(name, inducing=True):
    from gumbi_amd.engine import Engine

    spec, theta, X, y, Z, _ = F.problem(name)
    eng = Engine(0)
    eng.set_data(X, y)
    eng.set_kernel(kernel_spec(spec))
    if inducing:
        eng.set_inducing(Z)
    return eng


def scaled_errors(key, got, want):
    """the errors of one quantity in the units of its bar: NLML relative to max(1, |NLML|), gradient entries of max |grad|, the mean
    of max |mean|, variances absolute"""
    got, want = np.asarray(got, float), np.asarray(want, float)
    scale = {"nlml": max(1.0, abs(float(want))) if key == "nlml" else 1.0, "grad": np.max(np.abs(want)), "mean": np.max(np.abs(want))}.get(key, 1.0)
    return np.atleast_1d(np.abs(got - want)) / scale


class Bars:
    def __init__(self, name):
        self.name, self.ref, self.bad = name, F.references(name), []

    def check(self, key, got, rows=None, label=None):
        ref = self.ref[key] if rows is None else self.ref[key][:rows]
        host = self.ref["h_" + key] if rows is None else self.ref["h_" + key][:rows]
        err, e64 = scaled_errors(key, got, ref), scaled_errors(key, host, ref)
        # (the gradient entry by entry; every other quantity by its worst element, host and engine alike)
        if key != "grad":
            err, e64 = np.array([err.max()]), np.array([e64.max()])
        bound = np.maximum(K * e64, FLOOR[key])
        label = label or key
        for j in range(err.size):
            tag = f"{label}[{j}]" if key == "grad" else label
            print(f"FITC {self.name} {tag} {err[j]:.3e} {e64[j]:.3e} {err[j] / max(e64[j], 1e-300):.4g}")
            if not err[j] <= bound[j]:
                self.bad.append(f"{tag}: {err[j]:.3e} > {bound[j]:.3e} = max(8 x host {e64[j]:.2e}, floor {FLOOR[key]:.0e})")

    def done(self):
        assert not self.bad, f"{self.name}: " + "; ".join(self.bad)


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES + list(F.DISPATCH))  # (DISPATCH: fitc_deriv_kernel<KIND, NC> at every kind and width)
def test_engine_within_8x_of_the_float64_host(gpu, name):
    spec, theta, X, y, Z, Xs = F.problem(name)
    bars = Bars(name)
    with make_engine(name) as eng:
        nlml, grad = eng.fitc_evaluate(theta, grad=True)
        bars.check("nlml", nlml)
        bars.check("grad", grad)
        for M in F.TEST_POINTS:
            mean, var_noise = eng.fitc_predict(Xs[:M], with_noise=True)
            _, var = eng.fitc_predict(Xs[:M], with_noise=False)
            bars.check("mean", mean, rows=M, label=f"mean(M={M})")
            bars.check("var_noise", var_noise, rows=M, label=f"var_noise(M={M})")
            bars.check("var", var, rows=M, label=f"var(M={M})")
        assert eng.notpd_index() == -1
    bars.done()


# ---- the same bits --------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", ["m52-ragged-0.2", "seam"])
def test_repeated_calls_give_the_same_bits(gpu, name):
    spec, theta, X, y, Z, Xs = F.problem(name)
    with make_engine(name) as eng:
        v0, g0 = eng.fitc_evaluate(theta, grad=True)
        p0 = eng.fitc_predict(Xs, with_noise=True)
        v1 = eng.fitc_evaluate(theta, grad=False)  # grad = NULL: the NLML of the call with a gradient
        p1 = eng.fitc_predict(Xs, with_noise=True)
        v2, g2 = eng.fitc_evaluate(theta * 1.01, grad=True)
        v3, g3 = eng.fitc_evaluate(theta, grad=True)
        p3 = eng.fitc_predict(Xs, with_noise=True)
    assert bits(v0) == bits(v1) == bits(v3) and v2 != v0
    assert np.array_equal(bits(g0), bits(g3)) and not np.array_equal(g0, g2)
    for a, b, c in zip(p0, p1, p3):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_points_behind_a_tile_seam_against_the_same_points_alone(gpu):
    """M = 32768 + 77 test points are two M-tiles of the plan; the 77 behind the seam, sent alone, are one tile of the same shape"""
    from gumbi_amd import engine

    name = "m52-ragged-0.2"
    spec, theta, X, y, Z, _ = F.problem(name)
    tile = engine.fitc_plan(len(X), len(Z))["tile_rows"]
    Xs = np.random.default_rng(8).standard_normal((tile + 77, X.shape[1]))
    with make_engine(name) as eng:
        eng.fitc_evaluate(theta, grad=False)
        mean, var = eng.fitc_predict(Xs)
        mean_t, var_t = eng.fitc_predict(Xs[tile:])
        mean_1, var_1 = eng.fitc_predict(Xs[tile + 5:tile + 6])
    assert np.array_equal(bits(mean[tile:]), bits(mean_t)) and np.array_equal(bits(var[tile:]), bits(var_t))
    assert bits(mean[tile + 5]) == bits(mean_1[0]) and bits(var[tile + 5]) == bits(var_1[0])
    # ... and the long call is right on both sides of the seam
    pick = np.r_[0:40, tile - 40:tile + 77]
    ref = F.precise(spec, theta, X, y, Z, Xs[pick])
    assert np.max(np.abs(mean[pick] - np.asarray(ref["mean"], float))) <= 1e-8 * np.max(np.abs(ref["mean"]))
    assert np.max(np.abs(var[pick] - np.asarray(ref["var_noise"], float))) <= 1e-9


def test_every_call_form_against_the_packed_host_call(gpu):
    """device memory and leading dimensions larger than the row, for Z and for the test points: the same bits, nothing written
    outside the M results"""
    import ctypes as C

    from test_gpu_abi_forms import FORMS, PACKED_HOST, mat_in, same_bits, sync, take_vec, vec_out

    name = "m32-2d"
    spec, theta, X, y, Z, Xs = F.problem(name)
    Xs = Xs[:129]
    th = np.ascontiguousarray(theta)

    def run(form):
        with make_engine(name, inducing=False) as eng:
            z = mat_in(Z, form, 3)
            sync()
            eng._check(eng._lib.gmb_fitc_set_inducing(eng._h, z.ptr, len(Z), z.ld, form.memspace), f"gmb_fitc_set_inducing ({form.name})")
            z.poison()  # the library keeps no caller pointer
            sync()
            val = C.c_double()
            g = np.empty(th.size)
            eng._check(eng._lib.gmb_fitc_evaluate(eng._h, th.ctypes.data_as(C.POINTER(C.c_double)), th.size, C.byref(val),
                                                  g.ctypes.data_as(C.POINTER(C.c_double))), "gmb_fitc_evaluate")
            what = f"gmb_fitc_predict ({form.name})"
            x, mean, var = mat_in(Xs, form, 3), vec_out(len(Xs), form), vec_out(len(Xs), form)
            sync()
            eng._check(eng._lib.gmb_fitc_predict(eng._h, x.ptr, len(Xs), x.ld, 1, mean.ptr, var.ptr, form.memspace), what)
            return val.value, g, take_vec(mean, len(Xs), what + " mean"), take_vec(var, len(Xs), what + " var")

    v0, g0, m0, s0 = run(PACKED_HOST)
    with make_engine(name) as eng:  # engine.py's own calls
        v, g = eng.fitc_evaluate(theta)
        m, s = eng.fitc_predict(Xs)
    assert bits(v) == bits(v0)
    same_bits(g, g0, "engine.py gradient")
    same_bits(m, m0, "engine.py mean")
    same_bits(s, s0, "engine.py var")
    for form in FORMS[1:]:
        v1, g1, m1, s1 = run(form)
        assert bits(v1) == bits(v0), form.name
        same_bits(g1, g0, f"{form.name}: gradient")
        same_bits(m1, m0, f"{form.name}: mean")
        same_bits(s1, s0, f"{form.name}: var")


# ---- state ----------------------------------------------------------------------------------------------------------------------------
def test_predict_is_refused_without_a_resident_state(gpu):
    name = "expquad-1d"
    spec, theta, X, y, Z, Xs = F.problem(name)
    with make_engine(name, inducing=False) as eng:
        with pytest.raises(ValueError, match="gmb_fitc_set_inducing"):
            eng.fitc_evaluate(theta)
        with pytest.raises(ValueError, match="gmb_fitc_set_inducing"):
            eng.fitc_predict(Xs)
        eng.set_inducing(Z)
        with pytest.raises(ValueError, match="gmb_fitc_evaluate first"):
            eng.fitc_predict(Xs)  # before any evaluation
        eng.fitc_evaluate(theta, grad=False)
        want = eng.fitc_predict(Xs)
        eng.set_theta(theta)
        with pytest.raises(ValueError, match="gmb_fitc_evaluate first"):
            eng.fitc_predict(Xs)  # after set_theta, even to the same values
        eng.fitc_evaluate(theta, grad=False)
        eng.set_inducing(Z)
        with pytest.raises(ValueError, match="gmb_fitc_evaluate first"):
            eng.fitc_predict(Xs)  # after new inducing points
        eng.fitc_evaluate(theta, grad=False)
        eng.set_y(y)
        with pytest.raises(ValueError, match="gmb_fitc_evaluate first"):
            eng.fitc_predict(Xs)
        eng.fitc_evaluate(theta, grad=False)
        eng.set_data(X, y)
        with pytest.raises(ValueError, match="gmb_fitc_set_inducing"):
            eng.fitc_predict(Xs)  # after set_data: the inducing points are gone with it
        eng.set_kernel(kernel_spec(spec))
        eng.set_inducing(Z)
        eng.fitc_evaluate(theta, grad=False)
        got = eng.fitc_predict(Xs)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        with pytest.raises(ValueError, match="exceed the limit"):
            eng.set_inducing(np.zeros((16385, 1)))
        with pytest.raises(ValueError):
            eng.set_inducing(np.full((3, 1), np.nan))


def test_models_outside_the_scope_are_refused(gpu):
    from gumbi_amd.engine import Engine, KernelSpec

    rng = np.random.default_rng(0)
    X = np.column_stack([rng.standard_normal(50), rng.integers(0, 2, 50).astype(float)])
    y = rng.standard_normal(50)
    cases = {"categorical": KernelSpec(D=2, idx_cont=[0], coreg=[(1, 2)]), "linear": KernelSpec(D=2, idx_cont=[0, 1], idx_lin=[0]),
             "outputs": KernelSpec(D=2, idx_cont=[0], out_col=1, n_out=2),
             "periodic": KernelSpec(D=2, idx_cont=[0, 1], periodic=1, periods=[1.0, 2.0])}
    for what, ks in cases.items():
        with Engine(0) as eng:
            eng.set_data(X, y)
            eng.set_kernel(ks)
            with pytest.raises(ValueError, match="sparse approximation"):
                eng.set_inducing(X[:5])


def test_exact_fit_on_the_same_engine_is_untouched(gpu):
    """factorize + predict before and after the sparse calls: the bits of an engine that never saw them"""
    name = "m52-ragged-0.2"
    spec, theta, X, y, Z, Xs = F.problem(name)

    def exact(eng):
        eng.set_theta(theta)
        eng.factorize()
        return eng.predict(Xs) + (np.array([eng.nlml()]),)

    with make_engine(name, inducing=False) as clean:
        want = exact(clean)
    with make_engine(name) as eng:
        before = exact(eng)
        assert eng.factor_is_current()
        eng.fitc_evaluate(theta, grad=True)
        assert not eng.factor_is_current()  # theta was set: the exact factor is stale by FactorState's rules
        with pytest.raises(ValueError):
            eng.predict(Xs)
        eng.fitc_predict(Xs)
        after = exact(eng)
        sparse = eng.fitc_evaluate(theta, grad=False)
    for a, b, c in zip(want, before, after):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    assert abs(sparse - F.references(name)["nlml"]) <= 1e-9 * abs(sparse)


# ---- memory ---------------------------------------------------------------------------------------------------------------------------
def test_nothing_of_n_squared_is_allocated(gpu):
    from gumbi_amd.engine import Engine

    N, d, m = 20000, 2, 128
    X, y, ls = O.synthetic_table(N, d)
    spec = O.make_spec(d, range(d), kind="Matern52")
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    Z = F.kmeans_points(X[:4000], m, seed=1)
    Xs = np.random.default_rng(0).standard_normal((256, d))
    with Engine(0) as eng:
        eng.set_data(X, y)
        eng.set_kernel(kernel_spec(spec))
        eng.set_inducing(Z)
        nlml, grad = eng.fitc_evaluate(theta, grad=True)
        mean, var = eng.fitc_predict(Xs)
        peak = eng.resident_bytes(peak=True)
    print(f"FITC-MEM N={N} m={m}: peak {peak / 2**20:.1f} MiB against the bound {8 * N * N / 4 / 2**20:.0f} MiB")
    assert np.isfinite(nlml) and np.all(np.isfinite(grad)) and np.all(np.isfinite(mean)) and np.all(var > 0)
    assert peak < 8 * N * N / 4  # any N x N allocation, a triangle included, exceeds this
    # a sub-sample of the same table agrees with the reference on the host (the call above is not only small, it is right)
    sub = slice(0, N, 10)
    with Engine(0) as eng:
        eng.set_data(X[sub], y[sub])
        eng.set_kernel(kernel_spec(spec))
        eng.set_inducing(Z)
        val = eng.fitc_evaluate(theta, grad=False)
    assert abs(val - F.nlml(spec, theta, X[sub], y[sub], Z)) <= 1e-9 * abs(val)


# ---- the front end --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic_fit():
    import pandas as pd

    import gumbi_amd as gmb

    rng = np.random.default_rng(12)
    n = 2000
    a, b = rng.uniform(0.0, 6.0, n), rng.uniform(0.0, 6.0, n)
    f = np.sin(a) * np.cos(0.7 * b)
    df = pd.DataFrame({"a": a, "b": b, "y": f + 0.1 * rng.standard_normal(n)})
    gp = gmb.SparseGP(gmb.DataSet(df, outputs=["y"]))
    gp.fit(continuous_dims=["a", "b"], n_u=64, continuous_kernel="Matern52")
    return gp, df, f


def test_sparse_gp_on_a_synthetic_table(gpu):
    gp, df, f = synthetic_fit()
    assert gp.sparse and 1 <= gp.n_u <= 64 and gp.inducing_points.shape == (gp.n_u, 2)
    assert gp.nlml_trace[-1] < gp.nlml_trace[0]
    gp.prepare_grid(resolution=12)
    pred = gp.predict_grid()
    assert pred.shape == gp.grid_parray.shape == (12, 12)
    # gp.predict at the fitted theta is the reference's prediction, within the bars of this file
    X, y = gp.get_shaped_data("mean")
    spec = O.make_spec(2, [0, 1], kind="Matern52")
    pa = gp._prepare_points_for_prediction(gp.grid_points, output=gp._parse_prediction_output(None))[0]
    mean, var = gp.predict(pa)
    ref = F.precise(spec, gp._theta_fitted, X, y, gp.inducing_points, pa)
    h_mean, h_var = F.predict(spec, gp._theta_fitted, X, y, gp.inducing_points, pa)
    for key, got, host, want in (("mean", mean, h_mean, ref["mean"]), ("var_noise", var, h_var, ref["var_noise"])):
        want = np.asarray(want, float)
        err, e64 = scaled_errors(key, got, want).max(), scaled_errors(key, host, want).max()
        print(f"FITC frontend {key} {err:.3e} {e64:.3e} {err / max(e64, 1e-300):.4g}")
        assert err <= max(K * e64, FLOOR[key])
    # the fit follows the generator's function
    pts = gp.parray(a=df["a"].to_numpy()[:500], b=df["b"].to_numpy()[:500])
    mu = gp.predict_points(pts, with_noise=False).μ
    assert np.corrcoef(np.asarray(mu, float).ravel(), f[:500])[0, 1] > 0.99


def test_sparse_gp_cross_validates_and_refuses_the_rest(gpu):
    gp, df, f = synthetic_fit()
    cv = gp.cross_validate(pct_train=0.8, seed=3, maxeval=60)
    assert set(cv) == {"train", "test"} and np.all(np.isfinite(cv["test"]["NLPDs"]))
    for name in type(gp).NOT_BUILT:
        with pytest.raises(NotImplementedError, match="is not built for the sparse approximation"):
            getattr(gp, name)()
