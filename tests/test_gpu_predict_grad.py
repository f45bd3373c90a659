"""``gmb_predict_grad`` -- the gradient of the posterior mean with respect to the test point -- on the MI355X against the numpy
reference of tests/grad_reference.py (itself pinned to finite differences by tests/test_predict_grad_cpu.py).  Needs a GPU
(``-m gpu``).

Bars, each copied from where the project states it:

* against the reference: ``1e-8 max|G_ref|`` absolute -- the mean's bar of tests/test_gpu_parity.py;
* the two sources of alpha (back substitution behind ``factorize``; the gradient evaluation's alpha behind ``evaluate``):
  1e-10 relative -- the bar between the engine's two prediction forms;
* end to end against Richardson differences (h = 1e-3) of ``Engine.predict``'s mean: ``1e-4 max|G|`` -- the mean's 1e-8 bar
  divided by h / 2, with 5 x margin: a wiring check, not an accuracy claim;
* state and determinism: bit-identical.
"""
import ctypes as C

import numpy as np
import pytest

import grad_reference as GR
from oracle import gp_oracle as O
from test_gpu_parity import GOLD, golden_spec, kspec, make_engine, rel

pytestmark = pytest.mark.gpu


def table(N, d, kind="ExpQuad", ard=True, seed=0):
    X, y, ls = O.synthetic_table(N, d, seed=1000 * d + N + seed)
    spec = O.make_spec(d, range(d), kind=kind, ard=ard)
    theta = O.pack_theta(spec, ls if ard else [float(np.mean(ls))], 1.1, 0.25)
    return spec, theta, X, y


def points(X, M, cont, seed=1, on_train=0):
    """M test points: 0.3 sigma off randomly chosen training points along the continuous columns ``cont`` (every other column --
    categories, the output index -- kept), the first ``on_train`` of them exactly ON their training point."""
    rng = np.random.default_rng(seed)
    Xs = X[rng.integers(0, len(X), M)].copy()
    Xs[on_train:, cont] += 0.3 * rng.standard_normal((M - on_train, len(cont)))
    return Xs


def check(got, ref, what):
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max |G - G_ref| = {err:.3e}, max |G_ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert got.shape == ref.shape
    assert err <= 1e-8 * scale


# ---- 1. against the reference ------------------------------------------------------------------------------------------------
DISPATCH_DIMS = (1, 2, 3, 5, 9)  # continuous columns that pad to the widths 1, 2, 4, 8, 16 the kernels are compiled for

STATIONARY = ([("ExpQuad", 300, 1, 100, True, 0), ("Matern52", 600, 2, 400, True, 0)]
              + [(k, 300, 3, 77, True, 26) for k in O.KINDS]          # a third of the points exactly on training points
              + [("Matern32", 1000, 3, 333, True, 0),                 # ragged: 8 blocks of N, 6 of M, both with a tail
                 ("ExpQuad", 260, 16, 50, True, 0),                   # every prepared column in use
                 ("Matern52", 300, 3, 77, False, 0)]                  # one shared lengthscale
              # every kind at every padded width 1, 2, 4, 8, 16: two block columns of N, the second ragged
              + [(k, 200, d, 70, True, 0) for k in O.KINDS for d in DISPATCH_DIMS])


@pytest.mark.parametrize("kind,N,d,M,ard,on_train", STATIONARY)
def test_matches_the_reference(gpu, kind, N, d, M, ard, on_train):
    spec, theta, X, y = table(N, d, kind, ard)
    Xs = points(X, M, list(range(d)), on_train=on_train)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G = eng.predict_grad(Xs)
    check(G, GR.mean_grad(spec, theta, X, y, Xs), f"{kind} N={N} d={d} M={M} ard={ard}")


def test_composite_model_matches_the_reference(gpu):
    """Linear + coregion + two outputs (the golden composite case, N = 140): the categorical and output columns come back 0."""
    case = "composite_N140"
    spec, theta, X, y = golden_spec(case), GOLD[f"{case}/theta"], GOLD[f"{case}/X"], GOLD[f"{case}/y"]
    Xs = points(X, 90, spec["idx_cont"], on_train=10)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G = eng.predict_grad(Xs)
    check(G, GR.mean_grad(spec, theta, X, y, Xs), "composite N=140")
    assert not np.any(G[:, 2:])


def test_additive_model_matches_the_reference(gpu):
    from test_oracle import additive_problem

    spec, theta, X, y = additive_problem(n=150, two_outputs=True, lin=True, hetero=True)  # N = 300
    Xs = points(X, 130, spec["idx_cont"])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G = eng.predict_grad(Xs)
        check(G, GR.mean_grad(spec, theta, X, y, Xs), "additive N=300")
        mu, _ = eng.predict(Xs)  # term 0's preparation of the training points is back in place
    assert rel(mu, O.predict(spec, theta, X, y, Xs, dist_mode="direct")[0]) < 1e-8


@pytest.mark.parametrize("kind,mode", [("Matern52", 1), ("ExpQuad", 2)])
def test_periodic_models_match_the_reference(gpu, kind, mode):
    from test_gpu_periodic import case as periodic_case
    from test_gpu_periodic import make_engine as periodic_engine

    spec, theta, X, y, periods = periodic_case(kind, mode, 300, 2)
    Xs = points(X, 120, [0, 1], on_train=20)
    with periodic_engine(spec, mode, periods, theta, X, y) as eng:
        eng.factorize()
        G = eng.predict_grad(Xs)
    check(G, GR.mean_grad(spec, theta, X, y, Xs, periodic=mode, periods=periods), f"{kind} periodic mode {mode}")


def test_m_tiles_with_a_ragged_tail(gpu):
    """The call tiles M by 16384 rows: two tiles, the second of 77 rows."""
    spec, theta, X, y = table(300, 1, "ExpQuad")
    Xs = points(X, 16384 + 77, [0])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G = eng.predict_grad(Xs)
    check(G, GR.mean_grad(spec, theta, X, y, Xs), "M = 16384 + 77")


# ---- 2. the two sources of alpha ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [600, 4224])
def test_back_substitution_and_the_fit_path_agree(gpu, N):
    spec, theta, X, y = table(N, 3, "Matern52")
    Xs = points(X, 200, [0, 1, 2])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G_bs = eng.predict_grad(Xs)
        with pytest.raises(ValueError):
            eng.copy_alpha()  # back substitution leaves the gradient evaluation's alpha (and its flag) alone
        eng.evaluate(theta, grad=True)
        G_fit = eng.predict_grad(Xs)
    print(f"N={N}: back substitution vs fit path {rel(G_bs, G_fit):.3e}")
    assert rel(G_bs, G_fit) < 1e-10


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
def test_agrees_with_differences_of_the_predicted_mean(gpu):
    spec, theta, X, y = table(500, 2, "Matern52")
    Xs = points(X, 60, [0, 1])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        G = eng.predict_grad(Xs)
        fd = GR.fd_mean_grad(lambda P: eng.predict(P, with_noise=False)[0], Xs, [0, 1], h=1e-3)
    err = float(np.max(np.abs(G - fd))) / float(np.max(np.abs(G)))
    print(f"predict_grad vs Richardson differences of Engine.predict: {err:.3e}")
    assert err <= 1e-4


# ---- 4. state and determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [False, True])
def test_leaves_the_engine_as_it_found_it(gpu, fit):
    spec, theta, X, y = table(900, 3, "ExpQuad")
    Xs = points(X, 150, [0, 1, 2])

    def state(eng):
        mu, var = eng.predict(Xs)
        val, g = eng.nlml(grad=True)
        return mu.tobytes(), var.tobytes(), np.float64(val).tobytes(), g.tobytes(), eng.factor_is_current()

    def prepare(eng):
        if fit:
            eng.evaluate(theta, grad=True)
        else:
            eng.factorize()

    with make_engine(spec, theta, X, y) as eng:
        prepare(eng)
        before = state(eng)
        prepare(eng)
        G1 = eng.predict_grad(Xs)
        G2 = eng.predict_grad(Xs)
        after = state(eng)
    assert G1.tobytes() == G2.tobytes()
    assert before == after and before[4] is True


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_request(gpu):
    from gumbi_amd.engine import GMB_EINVAL, GMB_HOST

    spec, theta, X, y = table(200, 2, "ExpQuad")
    with make_engine(spec, theta, X, y) as eng:
        with pytest.raises(ValueError):
            eng.predict_grad(X[:5])  # no factorisation yet
        eng.factorize()
        with pytest.raises(ValueError):
            eng.predict_grad(np.zeros((5, 3)))  # wrong width
        empty = eng.predict_grad(np.zeros((0, 2)))
        assert empty.shape == (0, 2)
        Xs = np.ascontiguousarray(X[:5])
        out = np.zeros((5, 2))
        rc = eng._lib.gmb_predict_grad(eng._h, Xs.ctypes.data_as(C.c_void_p), 5, 2, out.ctypes.data_as(C.c_void_p), 1, GMB_HOST)
        assert rc == GMB_EINVAL  # ldg < D
        wide = np.full((5, 4), np.nan)
        rc = eng._lib.gmb_predict_grad(eng._h, Xs.ctypes.data_as(C.c_void_p), 5, 2, wide.ctypes.data_as(C.c_void_p), 4, GMB_HOST)
        assert rc == 0 and np.array_equal(wide[:, :2], eng.predict_grad(Xs)) and np.all(np.isnan(wide[:, 2:]))


# ---- 6. front end ----------------------------------------------------------------------------------------------------------------
def frontend_dataset(n, outputs, seed=3):
    import pandas as pd

    import gumbi_amd as gmb

    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 4.0, n), rng.uniform(10.0, 20.0, n)
    df = pd.DataFrame({"a": a, "b": b})
    for i, name in enumerate(outputs):
        df[name] = 3.0 + np.sin(a + i) * np.cos(0.3 * b) + 0.05 * rng.standard_normal(n)
    return gmb.DataSet(df, outputs=list(outputs))


def test_frontend_grid_gradient_matches_the_reference(gpu):
    import gumbi_amd as gmb

    ds = frontend_dataset(300, ["y"])
    gp = gmb.GP(ds, outputs="y")
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 25})
    gp.prepare_grid(resolution=12)
    grad = gp.predict_grid_grad(norm=False)
    assert grad.shape == (12, 12) and grad.names == ["δ[y]/δ[a]", "δ[y]/δ[b]"]
    norm = gp.predict_grid_grad()
    assert norm.shape == (12, 12) and norm.names == ["|∇|y"]
    theta = gp._theta_fitted
    pa, _, _ = gp._prepare_points_for_prediction(gp.grid_points, output=["y"])
    ref = GR.mean_grad(gp.model.spec.as_dict(), theta, gp.model.X, gp.model.y, pa)
    sy = np.sqrt(gp.stdzr["y"]["σ2"])
    parts = []
    for k, x_var in enumerate(["a", "b"]):
        want = ref[:, gp.dims.index(x_var)] * sy / np.sqrt(gp.stdzr[x_var]["σ2"])
        got = grad[f"δ[y]/δ[{x_var}]"].values().ravel()
        assert np.max(np.abs(got - want)) <= 1e-8 * np.max(np.abs(want))
        parts.append(want)
    want_norm = np.sqrt(parts[0] ** 2 + parts[1] ** 2)
    assert np.max(np.abs(norm["|∇|y"].values().ravel() - want_norm)) <= 1e-8 * np.max(want_norm)


def test_frontend_kronecker_gradient_equals_the_stacked_model(gpu):
    """Two outputs on shared inputs (N = 2 x 150): the Kronecker path's gradient against the stacked model's at the same
    hyper-parameters (tests/test_gpu_frontend.py's bar for Kronecker-vs-stacked predictions: 1e-8)."""
    import gumbi_amd as gmb
    from gumbi_amd.regression import icm

    ds = frontend_dataset(150, ["y", "w"])
    gk = gmb.GP(ds, outputs=["y", "w"], kronecker="auto")
    gk.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 15})
    assert isinstance(gk.engine, icm.IcmEngine)
    gs = gmb.GP(ds, outputs=["y", "w"], kronecker=False)
    gs.specify_model(continuous_dims=["a", "b"])
    gs.build_model()
    gs.find_MAP(theta=gk._theta_fitted)
    pts = gk.parray(a=np.linspace(0.8, 3.5, 40), b=np.linspace(11.0, 19.0, 40))
    a = gk.predict_points_grad(pts, norm=False)
    b = gs.predict_points_grad(pts, norm=False)
    assert a.names == b.names == ["δ[y]/δ[a]", "δ[y]/δ[b]", "δ[w]/δ[a]", "δ[w]/δ[b]"]
    for name in a.names:
        assert rel(a[name].values(), b[name].values()) < 1e-8
