"""``gmb_predict_with_grad`` -- posterior mean and variance with their gradients with respect to the test point -- on the MI355X
against the numpy reference of tests/var_grad_reference.py (itself pinned to finite differences and to an extended-precision
computation by tests/test_var_grad_cpu.py, which runs the cases of ``CASES`` below).  Needs a GPU (``-m gpu``).

Bars, each copied from where the project states it:

* ``dmean`` and ``dvar`` against the reference, separately: ``1e-8 max|G_ref|`` absolute -- the bar of tests/test_gpu_predict_grad.py;
* ``mean`` and ``var`` against ``Engine.predict``: 1e-10 relative -- the bar between the engine's two prediction forms; the same
  bar between the two sources of alpha;
* ``dvar`` against Richardson differences (h = 1e-3) of ``Engine.predict``'s variance: ``1e-4 max|G|`` -- the derivation of the
  mean gradient's wiring test: a wiring check, not an accuracy claim;
* state and determinism: bit-identical.

The tables use eta = 1.1 and sigma = 0.25 (``table``), so cond(Sigma) stays below about 2e4 at N = 1000.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import var_grad_reference as VR
from oracle import gp_oracle as O
from test_gpu_parity import GOLD, golden_spec, make_engine, rel
from test_gpu_predict_grad import DISPATCH_DIMS, frontend_dataset, points, table

pytestmark = pytest.mark.gpu

M_TILE = 32768  # gmb_predict's M-tile at these N (predict_tile_rows: 8 GiB / (8 Np) rows, at most 32768)


def check(got, ref, what):
    scale = float(np.max(np.abs(ref)))
    err = float(np.max(np.abs(got - ref)))
    print(f"{what}: max |G - G_ref| = {err:.3e}, max |G_ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert got.shape == ref.shape
    assert err <= 1e-8 * scale


# ---- the cases: name -> (spec, theta, X, y, Xs, periodic mode, periods) --------------------------------------------------------
def _stationary(kind, N, d, M, ard=True, on_train=0):
    def build():
        spec, theta, X, y = table(N, d, kind, ard)
        return spec, theta, X, y, points(X, M, list(range(d)), on_train=on_train), 0, None
    return build


def _composite():
    case = "composite_N140"
    spec, theta, X, y = golden_spec(case), GOLD[f"{case}/theta"], GOLD[f"{case}/X"], GOLD[f"{case}/y"]
    return spec, theta, X, y, points(X, 90, spec["idx_cont"], on_train=10), 0, None


def _additive():
    from test_oracle import additive_problem

    spec, theta, X, y = additive_problem(n=150, two_outputs=True, lin=True, hetero=True)  # N = 300
    return spec, theta, X, y, points(X, 130, spec["idx_cont"]), 0, None


def _periodic(kind, mode):
    def build():
        from test_gpu_periodic import case as periodic_case

        spec, theta, X, y, periods = periodic_case(kind, mode, 300, 2)
        return spec, theta, X, y, points(X, 120, [0, 1], on_train=20), mode, periods
    return build


CASES = {"ExpQuad-N300-d1-M100": _stationary("ExpQuad", 300, 1, 100),                       # three block columns, ragged
         **{f"{k}-N300-d3-M77": _stationary(k, 300, 3, 77, on_train=26) for k in O.KINDS},  # a third ON training points
         "Matern32-N1000-d3-M333": _stationary("Matern32", 1000, 3, 333),                   # eight block columns, M with a tail
         "ExpQuad-N260-d16-M50": _stationary("ExpQuad", 260, 16, 50),                       # every prepared column
         "Matern52-shared-ls": _stationary("Matern52", 300, 3, 77, ard=False),
         # every kind at every padded width 1, 2, 4, 8, 16: two block columns of N, the second ragged
         **{f"{k}-N200-d{d}-M70": _stationary(k, 200, d, 70) for k in O.KINDS for d in DISPATCH_DIMS},
         "composite_N140": _composite,
         "additive-N300": _additive,
         "Matern52+Periodic": _periodic("Matern52", 1),
         "Periodic": _periodic("ExpQuad", 2),
         "M-tiles": _stationary("ExpQuad", 300, 1, M_TILE + 77)}                            # a ragged second M-tile


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    spec, theta, X, y, Xs, mode, periods = case(name)
    return VR.mean_var_grad(spec, theta, X, y, Xs, periodic=mode, periods=periods)


def engine_for(name):
    spec, theta, X, y, Xs, mode, periods = case(name)
    if mode:
        from test_gpu_periodic import make_engine as periodic_engine

        return periodic_engine(spec, mode, periods, theta, X, y)
    return make_engine(spec, theta, X, y)


def run_case(name):
    """The engine's four results behind ``factorize`` checked against the reference and ``Engine.predict``; returns them."""
    Xs = case(name)[4]
    with engine_for(name) as eng:
        eng.factorize()
        mean, var, dmean, dvar = eng.predict_with_grad(Xs)
        mu_p, var_p = eng.predict(Xs)
    r_mean, r_var, r_dmean, r_dvar = reference(name)
    check(dmean, r_dmean, f"{name} dmean")
    check(dvar, r_dvar, f"{name} dvar")
    print(f"{name}: mean vs predict {rel(mean, mu_p):.2e}, var vs predict {rel(var, var_p):.2e}")
    assert rel(mean, mu_p) < 1e-10 and rel(var, var_p) < 1e-10
    return mean, var, dmean, dvar


# ---- 1. against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in CASES if n[0] in "EM" and n != "M-tiles" and "Periodic" not in n])
def test_matches_the_reference(gpu, name):
    run_case(name)


def test_noise_changes_the_variance_and_not_its_gradient(gpu):
    spec, theta, X, y, Xs, _, _ = case("Matern52-N300-d3-M77")
    with engine_for("Matern52-N300-d3-M77") as eng:
        eng.factorize()
        a = eng.predict_with_grad(Xs, with_noise=True)
        b = eng.predict_with_grad(Xs, with_noise=False)
    assert a[3].tobytes() == b[3].tobytes() and a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes()
    assert np.allclose(a[1] - b[1], O.noise_diag(spec, theta, Xs), rtol=1e-12, atol=0)


def test_composite_model_matches_the_reference(gpu):
    """Linear + coregion + two outputs (the golden composite case, N = 140): the prior term of the linear dimension; the
    categorical and output columns come back 0."""
    _, _, dmean, dvar = run_case("composite_N140")
    assert not np.any(dmean[:, 2:]) and not np.any(dvar[:, 2:])


def test_additive_model_matches_the_reference(gpu):
    name = "additive-N300"
    spec, theta, X, y, Xs, _, _ = case(name)
    with engine_for(name) as eng:
        eng.factorize()
        _, _, dmean, dvar = eng.predict_with_grad(Xs)
        mu, var = eng.predict(Xs)  # term 0's preparation of the training points is back in place
    ref = reference(name)
    check(dmean, ref[2], "additive dmean")
    check(dvar, ref[3], "additive dvar")
    mu_o, var_o = O.predict(spec, theta, X, y, Xs, dist_mode="direct")
    assert rel(mu, mu_o) < 1e-8 and rel(var, var_o) < 1e-8


@pytest.mark.parametrize("name", ["Matern52+Periodic", "Periodic"])
def test_periodic_models_match_the_reference(gpu, name):
    run_case(name)


@functools.lru_cache(maxsize=None)
def oracle_predict(name):
    """``O.predict`` (direct distances, with noise) at the points of a stationary case: the float64 reference of mean and variance."""
    spec, theta, X, y, Xs, _, _ = case(name)
    return O.predict(spec, theta, X, y, Xs, with_noise=True, dist_mode="direct")


def test_m_tiles_with_a_ragged_tail(gpu):
    """The call tiles M as ``gmb_predict`` does: two tiles, the second of 77 rows.  ``run_case`` compares mean and variance with
    ``Engine.predict``, which walks the same tile loop; they are therefore held to the oracle as well, at the bars of
    tests/test_gpu_parity.py against ``O.predict(direct)``: mean 1e-10 relative, variance 1e-11 absolute (on these inputs the
    float64 oracle is itself 1.8e-13 / 2.2e-15 from the extended-precision reference, cond(Sigma) ~ 3.7e3)."""
    mean, var, _, _ = run_case("M-tiles")
    mu_o, var_o = oracle_predict("M-tiles")
    e_m, e_v = rel(mean, mu_o), float(np.max(np.abs(var - var_o)))
    e_m2, e_v2 = rel(mean[M_TILE:], mu_o[M_TILE:]), float(np.max(np.abs(var[M_TILE:] - var_o[M_TILE:])))
    print(f"M-tiles vs oracle: mean {e_m:.2e} (second tile {e_m2:.2e}), var {e_v:.2e} (second tile {e_v2:.2e})")
    assert mean.shape == mu_o.shape and var.shape == var_o.shape
    assert e_m < 1e-10 and e_v < 1e-11


@pytest.mark.parametrize("name, fit", [("Matern52-N300-d3-M77", False),   # a padded prepared column, points on training points
                                       ("Matern52-N300-d3-M77", True),    # ... with the fit's alpha as the source
                                       ("ExpQuad-N260-d16-M50", False),   # every prepared column, a ragged last piece
                                       ("composite_N140", False),         # linear + two tables
                                       ("additive-N300", False),          # two terms
                                       ("Matern52+Periodic", False), ("Periodic", False)])  # both periodic rules
def test_mean_gradient_is_predict_grads_bit_for_bit(gpu, name, fit):
    """One kernel forms d mu / d x* for both calls (``predict_grad_partial_kernel``, NSET = 1 and 2, set 0 the same operations),
    and both tile M <= 16384 identically: the ``dmean`` of ``predict_with_grad`` is ``predict_grad``'s, to the bit."""
    theta, Xs = case(name)[1], case(name)[4]
    with engine_for(name) as eng:
        if fit:
            eng.evaluate(theta, grad=True)
        else:
            eng.factorize()
        dmean = eng.predict_with_grad(Xs)[2]
        G = eng.predict_grad(Xs)
    print(f"{name}: max |dmean - G| = {float(np.max(np.abs(dmean - G))):.3e}, max |G| = {float(np.max(np.abs(G))):.3e}")
    assert dmean.tobytes() == G.tobytes()


# ---- 2. the two sources of alpha; the gemm-form state -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", [600, 4224])
def test_back_substitution_and_the_fit_path_agree(gpu, N):
    spec, theta, X, y = table(N, 3, "Matern52")
    Xs = points(X, 200, [0, 1, 2])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        bs = eng.predict_with_grad(Xs)
        with pytest.raises(ValueError):
            eng.copy_alpha()  # back substitution leaves the gradient evaluation's alpha (and its flag) alone
        eng.evaluate(theta, grad=True)
        before = eng.predict(Xs)
        form = eng.timings()["predict_gemm_form"]
        alpha = eng.copy_alpha()
        fit = eng.predict_with_grad(Xs)
        fit2 = eng.predict_with_grad(Xs)
        after = eng.predict(Xs)
        assert eng.timings()["predict_gemm_form"] == form
        assert np.array_equal(alpha, eng.copy_alpha()) and eng.factor_is_current()
    for a, b, what in zip(bs, fit, ("mean", "var", "dmean", "dvar")):
        print(f"N={N} {what}: back substitution vs fit path {rel(a, b):.3e}")
        assert rel(a, b) < 1e-10
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fit, fit2))
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    if N == 4224:  # the fit left U and the inverse factor resident: predictions take the product form, before and after
        assert form == 1


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
def test_agrees_with_differences_of_the_predicted_variance(gpu):
    spec, theta, X, y = table(500, 2, "Matern52")
    Xs = points(X, 60, [0, 1])
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        dvar = eng.predict_with_grad(Xs)[3]
        fd = VR.fd_var_grad(lambda P: eng.predict(P, with_noise=False)[1], Xs, [0, 1], h=1e-3)
    err = float(np.max(np.abs(dvar - fd))) / float(np.max(np.abs(dvar)))
    print(f"dvar vs Richardson differences of Engine.predict's variance: {err:.3e}")
    assert err <= 1e-4


# ---- 4. state and determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit", [False, True])
def test_leaves_the_engine_as_it_found_it(gpu, fit):
    spec, theta, X, y = table(900, 3, "ExpQuad")
    Xs = points(X, 150, [0, 1, 2])

    def state(eng):
        mu, var = eng.predict(Xs)
        G = eng.predict_grad(Xs)
        val, g = eng.nlml(grad=True)
        return mu.tobytes(), var.tobytes(), G.tobytes(), np.float64(val).tobytes(), g.tobytes(), eng.factor_is_current()

    def prepare(eng):
        if fit:
            eng.evaluate(theta, grad=True)
        else:
            eng.factorize()

    with make_engine(spec, theta, X, y) as eng:
        prepare(eng)
        before = state(eng)
        prepare(eng)
        r1 = eng.predict_with_grad(Xs)
        r2 = eng.predict_with_grad(Xs)
        after = state(eng)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(r1, r2))
    assert before == after and before[5] is True


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_and_the_empty_request(gpu):
    from gumbi_amd.engine import GMB_EINVAL, GMB_HOST

    spec, theta, X, y = table(200, 2, "ExpQuad")
    with make_engine(spec, theta, X, y) as eng:
        with pytest.raises(ValueError):
            eng.predict_with_grad(X[:5])  # no factorisation yet
        eng.factorize()
        with pytest.raises(ValueError):
            eng.predict_with_grad(np.zeros((5, 3)))  # wrong width
        empty = eng.predict_with_grad(np.zeros((0, 2)))
        assert [a.shape for a in empty] == [(0,), (0,), (0, 2), (0, 2)]
        Xs = np.ascontiguousarray(X[:5])
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        mean, var = np.zeros(5), np.zeros(5)
        dm, dv = np.zeros((5, 2)), np.zeros((5, 2))
        rc = eng._lib.gmb_predict_with_grad(eng._h, ptr(Xs), 5, 2, 1, ptr(mean), ptr(var), ptr(dm), ptr(dv), 1, GMB_HOST)
        assert rc == GMB_EINVAL  # ldg < D
        wm, wv = np.full((5, 4), np.nan), np.full((5, 4), np.nan)
        rc = eng._lib.gmb_predict_with_grad(eng._h, ptr(Xs), 5, 2, 1, ptr(mean), ptr(var), ptr(wm), ptr(wv), 4, GMB_HOST)
        ref = eng.predict_with_grad(Xs)
        assert rc == 0 and np.array_equal(mean, ref[0]) and np.array_equal(var, ref[1])
        assert np.array_equal(wm[:, :2], ref[2]) and np.array_equal(wv[:, :2], ref[3])
        assert np.all(np.isnan(wm[:, 2:])) and np.all(np.isnan(wv[:, 2:]))


# ---- 6. front end ----------------------------------------------------------------------------------------------------------------
def test_frontend_propose_continuous(gpu):
    import gumbi_amd as gmb
    from gumbi_amd import acquisition as acq

    ds = frontend_dataset(300, ["y"])
    gp = gmb.GP(ds, outputs="y")
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 25})
    prop = gp.propose_continuous(acquisition="EI", maximize=True, num_restarts=6, raw_samples=128, seed=1)
    assert prop is gp.proposal
    lo, hi = gp.optimization_bounds
    z = np.array([prop[d].z.values().ravel()[0] for d in gp.continuous_dims])
    assert np.all(z >= lo - 1e-12) and np.all(z <= hi + 1e-12)
    for d in ("a", "b"):
        assert ds.wide[d].min() - 1e-9 <= prop[d].values().ravel()[0] <= ds.wide[d].max() + 1e-9
    # the acquisition recomputed from the public (noise-free) ``predict_points`` at the proposal
    pz = gp.predict_points(prop, with_noise=False).z
    value = acq.expected_improvement(np.ravel(pz.μ), np.ravel(pz.σ2), best=float(np.max(gp.model.y)), maximize=True)[0]
    print(f"proposal {z}, log EI {gp.proposal_acquisition:.6f}, recomputed {float(value[0]):.6f}")
    assert abs(float(value[0]) - gp.proposal_acquisition) <= 1e-8 * max(1.0, abs(gp.proposal_acquisition))
    # the search ran on the engine's gradients: scipy's jac is minus the chained gradient, and the lock-step run improved on
    # its starts (the best six raw samples)
    res = gp.proposal_result
    val, grad = gp.acquisition_with_grad(res.x.reshape(6, 2), acquisition="EI", maximize=True)
    start_total = float(np.sum(np.sort(gp.proposal_raw_acquisition)[-6:]))
    print(f"summed log EI: starts {start_total:.6f} -> optimised {-res.fun:.6f} in {res.nit} iterations")
    assert np.array_equal(res.jac, -grad.ravel()) and res.nit >= 1 and -res.fun > start_total


def test_frontend_kronecker_equals_the_stacked_model(gpu):
    """Two outputs on shared inputs (N = 2 x 150): the Kronecker path's ``predict_with_grad`` against the stacked model's at the
    same hyper-parameters (tests/test_gpu_frontend.py's bar for Kronecker-vs-stacked predictions: 1e-8)."""
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
    pa, _, _ = gk._prepare_points_for_prediction(pts, output=["y", "w"])
    for noise in (False, True):
        a = gk.engine.predict_with_grad(pa, with_noise=noise)
        b = gs.engine.predict_with_grad(pa, with_noise=noise)
        for x, z, what in zip(a, b, ("mean", "var", "dmean", "dvar")):
            print(f"Kronecker vs stacked, noise={noise}, {what}: {rel(x, z):.2e}")
            assert rel(x, z) < 1e-8
        assert not np.any(a[2][:, -1]) and not np.any(a[3][:, -1])
