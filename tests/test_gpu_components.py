"""The components of an additive model on the MI355X: the ``*_terms`` forms of the four prediction calls (a selection of the
model's covariance terms) and ``gmb_predict_decompose`` (all components and their pointwise covariance from one stacked solve),
against the numpy restatement in tests/components_reference.py.  Needs a GPU (``-m gpu``).

Shapes: the three-term additive model of components_reference.three_term_problem -- N = 300 (three block columns, the last
ragged; two categorical tables, output table, linear part and hetero noise all live), M = 75 test points (one ragged tile) -- once
behind ``factorize`` (the triangular solve) and once behind ``evaluate(theta, grad=True)`` (the product with the resident inverse
factor, which the selecting calls take exactly as their parents do).  The multi-tile case is M = 10880 + 77 at the same N: the
smallest shape at which the stacked offsets ``t * mpad`` and the tile offsets ``m0`` both run, with a ragged last tile.  The
single-term control is Matern52, d = 3, at N = 300.

Bars, each copied from the existing additive test of the call's parent (tests/test_gpu_term_walk.py lists them):

* ``predict``: mean 1e-8 relative to max |ref|, variance 1e-9 absolute;
* ``predict_grad``: ``1e-8 max|G_ref|`` absolute;
* ``predict_joint``: covariance 1e-9 absolute, mean 1e-8 relative; ``draw_joint`` (``with_noise=True``, ``jitter=0``): 1e-8 of
  max |Y_ref|;
* two GPU results that are the same quantity by different launches (a sum of components against the total; a joint diagonal
  against ``predict``): 1e-10 relative for means and gradients, 1e-9 absolute for variances;
* all bits set against the call without a selection, and any call repeated: bit-identical.

The reference's own two formulations agree to 6e-13 on this problem (tests/test_components_cpu.py), three orders inside these.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import abi_forms as AF
import components_reference as CR
from oracle import gp_oracle as O
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

STATES = ["solve", "product"]
SELECTIONS = [(0,), (1,), (2,), (0, 2), (1, 2)]
M_TILE = 10880  # the decomposition's M-tile at N = 300, T = 3: floor(32768 / 3 / 128) * 128


@functools.lru_cache(maxsize=None)
def reference():
    """The three-term problem, its reference and three rows of fixed normals."""
    spec, theta, X, y, Xs = CR.three_term_problem()
    return CR.Components(spec, theta, X, y, Xs), np.random.default_rng(6).standard_normal((3, len(Xs)))


@contextlib.contextmanager
def engine_in(state, problem=None):
    spec, theta, X, y = (problem or CR.three_term_problem())[:4]
    with make_engine(spec, theta, X, y) as eng:
        if state == "solve":
            eng.factorize()
        else:
            eng.evaluate(theta, grad=True)
        yield eng


def same_bits(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def close_to(got, ref, what):
    """max |got - ref| / max |ref|, printed."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale, err = float(np.max(np.abs(ref))), float(np.max(np.abs(got - ref)))
    print(f"COMPONENTS {what}: max |got - ref| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    return err / scale


def abs_err(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.max(np.abs(got - ref)))
    print(f"COMPONENTS {what}: max |got - ref| = {err:.3e}")
    return err


# ---- 1. predict(terms=S) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", SELECTIONS)
@pytest.mark.parametrize("state", STATES)
def test_predict_of_a_selection(gpu, state, sel):
    """{1}, {2} and {1, 2} never visit term 0: the first selected pass stores and carries the model's noise."""
    comps, _ = reference()
    with engine_in(state) as eng:
        for with_noise in (True, False):
            mu, var = eng.predict(comps.Xs, with_noise=with_noise, terms=sel)
            mu_r, var_r = comps.predict_terms(sel, with_noise=with_noise)
            what = f"{state} predict terms={sel} noise={with_noise}"
            assert close_to(mu, mu_r, what + " mean") <= 1e-8
            assert abs_err(var, var_r, what + " var") <= 1e-9
        assert eng.timings()["predict_gemm_form"] == (1 if state == "product" else 0)


# ---- 2. all bits: the calls without a selection, to the bit ------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
def test_all_terms_is_the_call_without_a_selection(gpu, state):
    comps, Z = reference()
    Xs = comps.Xs
    with engine_in(state) as eng:
        assert eng.num_terms == 3
        pairs = [("predict", lambda **k: eng.predict(Xs, **k)),
                 ("predict noise-free", lambda **k: eng.predict(Xs, with_noise=False, **k)),
                 ("predict_grad", lambda **k: eng.predict_grad(Xs, **k)),
                 ("predict_joint", lambda **k: eng.predict_joint(Xs, with_noise=True, jitter=0.0, **k)),
                 ("draw_joint", lambda **k: eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0, return_mean=True, **k))]
        for name, call in pairs:
            plain = call()
            assert same_bits(call(terms=0b111), plain), f"{state}: {name}(terms=all) differs from {name}()"
            assert same_bits(call(terms=[0, 1, 2]), plain), f"{state}: {name}(terms=[0, 1, 2]) differs from {name}()"


# ---- 3. predict_grad(terms=S) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
def test_gradient_of_a_selection(gpu, state):
    comps, _ = reference()
    with engine_in(state) as eng:
        total = eng.predict_grad(comps.Xs)
        single = []
        for sel in SELECTIONS:
            G = eng.predict_grad(comps.Xs, terms=sel)
            assert close_to(G, comps.grad_terms(sel), f"{state} predict_grad terms={sel}") <= 1e-8
            if len(sel) == 1:
                single.append(G)
        assert close_to(sum(single), total, f"{state} sum of single-term gradients against the total") <= 1e-10


# ---- 4. the joint posterior of a selection -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", [(1,), (0, 2)])
@pytest.mark.parametrize("state", STATES)
def test_joint_posterior_of_a_selection(gpu, state, sel):
    comps, Z = reference()
    with engine_in(state) as eng:
        mean, cov = eng.predict_joint(comps.Xs, with_noise=True, jitter=0.0, terms=sel)
        mean_r, cov_r = comps.joint_terms(sel, with_noise=True, jitter=0.0)
        assert abs_err(cov, cov_r, f"{state} joint cov terms={sel}") <= 1e-9
        assert close_to(mean, mean_r, f"{state} joint mean terms={sel}") <= 1e-8
        assert np.array_equal(cov, cov.T)
        _, var = eng.predict(comps.Xs, with_noise=True, terms=sel)
        assert close_to(np.diag(cov), var, f"{state} joint diagonal against predict terms={sel}") <= 1e-10
        if sel == (1,):
            Y, m2 = eng.draw_joint(comps.Xs, Z, with_noise=True, jitter=0.0, return_mean=True, terms=sel)
            Y_r = mean_r[None, :] + Z @ O.cholesky_lower(cov_r).T
            assert close_to(Y, Y_r, f"{state} draws terms={sel}") <= 1e-8
            assert same_bits(m2, mean)


# ---- 5. the decomposition -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
def test_decomposition(gpu, state):
    comps, _ = reference()
    Xs = comps.Xs
    means_r, cov_r, noise_r = comps.decompose()
    with engine_in(state) as eng:
        means, cov, noise = eng.predict_decompose(Xs)
        assert means.shape == (3, 75) and cov.shape == (3, 3, 75) and noise.shape == (75,)
        for t in range(3):
            assert close_to(means[t], means_r[t], f"{state} decompose mean {t}") <= 1e-8
            for u in range(t + 1):
                assert abs_err(cov[t, u], cov_r[t, u], f"{state} decompose cov {t},{u}") <= 1e-9
                assert np.array_equal(cov[t, u], cov[u, t])
        assert close_to(noise, O.noise_diag(comps.spec, comps.theta, Xs), f"{state} decompose noise") <= 1e-14
        mu, var = eng.predict(Xs, with_noise=False)
        assert close_to(means.sum(axis=0), mu, f"{state} sum of means against predict") <= 1e-10
        assert abs_err(cov.sum(axis=(0, 1)), var, f"{state} sum of covariances against predict") <= 1e-9
        _, var02 = eng.predict(Xs, with_noise=False, terms=(0, 2))
        assert abs_err(cov[np.ix_([0, 2], [0, 2])].sum(axis=(0, 1)), var02, f"{state} selection (0, 2) from cov against predict_terms") <= 1e-9
        assert same_bits(eng.predict_decompose(Xs), (means, cov, noise))
        assert eng.predict_decompose(Xs[:0])[0].shape == (3, 0)


def test_decomposition_of_a_single_term_model_is_predict(gpu):
    from test_gpu_predict_grad import table

    spec, theta, X, y = table(300, 3, "Matern52")
    Xs = X[::4].copy()
    Xs[:, 0] += 0.17
    with engine_in("solve", (spec, theta, X, y)) as eng:
        assert eng.num_terms == 1
        means, cov, noise = eng.predict_decompose(Xs)
        mu, var = eng.predict(Xs, with_noise=False)
        assert means.shape == (1, len(Xs)) and cov.shape == (1, 1, len(Xs))
        assert close_to(means[0], mu, "single term decompose mean") <= 1e-10
        assert abs_err(cov[0, 0], var, "single term decompose var") <= 1e-9
        assert abs_err(noise, O.noise_diag(spec, theta, Xs), "single term noise") <= 1e-14


# ---- 6. more than one M-tile ------------------------------------------------------------------------------------------------------
def test_decomposition_over_two_tiles_with_padded_outputs(gpu):
    """M = 10880 + 77: the second tile's rows come from other stacked offsets (``t * 128`` against ``t * 10880``) and land at
    ``m0 = 10880`` of rows whose leading dimensions are larger than M; nothing beyond column M of a row is written."""
    spec, theta, X, y, _ = CR.three_term_problem()
    rng = np.random.default_rng(12)
    M = M_TILE + 77
    Xs = X[rng.integers(0, len(X), M)].copy()
    Xs[:, :2] += 0.3 * rng.standard_normal((M, 2))
    means_r, cov_r, noise_r = CR.decompose(spec, theta, X, y, Xs)
    packed_r = CR.pack_lower(cov_r)
    T, ldm, ldcv = 3, M + 37, M + 5
    means = AF.embed(np.zeros((T, M)), ldm, AF.FILL)
    packed = AF.embed(np.zeros((T * (T + 1) // 2, M)), ldcv, AF.FILL)
    noise = AF.padded(M, AF.SPARE, AF.FILL)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with engine_in("solve") as eng:
        rc = eng._lib.gmb_predict_decompose(eng._h, ptr(Xs), M, Xs.shape[1], ptr(means), ldm, ptr(packed), ldcv, ptr(noise), 0)
        assert rc == 0
    assert AF.untouched(means, M, AF.FILL_BITS, rows=T)
    assert AF.untouched(packed, M, AF.FILL_BITS, rows=T * (T + 1) // 2)
    assert AF.untouched(noise, M, AF.FILL_BITS)
    for name, lo, hi in (("first tile", 0, M_TILE), ("second tile", M_TILE, M)):
        for t in range(T):
            assert close_to(means[t, lo:hi], means_r[t, lo:hi], f"two tiles, {name}, mean {t}") <= 1e-8
        for p in range(T * (T + 1) // 2):
            assert abs_err(packed[p, lo:hi], packed_r[p, lo:hi], f"two tiles, {name}, cov row {p}") <= 1e-9
        assert close_to(noise[lo:hi], noise_r[lo:hi], f"two tiles, {name}, noise") <= 1e-14


# ---- 7. state ---------------------------------------------------------------------------------------------------------------------
def new_calls(eng, Xs, Z):
    return [("predict_terms", lambda: eng.predict(Xs, terms=(1,))),
            ("predict_grad_terms", lambda: eng.predict_grad(Xs, terms=(2,))),
            ("predict_joint_terms", lambda: eng.predict_joint(Xs, with_noise=True, jitter=0.0, terms=(1, 2))),
            ("draw_joint_terms", lambda: eng.draw_joint(Xs, Z, with_noise=True, jitter=0.0, terms=(1,))),
            ("predict_decompose", lambda: eng.predict_decompose(Xs))]


@pytest.mark.parametrize("state", STATES)
def test_new_calls_leave_the_engine_as_found(gpu, state):
    """Behind each new call: the factor is current, v (and behind the evaluation alpha) and a plain ``predict`` have the bits they
    had before, and the prediction still takes the form it took; each call gives the same bits in a second round run in the
    reverse order."""
    comps, Z = reference()
    Xs = comps.Xs
    with engine_in(state) as eng:
        def snapshot():
            snap = (eng.copy_v(),) + eng.predict(Xs)
            form = eng.timings()["predict_gemm_form"]
            return (snap + (eng.copy_alpha(),) if state == "product" else snap), form

        assert eng.factor_is_current()
        before, form = snapshot()
        assert form == (1 if state == "product" else 0)
        calls = new_calls(eng, Xs, Z)
        first = {}
        for name, call in calls:
            first[name] = call()
            assert eng.factor_is_current(), f"{state}: the factor is not current behind {name}"
            after, form_after = snapshot()
            assert same_bits(after, before), f"{state}: v / predict / alpha changed behind {name}"
            assert form_after == form, f"{state}: predict changed its form behind {name}"
        for name, call in reversed(calls):
            assert same_bits(call(), first[name]), f"{state}: {name} differs between its two runs"
        assert same_bits(snapshot()[0], before)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------
def test_empty_and_foreign_selections_are_refused(gpu):
    comps, Z = reference()
    Xs = comps.Xs
    with engine_in("solve") as eng:
        before = (eng.copy_v(),) + eng.predict(Xs)
        for bad in (0, 0b1000, 0b1001, [3], []):
            for call in (lambda: eng.predict(Xs, terms=bad), lambda: eng.predict_grad(Xs, terms=bad),
                         lambda: eng.predict_joint(Xs, terms=bad), lambda: eng.draw_joint(Xs, Z, terms=bad)):
                with pytest.raises(ValueError, match="terms"):
                    call()
        assert eng.factor_is_current()
        assert same_bits((eng.copy_v(),) + eng.predict(Xs), before)


# ---- 9. the front end ---------------------------------------------------------------------------------------------------------------
def additive_dataset(n=120, seed=5):
    import pandas as pd

    import gumbi_amd as gmb

    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.5, 4.0, n), rng.uniform(10.0, 20.0, n)
    g = rng.integers(0, 3, n)
    y = 3.0 + np.sin(a) * np.cos(0.3 * b) + 0.4 * g * np.cos(a) + 0.05 * rng.standard_normal(n)
    df = pd.DataFrame({"a": a, "b": b, "g": np.array(["u", "v", "w"])[g], "y": y})
    return gmb.DataSet(df, outputs=["y"])


def round_trip(got, want):
    """A standardized value that went through the uparray (un-standardized, then standardized again: two affine maps in f64)
    against the engine's: a few ulp of O(1) numbers, held to 1e-12."""
    return np.allclose(np.asarray(got).ravel(), np.asarray(want).ravel(), rtol=1e-12, atol=1e-12)


def test_front_end_levels(gpu):
    import gumbi_amd as gmb

    gp = gmb.GP(additive_dataset(), outputs="y")
    gp.specify_model(continuous_dims=["a", "b"], categorical_dims="g", additive=True)
    gp.build_model()
    assert gp.additive_levels == {"total": 0b11, "global": 0b01, "g": 0b10}
    theta = np.abs(np.random.default_rng(2).normal(1.0, 0.2, gp.model.spec.theta_size())) + 0.3
    gp.find_MAP(theta=theta)
    M = 40
    rng = np.random.default_rng(8)
    pts = gp.parray(a=rng.uniform(0.8, 3.5, M), b=rng.uniform(11.0, 19.0, M), g=np.full(M, gp.categorical_coords["g"]["v"]))
    pa, _, _ = gp._prepare_points_for_prediction(pts, output=["y"])
    eng = gp.engine
    assert eng.num_terms == 2
    for level, sel in (("global", (0,)), ("g", (1,))):
        up = gp.predict_points(pts, additive_level=level)
        mu, var = eng.predict(pa, with_noise=True, terms=sel)
        assert round_trip(up.z.μ, mu) and round_trip(up.z.σ2, var)
        mean_j, cov_j = gp.predict_joint(pa, additive_level=level)
        assert same_bits((mean_j, cov_j), eng.predict_joint(pa, with_noise=True, jitter=0.0, terms=sel))
        assert np.array_equal(gp.predict_grad(pa, additive_level=level), eng.predict_grad(pa, terms=sel))
    assert gp.predict_points_grad(pts, additive_level="g").names == ["|∇|y"]

    parts = gp.decompose_points(pts)
    assert list(parts) == ["total", "global", "g"] and gp.component_levels == ["global", "g"]
    assert gp.component_cov.shape == (2, 2, M)
    means, cov, _ = eng.predict_decompose(pa)
    assert np.array_equal(gp.component_cov, cov)
    for t, level in enumerate(["global", "g"]):
        assert round_trip(parts[level].z.μ, means[t]) and round_trip(parts[level].z.σ2, cov[t, t])
    total = gp.predict_points(pts, with_noise=False)
    assert close_to(np.asarray(parts["total"].z.μ), np.asarray(total.z.μ), "front end total mean") <= 1e-10
    assert abs_err(np.asarray(parts["total"].z.σ2), np.asarray(total.z.σ2), "front end total variance") <= 1e-9

    z = np.random.default_rng(9).standard_normal((2, M))
    draws = gp.draw_point_samples(pts, additive_level="g", n_draws=2, z=z)
    want = eng.draw_joint(pa, z, with_noise=False, jitter=float(gp.model.spec.jitter), terms=(1,))
    assert draws.shape == (2, M) and round_trip(draws.z.values(), want)
    with pytest.raises(ValueError, match="total.*global.*g"):
        gp.predict_points(pts, additive_level="h")
