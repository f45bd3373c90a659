"""Averages of the posterior over groups of points on the MI355X: ``gmb_predict_groups`` / ``gmb_predict_groups_terms`` and the front
end above them against the numpy yardstick of tests/group_average_reference.py -- the DEFINITION ``W mu``, ``W C W^T`` on the full
joint posterior of all the points, which the engine never forms.  Needs a GPU (``-m gpu``).

Shapes: the Matern-5/2 table (N = 700: six block columns, the last ragged) at cond 3e3 and 4.5e5 and the three-term additive
model (N = 300: coregion tables, two outputs, hetero noise, a linear dimension -- the kernels' general path and the term walk).
Groups of sizes [1, 2, 127, 128, 129, 2 GROUP_CHUNK + 1, 300, 64, 5, 131] (M = 1912: one point, a staged piece of 128 and its
neighbours, three tasks of one group, partial column blocks) and 130 groups of 1 - 3 points (G across a 128-row tile of C, a second
row block of the Q pass).  Weights: explicit plain means, NULL, and a contrast (half of the longest group negated).  States: behind
``factorize`` (the solve form) and behind ``evaluate(theta, grad=True)`` (the product form over the resident U).

Bars -- the suite's joint-posterior bars (tests/test_gpu_joint.py, tests/test_gpu_components.py), scaled by the weights' 1-norms
because the quantity is linear in C:

* means: 1e-8 max|ref|;
* variances and covariances: 1e-9 max(1, ||w_g||_1 ||w_h||_1) absolute, entry by entry;
* two GPU results that are the same quantity by different launches: 1e-10 relative;
* NULL against explicit weights, a call repeated, cov's diagonal against var, cov against its transpose: bit-identical.

The yardstick's own two forms agree to 2e-12 / 4e-14 on these problems (tests/test_group_average_cpu.py), three orders inside the
bars.  Measured errors are printed per test (``GROUP-AVERAGE ...``); the worst seen on an MI355X: means 3.3e-12 relative (cond
4.5e5), variances and covariances 6.9e-13.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abi_forms as AF
import group_average_reference as GA
from oracle import gp_oracle as O
from test_gpu_abi_forms import FORMS, mat_in, mat_out, sync, take, take_vec, vec_in, vec_out
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

STATES = ["solve", "product"]


@contextlib.contextmanager
def engine_in(name, state):
    spec, theta, X, y = GA.problem(name)
    with make_engine(spec, theta, X, y) as eng:
        if state == "solve":
            eng.factorize()
        else:
            eng.evaluate(theta, grad=True)
        yield eng


def takes_product_form(eng, X):
    eng.predict(X[:3])
    return eng.timings()["predict_gemm_form"] == 1


def rel_err(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
    print(f"GROUP-AVERAGE {what}: max |got - ref| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    return err / scale


def cov_err(got, ref, norms, what):
    """max over the entries of |got - ref| / max(1, ||w_g||_1 ||w_h||_1); ``norms`` per group, vectors take the diagonal's."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = np.maximum(1.0, np.outer(norms, norms) if got.ndim == 2 else np.asarray(norms) ** 2)
    err = float(np.max(np.abs(got - ref) / scale))
    print(f"GROUP-AVERAGE {what}: max |got - ref| / max(1, |w_g| |w_h|) = {err:.3e}")
    return err


def same_bits(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- 1. against the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", GA.PROBLEMS)
def test_against_the_definition(gpu, name, state):
    X = GA.problem(name)[2]
    with engine_in(name, state) as eng:
        for which in ("sizes", "many"):
            Xs, offsets = GA.points(name, which)
            results = {}
            for kind in GA.WEIGHTS:
                w = GA.weights_of(name, which, kind)
                mean_r, cov_r = GA.reference(name, which, "mean" if kind == "null" else kind)
                norms = GA.weight_norms(offsets, w)
                mean, var, cov = results[kind] = eng.predict_groups(Xs, offsets, w, cov=True)
                what = f"{name} {state} {which} (G = {len(offsets) - 1}, M = {len(Xs)}) {kind}"
                assert rel_err(mean, mean_r, what + " mean") <= 1e-8
                assert cov_err(var, np.diag(cov_r), norms, what + " var") <= 1e-9
                assert cov_err(cov, cov_r, norms, what + " cov") <= 1e-9
                assert np.array_equal(cov, cov.T), what + ": cov is not exactly symmetric"
                assert np.array_equal(np.diag(cov), var), what + ": cov's diagonal is not var"
                assert same_bits(eng.predict_groups(Xs, offsets, w, cov=True), results[kind]), what + ": a second call differs"
                # the diagonal-only Q path (no covariance asked for) against the full one
                mean_d, var_d = eng.predict_groups(Xs, offsets, w)
                assert same_bits(mean_d, mean), what + ": the mean depends on cov"
                assert rel_err(var_d, var, what + " var without cov against var with cov") <= 1e-10
            assert same_bits(results["null"], results["mean"]), f"{name} {state} {which}: NULL weights differ from explicit 1 / |g|"
        assert takes_product_form(eng, X) == (state == "product")


@pytest.mark.parametrize("kind", list(O.KINDS))
@pytest.mark.parametrize("d", [1, 2, 3, 5, 9])
def test_every_kind_and_width_against_the_definition(gpu, kind, d):
    """group_cov_partial_kernel<KIND, NC, false> for every kind at every padded width 1, 2, 4, 8, 16 (the general form
    is the three-term model's above).  N = 200 (two block columns, the second ragged), three groups of 1, 5 and 64 points (M = 70)
    0.3 off training rows, plain means; eta = 1.1, sigma = 0.25: cond(Sigma) <= 1 + N eta^2 / sigma^2 = 3.9e3, below the Matern
    table's, so the bars are the ones above."""
    N = 200
    X, y, ls = O.synthetic_table(N, d, seed=1000 * d + N)
    spec = O.make_spec(d, range(d), kind=kind)
    theta = O.pack_theta(spec, ls, 1.1, 0.25)
    offsets = GA.offsets_of([1, 5, 64])
    rng = np.random.default_rng(17)
    Xs = X[rng.integers(0, N, int(offsets[-1]))] + 0.3 * rng.standard_normal((int(offsets[-1]), d))
    mean_r, cov_r = GA.by_joint(spec, theta, X, y, Xs, offsets, None)
    norms = GA.weight_norms(offsets, None)
    with make_engine(spec, theta, X, y) as eng:
        eng.factorize()
        mean, var, cov = eng.predict_groups(Xs, offsets, None, cov=True)
    what = f"{kind} d = {d}"
    assert rel_err(mean, mean_r, what + " mean") <= 1e-8
    assert cov_err(var, np.diag(cov_r), norms, what + " var") <= 1e-9
    assert cov_err(cov, cov_r, norms, what + " cov") <= 1e-9


# ---- 2. engine against engine on the same factor -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", ["matern", "three_term"])
def test_against_the_engines_own_predictions(gpu, name, state):
    with engine_in(name, state) as eng:
        Xs, offsets = GA.points(name, "many")
        # every point a group of its own, weight 1: gmb_predict(with_noise = 0)
        M = len(Xs)  # (about 260: G crosses a 128-row tile and the Q pass takes a third row block)
        singles = np.arange(M + 1, dtype=np.int64)
        mean, var = eng.predict_groups(Xs[:M], singles, np.ones(M))
        mu_p, var_p = eng.predict(Xs[:M], with_noise=False)
        assert rel_err(mean, mu_p, f"{name} {state} one-point groups mean against predict") <= 1e-10
        assert rel_err(var, var_p, f"{name} {state} one-point groups var against predict") <= 1e-10
        # W C W^T from the engine's own joint posterior at the same points
        for kind in ("mean", "signed"):
            w = GA.weights_of(name, "many", kind)
            W = GA.weight_matrix(offsets, w)
            mu_j, C_j = eng.predict_joint(Xs, with_noise=False, jitter=0.0)
            mean, var, cov = eng.predict_groups(Xs, offsets, w, cov=True)
            assert rel_err(mean, W @ mu_j, f"{name} {state} {kind} mean against W mu of predict_joint") <= 1e-10
            assert rel_err(cov, W @ C_j @ W.T, f"{name} {state} {kind} cov against W C W^T of predict_joint") <= 1e-10
            assert rel_err(var, np.diag(W @ C_j @ W.T), f"{name} {state} {kind} var against W C W^T of predict_joint") <= 1e-10


# ---- 3. selections of an additive model's terms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
def test_term_selections(gpu, state):
    name = "three_term"
    Xs, offsets = GA.points(name, "many")
    w = GA.weights_of(name, "many", "signed")
    norms = GA.weight_norms(offsets, w)
    with engine_in(name, state) as eng:
        assert eng.num_terms == 3
        total = eng.predict_groups(Xs, offsets, w, cov=True)
        for terms in (0b001, 0b101, 0b111):
            mean_r, cov_r = GA.reference(name, "many", "signed", terms)
            mean, var, cov = eng.predict_groups(Xs, offsets, w, cov=True, terms=terms)
            what = f"three_term {state} terms = {terms:#05b}"
            assert rel_err(mean, mean_r, what + " mean") <= 1e-8
            assert cov_err(var, np.diag(cov_r), norms, what + " var") <= 1e-9
            assert cov_err(cov, cov_r, norms, what + " cov") <= 1e-9
            assert np.array_equal(cov, cov.T)
        assert rel_err(mean, total[0], f"three_term {state} all terms against the call without a selection, mean") <= 1e-10
        assert rel_err(cov, total[2], f"three_term {state} all terms against the call without a selection, cov") <= 1e-10
        parts = [eng.predict_groups(Xs, offsets, w, terms=1 << t)[0] for t in range(3)]
        assert rel_err(parts[0] + parts[1] + parts[2], total[0], f"three_term {state} single-term means summed") <= 1e-10


def test_front_end_level_is_a_term_selection(gpu):
    import gumbi_amd as gmb
    from test_gpu_components import additive_dataset, round_trip

    gp = gmb.GP(additive_dataset(), outputs="y")
    gp.specify_model(continuous_dims=["a", "b"], categorical_dims="g", additive=True)
    gp.build_model()
    theta = np.abs(np.random.default_rng(2).normal(1.0, 0.2, gp.model.spec.theta_size())) + 0.3
    gp.find_MAP(theta=theta)
    kwargs = {"resolution": 6, "n_background": 50, "seed": 3}
    pred = gp.predict_marginal("a", joint=True, additive_level="global", **kwargs)
    design = gp.marginal_design("a", **kwargs)
    mean, var, cov = gp.engine.predict_groups(design["points_array"], design["offsets"], design["weights"], cov=True, terms=1)
    assert pred.shape == (6,) and round_trip(pred.z.μ, mean) and round_trip(pred.z.σ2, var) and np.array_equal(gp.marginal_cov, cov)
    whole = gp.predict_marginal("a", **kwargs)
    assert not np.allclose(np.asarray(whole.z.μ), np.asarray(pred.z.μ), rtol=1e-6, atol=0)
    ab = gp.compare_levels("g", "u", "w", n_background=50, seed=3)
    ba = gp.compare_levels("g", "w", "u", n_background=50, seed=3)
    assert abs(ab["mean"] + ba["mean"]) <= 1e-10 * abs(ab["mean"]) and abs(ab["var"] - ba["var"]) <= 1e-10 * ab["var"] and ab["var"] > 0.0


# ---- 4. state contract ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
def test_calls_leave_the_engine_as_found(gpu, state):
    name = "matern"
    X = GA.problem(name)[2]
    Xp = X[::9] + 0.05
    Xs, offsets = GA.points(name, "sizes")
    Xm, offsets_m = GA.points(name, "many")
    with engine_in(name, state) as eng:
        def snapshot():
            snap = (eng.copy_factor(0, 128, 0, 128), eng.copy_factor(640, 60, 256, 444), eng.copy_v())
            snap += eng.predict(Xp)
            form = eng.timings()["predict_gemm_form"]
            snap += eng.predict_joint(Xp, with_noise=True, jitter=0.0)
            if state == "product":
                snap += (eng.copy_alpha(),)
            return snap, form

        assert eng.factor_is_current()
        before, form = snapshot()
        assert form == (1 if state == "product" else 0)
        calls = [("groups", lambda: eng.predict_groups(Xs, offsets)), ("groups cov", lambda: eng.predict_groups(Xm, offsets_m, cov=True)),
                 ("groups signed", lambda: eng.predict_groups(Xs, offsets, GA.weights_of(name, "sizes", "signed"), cov=True))]
        first = {}
        for label, call in calls:
            first[label] = call()
            assert same_bits(call(), first[label]), f"{state}: two consecutive {label} calls differ"
            assert eng.factor_is_current(), f"{state}: the factor is not current behind {label}"
            after, form_after = snapshot()
            assert same_bits(after, before), f"{state}: factor / v / alpha / predict / predict_joint changed behind {label}"
            assert form_after == form, f"{state}: predict changed its form behind {label}"
        for label, call in reversed(calls):
            assert same_bits(call(), first[label]), f"{state}: {label} differs between its two rounds"


# ---- 5. call forms ------------------------------------------------------------------------------------------------------------------------
def raw_call(eng, Xs, offsets, weights, form, cov=True, var=True, terms=None):
    M, G = Xs.shape[0], len(offsets) - 1
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    x = mat_in(Xs, form, 3)
    w = vec_in(weights, form) if weights is not None else None
    mean, v, c = vec_out(G, form), vec_out(G, form) if var else None, mat_out(G, G, form, 5) if cov else None
    sync()
    tail = (x.ptr, M, x.ld, off.ctypes.data_as(C.c_void_p), G, w.ptr if w else None, mean.ptr, v.ptr if v else None, c.ptr if c else None,
            c.ld if c else 0, form.memspace)
    if terms is None:
        rc = eng._lib.gmb_predict_groups(eng._h, *tail)
    else:
        rc = eng._lib.gmb_predict_groups_terms(eng._h, terms, *tail)
    assert rc == 0, (form.name, rc)
    what = f"gmb_predict_groups ({form.name})"
    out = (take_vec(mean, G, what + " mean"),)
    if var:
        out += (take_vec(v, G, what + " var"),)
    if cov:
        out += (take(c, G, G, what + " cov"),)
    return out


@pytest.mark.parametrize("state", STATES)
def test_call_forms(gpu, state):
    """``Xs`` with ``ldxs > D`` (NaN padding), ``ldc > G``, every array but the offsets in device memory: the same bits as the packed
    host call, the padding and everything behind the outputs' last elements untouched."""
    name = "three_term"
    Xs, offsets = GA.points(name, "many")
    w = GA.weights_of(name, "many", "signed")
    with engine_in(name, state) as eng:
        want = eng.predict_groups(Xs, offsets, w, cov=True)
        want_null = eng.predict_groups(Xs, offsets, None, cov=True)
        want_sel = eng.predict_groups(Xs, offsets, w, cov=True, terms=0b101)
        for form in FORMS:
            assert same_bits(raw_call(eng, Xs, offsets, w, form), want), f"{form.name}: differs from the packed host call"
            assert same_bits(raw_call(eng, Xs, offsets, None, form), want_null), f"{form.name}: NULL weights differ"
            assert same_bits(raw_call(eng, Xs, offsets, w, form, terms=0b101), want_sel), f"{form.name}: the selection differs"
            # var may be NULL when cov is not, cov may be NULL
            assert same_bits(raw_call(eng, Xs, offsets, w, form, var=False), (want[0], want[2]))
            assert same_bits(raw_call(eng, Xs, offsets, w, form, cov=False), want[:2])


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------
def poisoned_call(eng, Xs, offsets, G=None, M=None, weights=None, ldxs=None, ldc=None, terms=None, null=()):
    """``(status, outputs still poisoned)`` of a raw host call."""
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    G = len(off) - 1 if G is None else G
    k = max(len(off), 2)
    mean, var = AF.padded(k, AF.SPARE, AF.FILL), AF.padded(k, AF.SPARE, AF.FILL)
    cov = AF.embed(np.full((k, k), AF.FILL), k, AF.FILL)
    wts = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    tail = (None if "Xs" in null else ptr(Xs), Xs.shape[0] if M is None else M, Xs.shape[1] if ldxs is None else ldxs,
            None if "offsets" in null else ptr(off), G, None if wts is None else ptr(wts), None if "mean" in null else ptr(mean),
            None if "var" in null else ptr(var), None if "cov" in null else ptr(cov), k if ldc is None else ldc, 0)
    rc = eng._lib.gmb_predict_groups(eng._h, *tail) if terms is None else eng._lib.gmb_predict_groups_terms(eng._h, terms, *tail)
    clean = AF.untouched(mean, 0, AF.FILL_BITS) and AF.untouched(var, 0, AF.FILL_BITS) and AF.untouched(cov, 0, AF.FILL_BITS, rows=0)
    return rc, clean


def test_bad_arguments_are_refused_and_write_nothing(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    name = "three_term"
    Xs, offsets = GA.points(name, "many")
    Xs, offsets = Xs[:offsets[6]], offsets[:7]
    M = len(Xs)
    with engine_in(name, "solve") as eng:
        before = (eng.copy_v(),) + eng.predict_groups(Xs, offsets, cov=True)
        empty = offsets.copy()
        empty[3] = empty[2]
        backwards = offsets.copy()
        backwards[3] = backwards[2] - 1
        shifted = offsets.copy()
        shifted[0] = 1
        nan_w = np.full(M, 0.1)
        nan_w[M // 2] = np.nan
        inf_w = np.full(M, 0.1)
        inf_w[-1] = np.inf
        bad = [("an empty group", {"offsets": empty}), ("offsets run backwards", {"offsets": backwards}),
               ("offsets start at 1", {"offsets": shifted}), ("a wrong last offset", {"M": M - 1}), ("M beyond the last offset", {"M": M + 1}),
               ("ldc < G", {"ldc": 5}), ("G = 0", {"G": 0}), ("G < 0", {"G": -2}), ("ldxs < D", {"ldxs": Xs.shape[1] - 1}),
               ("a NaN weight", {"weights": nan_w}), ("an infinite weight", {"weights": inf_w}),
               ("null Xs", {"null": ("Xs",)}), ("null offsets", {"null": ("offsets",)}), ("null mean", {"null": ("mean",)}),
               ("neither var nor cov", {"null": ("var", "cov")}),
               ("terms = 0", {"terms": 0}), ("a term bit beyond T", {"terms": 0b1001})]
        for label, kw in bad:
            kw = dict(kw)
            rc, clean = poisoned_call(eng, Xs, kw.pop("offsets", offsets), **kw)
            assert rc == GMB_EINVAL, f"{label}: status {rc}"
            assert clean, f"{label}: outputs were written"
        assert poisoned_call(eng, Xs, offsets)[0] == 0 and poisoned_call(eng, Xs, offsets, terms=0b111)[0] == 0
        with pytest.raises(ValueError, match="empty"):
            eng.predict_groups(Xs, empty)
        with pytest.raises(ValueError, match="not M"):
            eng.predict_groups(Xs[:-1], offsets)
        with pytest.raises(ValueError, match="not finite"):
            eng.predict_groups(Xs, offsets, nan_w)
        with pytest.raises(ValueError, match="weights for"):
            eng.predict_groups(Xs, offsets, nan_w[:-1])
        assert eng.factor_is_current()
        assert same_bits((eng.copy_v(),) + eng.predict_groups(Xs, offsets, cov=True), before)


def test_engines_without_a_usable_single_factor_refuse(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    name = "three_term"
    spec, theta, X, y = GA.problem(name)
    Xs, offsets = GA.points(name, "many")
    Xs, offsets = Xs[:offsets[6]], offsets[:7]
    with make_engine(spec, theta, X, y) as eng:
        def refused(label):
            for rc, clean in (poisoned_call(eng, Xs, offsets), poisoned_call(eng, Xs, offsets, terms=1)):
                assert rc == GMB_EINVAL and clean, f"{label}: status {rc}, outputs clean {clean}"

        refused("before gmb_factorize")
        eng.factorize()
        assert poisoned_call(eng, Xs, offsets)[0] == 0
        eng.set_theta(theta * 1.01)
        refused("after gmb_set_theta")
        eng.factorize()
        # (a CONSUMED factor is joint_ready's refusal, shared with gmb_predict_joint; a single engine holds that state only while a
        # gradient is in flight -- tests/test_gpu_append.py -- so behind a gradient call the factor is either current or refused)
        eng.nlml(grad=True)
        if eng.factor_is_current():
            assert poisoned_call(eng, Xs, offsets)[0] == 0
        else:
            refused("on a consumed factor")
        eng.factorize()
        assert poisoned_call(eng, Xs, offsets)[0] == 0
        eng.set_dist_mode(eng.DIST_CAPACITY)
        refused("capacity mode")
        with pytest.raises(ValueError):
            eng.predict_groups(Xs, offsets)


# ---- 7. the front end ---------------------------------------------------------------------------------------------------------------------
def test_front_end_on_the_device(gpu, monkeypatch):
    """``predict_marginal(["X"])`` of the fitted example against the same call over the oracle engine at the same theta."""
    from test_gpu_frontend import example_gp

    gp = example_gp().fit(continuous_dims=["X", "Y"], MAP_kwargs={"maxeval": 30})
    pred = gp.predict_marginal(["X"], resolution=12, joint=True)
    cov = gp.marginal_cov
    assert pred.shape == (12,) and cov.shape == (12, 12) and np.array_equal(cov, cov.T)
    assert gp.marginal_points.names == ["X"] and gp.marginal_points.shape == (12,)

    GA.use_group_oracle(monkeypatch)
    ref = example_gp()
    ref.specify_model(continuous_dims=["X", "Y"])
    ref.build_model()
    ref.find_MAP(theta=gp._theta_fitted)
    assert isinstance(ref.engine, GA.GroupOracleEngine)
    pred_r = ref.predict_marginal(["X"], resolution=12, joint=True)
    assert rel_err(np.asarray(pred.z.μ), np.asarray(pred_r.z.μ), "front end marginal mean") <= 1e-8
    ones = np.ones(12)
    assert cov_err(np.asarray(pred.z.σ2), np.asarray(pred_r.z.σ2), ones, "front end marginal var") <= 1e-9
    assert cov_err(cov, ref.marginal_cov, ones, "front end marginal cov") <= 1e-9
    # the variance of the average is not the mean of the pointwise variances
    design = gp.marginal_design(["X"], resolution=12)
    _, var_pts = gp.engine.predict(design["points_array"], with_noise=False)
    naive = var_pts.reshape(12, -1).mean(axis=1)
    print("GROUP-AVERAGE mean of the pointwise variances / variance of the average:", np.array2string(naive / np.asarray(pred.z.σ2), precision=3))
    assert np.all(naive > np.asarray(pred.z.σ2))
