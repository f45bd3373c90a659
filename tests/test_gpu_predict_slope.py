"""``gmb_predict_slope`` -- the posterior of the slope ``d f / d x*``: mean, variance and covariance of the partial derivatives -- on
the MI355X against the closed form of tests/slope_reference.py (itself held against ``grad_reference.mean_grad``, the literal prior
curvatures and finite differences of the oracle's joint covariance by tests/test_predict_slope_cpu.py).  Needs a GPU (``-m gpu``).

Shapes, the smallest that reach every path: Matern-5/2, N = 700, d = 3 (six block columns, the last ragged, three columns padded to
four) at the suite's two noise levels (cond about 3e3 and 4.5e5); Matern-3/2, N = 200, d = 1; the three-term additive model
(N = 300: coregion tables, two outputs, hetero noise, a linear dimension -- the kernel's general path and the term walk);
``Periodic`` and ``Matern52+Periodic``, N = 200, d = 2.  M in {1, 129, 200}; behind ``factorize`` and behind
``evaluate(theta, grad=True)``.

Bars:

* ``dmean`` against the reference, and against ``gmb_predict_grad`` on the same state (two algorithms for one quantity):
  ``1e-8 max|ref|`` -- the suite's bar for means;
* ``dvar`` / ``dcov`` against the reference: ``1e-9 max(1, max_d P_dd)`` absolute -- the suite's covariance bar scaled by the size of
  the two terms whose difference the result is;
* per-level slopes of the additive model summed against the total's: 1e-10 relative;
* a repeated call, ``dcov``'s diagonal against ``dvar``, ``dcov[m]`` against its transpose, ``dvar`` with and without ``dcov``, the
  categorical columns' zeros, the points behind an M-tile against the same points sent alone, every call form against the packed
  host call, the engine's state before and after: bit-identical.

Measured errors are printed per test (``SLOPE ...``); the worst seen on an MI355X: means 4.1e-12 of max|ref| (cond 4.5e5; 1.4e-12
against ``gmb_predict_grad``), variances and covariances 5.4e-14 of max(1, max P).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abi_forms as AF
import slope_reference as SR
from oracle import gp_oracle as O
from test_gpu_abi_forms import FORMS, mat_in, mat_out, sync, take
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

STATES = ["solve", "product"]


@contextlib.contextmanager
def engine_for(spec, theta, X, y, periodic=0, periods=None, state=None):
    if periodic:
        from test_gpu_periodic import make_engine as periodic_engine

        eng = periodic_engine(spec, periodic, periods, theta, X, y)
    else:
        eng = make_engine(spec, theta, X, y)
    with eng:
        if state == "solve":
            eng.factorize()
        elif state == "product":
            eng.evaluate(theta, grad=True)
        yield eng


def engine_in(name, state):
    return engine_for(*SR.problem(name), state=state)


def mean_err(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
    print(f"SLOPE {what}: max |got - ref| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    return err / scale


def cov_err(got, ref, scale, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.max(np.abs(got - ref)))
    print(f"SLOPE {what}: max |got - ref| = {err:.3e}, max(1, max P) = {scale:.3e}, ratio {err / scale:.2e}")
    return err / scale


def same_bits(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def check_structure(out, spec, what):
    """What holds bit for bit of any ``(dmean, dvar, dcov)``."""
    dmean, dvar, dcov = out
    D = dmean.shape[1]
    idx = np.arange(D)
    assert np.array_equal(dcov, np.swapaxes(dcov, 1, 2)), what + ": dcov is not exactly symmetric"
    assert np.array_equal(dcov[:, idx, idx], dvar), what + ": dcov's diagonal is not dvar"
    flat = [c for c in range(D) if c not in SR.cont_columns(spec)]
    assert not np.any(dmean[:, flat]) and not np.any(dvar[:, flat]), what + ": a column without a derivative is not 0"
    assert not np.any(dcov[:, flat, :]) and not np.any(dcov[:, :, flat]), what + ": dcov of a column without a derivative is not 0"


# ---- 1. against the reference, and against gmb_predict_grad ---------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", SR.PROBLEMS)
def test_against_the_reference(gpu, name, state):
    spec = SR.problem(name)[0]
    with engine_in(name, state) as eng:
        for M in SR.POINT_COUNTS:
            Xs = SR.points(name, M)
            dmean_r, dvar_r, dcov_r = SR.reference(name, M)
            scale = SR.p_scale(name, M)
            out = dmean, dvar, dcov = eng.predict_slope(Xs, cov=True)
            what = f"{name} {state} M = {M}"
            assert mean_err(dmean, dmean_r, what + " dmean") <= 1e-8
            assert cov_err(dvar, dvar_r, scale, what + " dvar") <= 1e-9
            assert cov_err(dcov, dcov_r, scale, what + " dcov") <= 1e-9
            check_structure(out, spec, what)
            assert same_bits(eng.predict_slope(Xs, cov=True), out), what + ": a second call differs"
            assert same_bits(eng.predict_slope(Xs), (dmean, dvar)), what + ": dmean / dvar depend on whether dcov is asked for"
            G = eng.predict_grad(Xs)
            assert mean_err(dmean, G, what + " dmean against gmb_predict_grad") <= 1e-8
        eng.predict(SR.points(name, 129)[:3])
        assert eng.timings()["predict_gemm_form"] == (1 if state == "product" else 0)


@pytest.mark.parametrize("kind", ["ExpQuad", "Matern52", "Matern32"])
@pytest.mark.parametrize("d", [1, 2, 3, 5, 9])
def test_every_kind_and_width_against_the_reference(gpu, kind, d):
    """slope_cross_cov_kernel<KIND, NC, false> for every kind with a derivative process at every padded width 1, 2, 4, 8, 16 (DESIGN
    2.4; the general form is the three-term model's above).  N = 200 (two block columns, the second ragged), M = 70 points 0.3 off
    training rows; eta = 1.1, sigma = 0.25: cond(Sigma) <= 1 + N eta^2 / sigma^2 = 3.9e3, below the N = 700 table's bound, so the
    bars are the ones above."""
    N, M = 200, 70
    X, y, ls = O.synthetic_table(N, d, seed=1000 * d + N)
    spec = O.make_spec(d, range(d), kind=kind)
    theta = O.pack_theta(spec, ls, 1.1, 0.25)
    rng = np.random.default_rng(M)
    Xs = X[rng.integers(0, N, M)] + 0.3 * rng.standard_normal((M, d))
    dmean_r, dvar_r, dcov_r = SR.posterior(spec, theta, X, y, Xs)
    scale = max(1.0, float(np.max(np.abs(SR.prior_curvature(spec, theta, X, Xs)))))
    with engine_for(spec, theta, X, y, state="solve") as eng:
        out = dmean, dvar, dcov = eng.predict_slope(Xs, cov=True)
    what = f"{kind} d = {d}"
    assert mean_err(dmean, dmean_r, what + " dmean") <= 1e-8
    assert cov_err(dvar, dvar_r, scale, what + " dvar") <= 1e-9
    assert cov_err(dcov, dcov_r, scale, what + " dcov") <= 1e-9
    check_structure(out, spec, what)


# ---- 2. selections of an additive model's terms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
def test_term_selections(gpu, state):
    name, M = "three_term", 129
    spec = SR.problem(name)[0]
    Xs = SR.points(name, M)
    with engine_in(name, state) as eng:
        assert eng.num_terms == 3
        total = eng.predict_slope(Xs, cov=True)
        for terms in (0b001, 0b101, 0b110, 0b111):
            dmean_r, dvar_r, dcov_r = SR.reference(name, M, terms)
            scale = SR.p_scale(name, M, terms)
            out = dmean, dvar, dcov = eng.predict_slope(Xs, cov=True, terms=terms)
            what = f"three_term {state} terms = {terms:#05b}"
            assert mean_err(dmean, dmean_r, what + " dmean") <= 1e-8
            assert cov_err(dvar, dvar_r, scale, what + " dvar") <= 1e-9
            assert cov_err(dcov, dcov_r, scale, what + " dcov") <= 1e-9
            check_structure(out, spec, what)
            assert mean_err(dmean, eng.predict_grad(Xs, terms=terms), what + " dmean against gmb_predict_grad_terms") <= 1e-8
        assert same_bits(out, total), "all terms selected differs from the call without a selection"
        levels = [eng.predict_slope(Xs, terms=1 << t)[0] for t in range(3)]
        assert mean_err(levels[0] + levels[1] + levels[2], total[0], f"three_term {state} per-level means summed") <= 1e-10
        mu, _ = eng.predict(Xs)  # term 0's preparation of the training points is back in place
        assert same_bits(mu, eng.predict(Xs)[0])


# ---- 3. M-tiles -----------------------------------------------------------------------------------------------------------------------------
def test_points_behind_an_m_tile(gpu):
    """M = one M-tile + 130 on the N = 700 problem (Np = 768, Dc = 3: 10880 + 130 points): the points beyond the tile equal the same
    points sent alone, bit for bit; those before it meet the bars (every 16th against the reference)."""
    from gumbi_amd.engine import slope_tile_rows

    name = "matern52"
    spec, theta, X, y, _, _ = SR.problem(name)
    Mt = slope_tile_rows(768, 3)
    assert Mt == 10880
    Xs = SR.points(name, Mt + 130)
    with engine_in(name, "solve") as eng:
        out = eng.predict_slope(Xs, cov=True)
        tail = eng.predict_slope(Xs[Mt:], cov=True)
        assert same_bits(tuple(a[Mt:] for a in out), tail), "the points behind the M-tile differ from the same points sent alone"
        assert same_bits(eng.predict_slope(Xs)[1], out[1])
    head = Xs[:Mt:16]
    dmean_r, dvar_r, dcov_r = SR.posterior(spec, theta, X, y, head)
    scale = max(1.0, float(np.max(SR.prior_curvature(spec, theta, X, head))))
    assert mean_err(out[0][:Mt:16], dmean_r, "first M-tile dmean") <= 1e-8
    assert cov_err(out[1][:Mt:16], dvar_r, scale, "first M-tile dvar") <= 1e-9
    assert cov_err(out[2][:Mt:16], dcov_r, scale, "first M-tile dcov") <= 1e-9
    check_structure(out, spec, "M = tile + 130")


# ---- 4. call forms ----------------------------------------------------------------------------------------------------------------------
def raw_call(eng, Xs, form, var=True, cov=True, terms=None):
    M, D = Xs.shape
    x = mat_in(Xs, form, 3)
    dm, dv, dc = mat_out(M, D, form, 3), mat_out(M, D, form, 3) if var else None, mat_out(M, D * D, form, 5) if cov else None
    sync()
    tail = (x.ptr, M, x.ld, dm.ptr, dv.ptr if var else None, dm.ld, dc.ptr if cov else None, dc.ld if cov else 0, form.memspace)
    rc = eng._lib.gmb_predict_slope(eng._h, *tail) if terms is None else eng._lib.gmb_predict_slope_terms(eng._h, terms, *tail)
    assert rc == 0, (form.name, rc)
    what = f"gmb_predict_slope ({form.name})"
    out = (take(dm, M, D, what + " dmean"),)
    if var:
        out += (take(dv, M, D, what + " dvar"),)
    if cov:
        out += (take(dc, M, D * D, what + " dcov").reshape(M, D, D),)
    return out


@pytest.mark.parametrize("state", STATES)
def test_call_forms(gpu, state):
    """``Xs`` with ``ldxs > D`` (NaN padding), ``ldg > D``, ``ldc > D * D``, every array in device memory: the same bits as the packed
    host call, the padding and everything behind the outputs' last rows untouched; ``dvar`` and ``dcov`` may be NULL."""
    name = "three_term"
    Xs = np.array(SR.points(name, 129))
    with engine_in(name, state) as eng:
        want = eng.predict_slope(Xs, cov=True)
        want_sel = eng.predict_slope(Xs, cov=True, terms=0b101)
        for form in FORMS:
            assert same_bits(raw_call(eng, Xs, form), want), f"{form.name}: differs from the packed host call"
            assert same_bits(raw_call(eng, Xs, form, terms=0b101), want_sel), f"{form.name}: the selection differs"
            assert same_bits(raw_call(eng, Xs, form, var=False), (want[0], want[2])), f"{form.name}: NULL dvar"
            assert same_bits(raw_call(eng, Xs, form, cov=False), want[:2]), f"{form.name}: NULL dcov"
            assert same_bits(raw_call(eng, Xs, form, var=False, cov=False), want[:1]), f"{form.name}: the mean alone"


# ---- 5. state contract ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", ["matern52", "three_term"])
def test_calls_leave_the_engine_as_found(gpu, name, state):
    Xs = SR.points(name, 200)
    Xp = SR.points(name, 129)

    def snapshot(eng):
        mu, var = eng.predict(Xp)
        form = eng.timings()["predict_gemm_form"]
        val, g = eng.nlml(grad=True)
        return (mu, var, np.float64(val), g), form, eng.factor_is_current()

    def prepare(eng):
        if state == "solve":
            eng.factorize()
        else:
            eng.evaluate(SR.problem(name)[1], grad=True)

    with engine_in(name, None) as eng:
        prepare(eng)
        before, form, current = snapshot(eng)
        assert current and form == (1 if state == "product" else 0)
        prepare(eng)
        first = eng.predict_slope(Xs, cov=True)
        assert eng.factor_is_current()
        eng.predict(Xp)
        assert eng.timings()["predict_gemm_form"] == form, f"{state}: predict changed its form behind predict_slope"
        assert same_bits(eng.predict_slope(Xs, cov=True), first)
        after, form_after, current_after = snapshot(eng)
        assert same_bits(after, before), f"{state}: predict / nlml / its gradient changed behind predict_slope"
        assert form_after == form and current_after


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def poisoned_call(eng, Xs, M=None, ldxs=None, ldg=None, ldc=None, terms=None, null=()):
    """``(status, outputs still poisoned)`` of a raw host call."""
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Xs = np.ascontiguousarray(Xs, dtype=np.float64)
    n, D = Xs.shape
    dm, dv = AF.embed(np.full((n, D), AF.FILL), D, AF.FILL), AF.embed(np.full((n, D), AF.FILL), D, AF.FILL)
    dc = AF.embed(np.full((n, D * D), AF.FILL), D * D, AF.FILL)
    tail = (None if "Xs" in null else ptr(Xs), n if M is None else M, D if ldxs is None else ldxs, None if "dmean" in null else ptr(dm),
            ptr(dv), D if ldg is None else ldg, ptr(dc), D * D if ldc is None else ldc, 0)
    rc = eng._lib.gmb_predict_slope(eng._h, *tail) if terms is None else eng._lib.gmb_predict_slope_terms(eng._h, terms, *tail)
    clean = all(AF.untouched(b, 0, AF.FILL_BITS, rows=0) for b in (dm, dv, dc))
    return rc, clean, (eng._lib.gmb_last_error(eng._h) or b"").decode()


def test_kernels_without_a_derivative_are_refused(gpu):
    from gumbi_amd.engine import GMB_EINVAL
    from oracle import gp_oracle as O

    X, y, ls = O.synthetic_table(200, 2, seed=8)
    spec = O.make_spec(2, range(2), kind="Matern12")
    spec3, theta3, X3, y3, _, _ = SR.problem("three_term")
    cases = [("Matern-1/2", spec, O.pack_theta(spec, ls, 1.1, 0.25), X, y, [None]),
             ("additive Exponential", dict(spec3, kind=O.KINDS["Exponential"]), theta3, X3, y3, [None, 0b010, 0b101])]
    for label, sp, th, XX, yy, selections in cases:
        with engine_for(sp, th, XX, yy, state="solve") as eng:
            before = eng.predict(XX[:50])
            for terms in selections:
                rc, clean, msg = poisoned_call(eng, XX[:50], terms=terms)
                assert rc == GMB_EINVAL and clean, f"{label} terms = {terms}: status {rc}, outputs clean {clean}"
                assert "the process has no derivative" in msg, msg
            with pytest.raises(ValueError, match="no derivative"):
                eng.predict_slope(XX[:50])
            assert eng.predict_grad(XX[:5]).shape == (5, XX.shape[1])  # the mean's gradient stays available (sqrt(r^2 + 1e-12))
            assert eng.factor_is_current() and same_bits(eng.predict(XX[:50]), before)


def test_bad_arguments_and_missing_factors_are_refused(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    name = "three_term"
    spec, theta, X, y, _, _ = SR.problem(name)
    Xs = SR.points(name, 129)[:40]
    with engine_in(name, None) as eng:
        def refusal_of(call):
            with pytest.raises(ValueError) as info:
                call()
            return str(info.value)

        def refused(label):
            for rc, clean, _ in (poisoned_call(eng, Xs), poisoned_call(eng, Xs, terms=1)):
                assert rc == GMB_EINVAL and clean, f"{label}: status {rc}, outputs clean {clean}"
            # word for word gmb_predict_grad's refusal
            assert refusal_of(lambda: eng.predict_slope(Xs)).replace("slope", "grad") == refusal_of(lambda: eng.predict_grad(Xs)), label

        refused("before gmb_factorize")
        eng.factorize()
        assert poisoned_call(eng, Xs)[:2] == (0, False)
        eng.set_theta(theta * 1.01)
        refused("after gmb_set_theta")
        eng.factorize()
        before = eng.predict_slope(Xs, cov=True)
        D = X.shape[1]
        bad = [("M < 0", {"M": -1}), ("ldxs < D", {"ldxs": D - 1}), ("ldg < D", {"ldg": D - 1}), ("ldc < D x D", {"ldc": D * D - 1}),
               ("null Xs", {"null": ("Xs",)}), ("null dmean", {"null": ("dmean",)}), ("terms = 0", {"terms": 0}),
               ("a term bit beyond T", {"terms": 0b1001})]
        for label, kw in bad:
            rc, clean, _ = poisoned_call(eng, Xs, **kw)
            assert rc == GMB_EINVAL and clean, f"{label}: status {rc}, outputs clean {clean}"
        rc, clean, _ = poisoned_call(eng, Xs, M=0)
        assert rc == 0 and clean, "M = 0 is the empty request"
        assert eng.predict_slope(np.zeros((0, D)))[0].shape == (0, D)
        assert eng.factor_is_current() and same_bits(eng.predict_slope(Xs, cov=True), before)
        eng.set_dist_mode(eng.DIST_CAPACITY)
        refused("capacity mode")


# ---- 7. the front end -------------------------------------------------------------------------------------------------------------------
def test_front_end_on_the_device(gpu):
    """``predict_grid_slope(joint=True)`` of the fitted example table against the reference at the same theta, through the
    standardizer: the bars above, in standardized units."""
    from test_gpu_frontend import example_gp

    gp = example_gp().fit(continuous_dims=["X", "Y"], MAP_kwargs={"maxeval": 30})
    gp.prepare_grid(resolution=12)
    slope = gp.predict_grid_slope(joint=True)
    cov = gp.slope_cov["d"]
    assert list(slope) == ["δ[d]/δ[X]", "δ[d]/δ[Y]"] and all(ua.shape == (12, 12) for ua in slope.values()) and cov.shape == (12, 12, 2, 2)
    assert np.array_equal(cov, np.swapaxes(cov, 2, 3))
    grad = gp.predict_grid_grad(norm=False)
    pa, _, _ = gp._prepare_points_for_prediction(gp.grid_points, output=["d"])
    spec, theta = gp.model.spec.as_dict(), gp._theta_fitted
    dmean, dvar, dcov = SR.posterior(spec, theta, gp.model.X, gp.model.y, pa)
    scale = max(1.0, float(np.max(SR.prior_curvature(spec, theta, gp.model.X, pa))))
    sy = np.sqrt(gp.stdzr["d"]["σ2"])
    sx = np.array([np.sqrt(gp.stdzr[x]["σ2"]) for x in ("X", "Y")])
    cols = [gp.dims.index(x) for x in ("X", "Y")]
    for k, x in enumerate(("X", "Y")):
        ua = slope[f"δ[d]/δ[{x}]"]
        assert mean_err(ua.μ.ravel() * sx[k] / sy, dmean[:, cols[k]], f"front end δ[d]/δ[{x}] mean") <= 1e-8
        assert cov_err(ua.σ2.ravel() * (sx[k] / sy) ** 2, dvar[:, cols[k]], scale, f"front end δ[d]/δ[{x}] variance") <= 1e-9
        assert np.array_equal(ua.σ2, cov[:, :, k, k])
        assert mean_err(ua.μ.ravel(), grad[f"δ[d]/δ[{x}]"].values().ravel(), f"front end δ[d]/δ[{x}] mean against predict_grid_grad") <= 1e-8
        assert np.all(ua.σ2 > 0.0)
    got = cov.reshape(144, 2, 2) * np.outer(sx, sx) / sy**2
    assert cov_err(got, dcov[:, cols][:, :, cols], scale, "front end slope_cov") <= 1e-9
