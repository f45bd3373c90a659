"""A batch of experiments by greedy integrated variance reduction on the MI355X: ``gmb_design_batch`` and the front end above it
against the numpy yardstick of tests/design_reference.py -- the definition, spelled out on the latent posterior covariance of the
candidates with the stacked set.  Needs a GPU (``-m gpu``).

Shapes: the Matern-5/2 table (N = 700: six block columns, the last ragged) and the three-term additive model (N = 300: coregion
tables, two outputs, hetero noise, a linear dimension -- the kernels' general path and the term walk), in both factor states
(``factorize``: the solve form; ``evaluate(theta, grad=True)``: the product form over the resident U).  M in {1, 127, 130}
(below, at and across a 128-row tile: a padded candidate block), R in {1, 129, 2 DESIGN_CHUNK + 1} (one reference point, a partial
tile, three column chunks with a ragged last), q in {0, 1, 8}; q = M + 2 without repeats at M = 5 (ends in -1s); a candidate set
with a training point and an exact duplicate pair.

Bars, by first-order propagation of the suite's joint-posterior bar ``eps_C = 1e-9 max(1, max|C|)`` (tests/test_gpu_joint.py)
through the definition:

* a gain at step t: ``(1 + 3 t) eps_C (2 sum_p w_p |D_ap| + gain_a) / s_a`` on the reference's own D at that step -- gain = sum w
  D^2 / s has the differential (2 sum w |D| dD + gain ds) / s, and each downdate adds the errors of three entries with
  coefficients bounded by sqrt(D_aa D_pp) / s <= 1 under noise;
* ``ivar0``: ``eps_C sum_r w_r`` (a weighted sum of variances);
* two results that are one quantity by different launches or orders (a zero weight against the point removed, permuted
  candidates): the gain bar;
* ``ivar0 - sum gains`` against the engine's own ``append`` + ``predict``: ``eps_C sum w`` + the gains' bars;
* ``picks`` equal the yardstick's at EVERY step: tests/test_design_cpu.py asserts that each pick leads its runner-up by more
  than 100 bars;
* NULL weights against explicit ``1 / R``, a repeated call, every call form: bit-identical.

Measured ratios are printed per test (``DESIGN ...``); the worst seen on an MI355X, as fractions of the bar: ``score0`` 1.2e-5,
gains 1.1e-5, ``ivar0`` 1.9e-5, a zero weight against the point removed 6.8e-8, permuted candidates 3.5e-7, the engine's own
``append`` + ``predict`` 1.2e-7.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abi_forms as AF
import design_reference as DR
from test_gpu_abi_forms import FORMS, mat_in, sync, take_vec, vec_in, vec_out
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

STATES = ["solve", "product"]


@contextlib.contextmanager
def engine_in(name, state, jitter=None):
    spec, theta, X, y = DR.problem(name)
    if jitter is not None:
        spec = dict(spec, jitter=jitter)
    with make_engine(spec, theta, X, y) as eng:
        if state == "solve":
            eng.factorize()
        else:
            eng.evaluate(theta, grad=True)
        yield eng


def takes_product_form(eng, X):
    eng.predict(X[:3])
    return eng.timings()["predict_gemm_form"] == 1


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def worst_ratio(got, ref, bars):
    """max |got - ref| / bar over the entries with a bar; an entry without one (an excluded candidate, a pick of -1) is exact."""
    got, ref, bars = np.asarray(got, float), np.asarray(ref, float), np.asarray(bars, float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    live = bars > 0
    assert np.array_equal(got[~live], ref[~live])
    return float(np.max(np.abs(got - ref)[live] / bars[live])) if np.any(live) else 0.0


def check(eng, Xc, Xr, ref, ivar_r, eps, q, what, weights=None, with_noise=True, allow_repeats=True):
    """One call against a reference run of at least q steps; returns the call's results."""
    picks, gains, score0, ivar0 = out = eng.design_batch(Xc, Xr, q, weights=weights, with_noise=with_noise, allow_repeats=allow_repeats)
    sw = 1.0 if weights is None else float(np.sum(weights))
    r_score = worst_ratio(score0, ref["score0"], ref["score0_bars"])
    r_gain = worst_ratio(gains, ref["gains"][:q], ref["bars"][:q]) if q else 0.0
    r_ivar = abs(ivar0 - ivar_r) / (eps * sw)
    print(f"DESIGN {what}: error / bar -- score0 {r_score:.2e}, gains {r_gain:.2e}, ivar0 {r_ivar:.2e}; picks {picks.tolist()}")
    assert picks.tolist() == ref["picks"][:q].tolist(), what
    assert r_score <= 1.0 and r_gain <= 1.0 and r_ivar <= 1.0, what
    return out


# ---- 1. against the definition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_against_the_definition(gpu, name, state):
    Xc_all, Xr_all = DR.points(name)
    with engine_in(name, state) as eng:
        for M in DR.M_SIZES:
            for R in DR.R_SIZES:
                eps = DR.eps_c(DR.rows_of(name, M, R)[0])
                for q in DR.Q_SIZES:
                    ref, ivar_r = DR.reference(name, M, R)
                    check(eng, Xc_all[:M], Xr_all[:R], ref, ivar_r, eps, q, f"{name} {state} M = {M} R = {R} q = {q}")
        M, R = 130, 129  # the other settings of noise and repeats, at the padded candidate block
        eps = DR.eps_c(DR.rows_of(name, M, R)[0])
        for with_noise, allow_repeats in ((True, False), (False, False)):
            ref, ivar_r = DR.reference(name, M, R, with_noise, allow_repeats)
            check(eng, Xc_all[:M], Xr_all[:R], ref, ivar_r, eps, DR.Q_MAX, f"{name} {state} M = {M} R = {R} noise {with_noise} repeats {allow_repeats}",
                  with_noise=with_noise, allow_repeats=allow_repeats)
        assert takes_product_form(eng, DR.problem(name)[2]) == (state == "product")


@pytest.mark.parametrize("state", STATES)
def test_a_batch_larger_than_the_candidates_ends_in_minus_ones(gpu, state):
    name, M, R = "matern", 5, 129
    Xc, Xr = DR.points(name)
    ref, ivar_r = DR.reference(name, M, R, True, False, M + 2)
    with engine_in(name, state) as eng:
        picks, gains, _, _ = check(eng, Xc[:M], Xr[:R], ref, ivar_r, DR.eps_c(DR.rows_of(name, M, R)[0]), M + 2, f"{name} {state} q = M + 2 without repeats",
                                   allow_repeats=False)
        assert picks[M:].tolist() == [-1, -1] and gains[M:].tolist() == [0.0, 0.0] and sorted(picks[:M]) == list(range(M))


@pytest.mark.parametrize("with_noise", [True, False])
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_a_training_point_and_an_exact_duplicate_pair(gpu, name, state, with_noise):
    Xc, Xr, ref, ivar_r, (lo, hi) = DR.duplicates_case(name, with_noise)
    D0 = DR.posterior_rows(*DR.problem(name), Xc, Xr)[0]
    with engine_in(name, state) as eng:
        picks, _, score0, _ = check(eng, Xc, Xr, ref, ivar_r, DR.eps_c(D0), DR.Q_MAX, f"{name} {state} duplicates noise {with_noise}",
                                    with_noise=with_noise, allow_repeats=False)
        assert score0[lo] == score0[hi] == score0.max(), "the two copies of the best candidate do not tie"
        picks = picks.tolist()
        assert picks[0] == lo, "the tie did not go to the lower index"
        print(f"DESIGN {name} {state} duplicates noise {with_noise}: copies {lo}, {hi} picked at steps "
              f"{picks.index(lo) if lo in picks else None}, {picks.index(hi) if hi in picks else None}")


# ---- 2. weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_weights(gpu, name, state):
    M, R, q, k = 127, 129, DR.Q_MAX, 40
    Xc, Xr = DR.points(name)
    Xc, Xr = Xc[:M], Xr[:R]
    D0, var_r = DR.rows_of(name, M, R)
    noise = DR.noise_of(name, Xc)
    with engine_in(name, state) as eng:
        null = eng.design_batch(Xc, Xr, q)
        assert same_bits(eng.design_batch(Xc, Xr, q, weights=np.full(R, 1.0 / R)), null), "NULL weights differ from explicit 1 / R"
        # one weight zero against that point removed: the chunking changes, the quantity does not
        rng = np.random.default_rng(2)
        w = rng.uniform(0.5, 1.5, R) / R
        w[k] = 0.0
        keep = np.arange(R) != k
        ref = DR.greedy(D0, noise, w, q)
        assert np.all(ref["gaps"] > 100.0 * ref["bars"]), "the weighted case's picks are not decided far above the bar"
        zeroed = check(eng, Xc, Xr, ref, float(w @ var_r), DR.eps_c(D0), q, f"{name} {state} one weight zero", weights=w)
        removed = eng.design_batch(Xc, Xr[keep], q, weights=w[keep])
        assert removed[0].tolist() == zeroed[0].tolist()
        ratio = worst_ratio(removed[1], zeroed[1], ref["bars"]), worst_ratio(removed[2], zeroed[2], ref["score0_bars"])
        print(f"DESIGN {name} {state} zero weight against the point removed: error / bar -- gains {ratio[0]:.2e}, score0 {ratio[1]:.2e}")
        assert max(ratio) <= 1.0 and abs(removed[3] - zeroed[3]) <= DR.eps_c(D0) * float(w.sum())


# ---- 3. repeats, permutations, the engine's own conditioning ---------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_repeatable_and_invariant_under_a_permutation_of_the_candidates(gpu, name, state):
    M, R, q = 130, 2 * DR.DESIGN_CHUNK + 1, DR.Q_MAX
    Xc, Xr = DR.points(name)
    Xc, Xr = Xc[:M], Xr[:R]
    ref, _ = DR.reference(name, M, R)
    with engine_in(name, state) as eng:
        first = eng.design_batch(Xc, Xr, q)
        assert same_bits(eng.design_batch(Xc, Xr, q), first), "a second call differs"
        perm = np.random.default_rng(9).permutation(M)
        picks_p, gains_p, score_p, ivar_p = eng.design_batch(Xc[perm], Xr, q)
        assert perm[picks_p].tolist() == first[0].tolist()
        back = np.empty(M)
        back[perm] = score_p
        ratio = worst_ratio(gains_p, first[1], ref["bars"]), worst_ratio(back, first[2], ref["score0_bars"])
        print(f"DESIGN {name} {state} permuted candidates: error / bar -- gains {ratio[0]:.2e}, score0 {ratio[1]:.2e}")
        assert max(ratio) <= 1.0 and ivar_p == first[3]


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_gains_are_what_the_engines_own_append_removes(gpu, name, state):
    """``ivar0 - sum gains`` against ``append`` of the picks (y = 0) to a second engine + ``predict`` of the reference points.  The
    model's jitter is set to 0 for BOTH engines: the definition's s_a is ``var f + noise`` -- what a prediction with noise
    reports -- while an appended observation gets the training diagonal's jitter on top, 1e-6 / s_a relatively."""
    M, R, q = 127, 129, DR.Q_MAX
    Xc, Xr = DR.points(name)
    Xc, Xr = Xc[:M], Xr[:R]
    spec, theta, X, y = DR.problem(name)
    spec0 = dict(spec, jitter=0.0)
    D0, var_r = DR.posterior_rows(spec0, theta, X, y, Xc, Xr)
    w = np.full(R, 1.0 / R)
    ref = DR.greedy(D0, DR.noise_of(name, Xc), w, q)
    eps = DR.eps_c(D0)
    assert np.all(ref["gaps"] > 100.0 * ref["bars"])
    with engine_in(name, state, jitter=0.0) as eng:
        picks, gains, _, ivar0 = check(eng, Xc, Xr, ref, float(w @ var_r), eps, q, f"{name} {state} jitter 0")
    with make_engine(spec0, theta, X, y) as grown:
        grown.factorize()
        grown.append(Xc[picks], np.zeros(q))
        _, var = grown.predict(Xr, with_noise=False)
    left, other = ivar0 - float(np.sum(gains)), float(w @ var)
    bar = eps * float(w.sum()) + float(np.sum(ref["bars"]))
    print(f"DESIGN {name} {state}: ivar0 {ivar0:.9e} - gains = {left:.9e}, append + predict {other:.9e}, |gap| / bar {abs(left - other) / bar:.2e}")
    assert abs(left - other) <= bar


# ---- 4. call forms ------------------------------------------------------------------------------------------------------------------------
def raw_call(eng, Xc, Xr, weights, q, form, score=True, ivar=True):
    M, R = len(Xc), len(Xr)
    xc, xr = mat_in(Xc, form, 3), mat_in(Xr, form, 5)
    w = vec_in(weights, form) if weights is not None else None
    picks = vec_out(q, form)  # (8-byte slots either way: the fill pattern is read back as int64)
    gains, s0, iv = vec_out(q, form), vec_out(M, form) if score else None, vec_out(1, form) if ivar else None
    sync()
    rc = eng._lib.gmb_design_batch(eng._h, xc.ptr, M, xc.ld, xr.ptr, R, xr.ld, w.ptr if w else None, q, 1, 1, picks.ptr, gains.ptr,
                                   s0.ptr if s0 else None, iv.ptr if iv else None, form.memspace)
    assert rc == 0, (form.name, rc, eng.last_error() if hasattr(eng, "last_error") else "")
    what = f"gmb_design_batch ({form.name})"
    out = (take_vec(picks, q, what + " picks").view(np.int64), take_vec(gains, q, what + " gains"))
    if score:
        out += (take_vec(s0, M, what + " score0"),)
    if ivar:
        out += (take_vec(iv, 1, what + " ivar0"),)
    return out


@pytest.mark.parametrize("state", STATES)
def test_call_forms(gpu, state):
    """Points with leading dimensions > D (NaN padding) and every array in device memory: the same bits as the packed host call,
    everything behind the outputs' last elements untouched; ``score0`` and ``ivar0`` may be NULL."""
    name, M, R, q = "three_term", 130, 129, 5
    Xc, Xr = DR.points(name)
    Xc, Xr = Xc[:M], Xr[:R]
    w = np.random.default_rng(4).uniform(0.0, 2.0, R) / R
    with engine_in(name, state) as eng:
        picks, gains, score0, ivar0 = eng.design_batch(Xc, Xr, q, weights=w)
        want = (picks, gains, score0, np.array([ivar0]))
        want_null = eng.design_batch(Xc, Xr, q)
        for form in FORMS:
            assert same_bits(raw_call(eng, Xc, Xr, w, q, form), want), f"{form.name}: differs from the packed host call"
            assert same_bits(raw_call(eng, Xc, Xr, None, q, form)[:3], want_null[:3]), f"{form.name}: NULL weights differ"
            assert same_bits(raw_call(eng, Xc, Xr, w, q, form, score=False, ivar=False), want[:2]), f"{form.name}: without score0 / ivar0"


# ---- 5. refusals and the state the call leaves ---------------------------------------------------------------------------------------------
def poisoned_call(eng, Xc, Xr, M=None, R=None, q=3, weights=None, ldc=None, ldr=None, null=()):
    """``(status, outputs still poisoned)`` of a raw host call."""
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    Xc, Xr = np.ascontiguousarray(Xc, dtype=np.float64), np.ascontiguousarray(Xr, dtype=np.float64)
    k = max(abs(q), len(Xc), 2)
    picks, gains, score0, ivar0 = (AF.padded(k, AF.SPARE, AF.FILL) for _ in range(4))
    wts = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    rc = eng._lib.gmb_design_batch(eng._h, None if "Xc" in null else ptr(Xc), len(Xc) if M is None else M, Xc.shape[1] if ldc is None else ldc,
                                   None if "Xr" in null else ptr(Xr), len(Xr) if R is None else R, Xr.shape[1] if ldr is None else ldr,
                                   None if wts is None else ptr(wts), q, 1, 1, None if "picks" in null else ptr(picks),
                                   None if "gains" in null else ptr(gains), ptr(score0), ptr(ivar0), 0)
    clean = all(AF.untouched(a, 0, AF.FILL_BITS) for a in (picks, gains, score0, ivar0))
    return rc, clean


def test_bad_arguments_are_refused_and_launch_nothing(gpu):
    from gumbi_amd.engine import GMB_EINVAL, GMB_ENOMEM

    name, M, R = "three_term", 20, 33
    Xc, Xr = DR.points(name)
    Xc, Xr = Xc[:M], Xr[:R]
    D = Xc.shape[1]
    with engine_in(name, "solve") as eng:
        before = (eng.copy_v(),) + eng.predict(Xr)
        resident = eng.resident_bytes()
        nan_c, nan_r = Xc.copy(), Xr.copy()
        nan_c[7, 1], nan_r[R - 1, 0] = np.nan, np.nan
        neg_w, nan_w, inf_w = np.full(R, 0.1), np.full(R, 0.1), np.full(R, 0.1)
        neg_w[3], nan_w[R // 2], inf_w[-1] = -1e-300, np.nan, np.inf
        bad = [("M = 0", {"M": 0}), ("M < 0", {"M": -1}), ("R = 0", {"R": 0}), ("R < 0", {"R": -4}), ("q < 0", {"q": -1}),
               ("ldc < D", {"ldc": D - 1}), ("ldr < D", {"ldr": D - 1}), ("null Xc", {"null": ("Xc",)}), ("null Xr", {"null": ("Xr",)}),
               ("null picks", {"null": ("picks",)}), ("null gains", {"null": ("gains",)}),
               ("a negative weight", {"weights": neg_w}), ("a NaN weight", {"weights": nan_w}), ("an infinite weight", {"weights": inf_w}),
               ("a NaN candidate", {"Xc": nan_c}), ("a NaN reference point", {"Xr": nan_r})]
        for label, kw in bad:
            kw = dict(kw)
            rc, clean = poisoned_call(eng, kw.pop("Xc", Xc), kw.pop("Xr", Xr), **kw)
            assert rc == GMB_EINVAL, f"{label}: status {rc}"
            assert clean, f"{label}: outputs were written"
            assert eng.resident_bytes() == resident, f"{label}: device memory was allocated"
        # a request the device cannot hold is measured before any of the caller's arrays is read: R = 2^29 behind these 33 rows
        rc, clean = poisoned_call(eng, Xc, Xr, R=1 << 29)
        assert rc == GMB_ENOMEM and clean and eng.resident_bytes() == resident
        with pytest.raises(MemoryError, match="bytes"):
            eng._check(rc, "gmb_design_batch")
        rc, clean = poisoned_call(eng, Xc, Xr, M=32769)  # more candidates than one M-tile of a prediction
        assert rc == GMB_ENOMEM and clean and eng.resident_bytes() == resident
        with pytest.raises(ValueError, match="negative"):
            eng.design_batch(Xc, Xr, 2, weights=neg_w)
        with pytest.raises(ValueError, match="NaN"):
            eng.design_batch(nan_c, Xr, 2)
        with pytest.raises(ValueError, match="weights for"):
            eng.design_batch(Xc, Xr, 2, weights=neg_w[:-1])
        assert eng.factor_is_current() and eng.resident_bytes() == resident
        assert same_bits((eng.copy_v(),) + eng.predict(Xr), before), "a prediction changed behind the refused calls"
        assert poisoned_call(eng, Xc, Xr)[0] == 0


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", DR.PROBLEMS)
def test_the_call_leaves_predictions_and_the_factor_as_found(gpu, name, state):
    Xc, Xr = DR.points(name)
    Xs = Xr[:300]
    with engine_in(name, state) as eng:
        before = (eng.copy_v(),) + eng.predict(Xs) + eng.predict(Xs, with_noise=False)
        form = eng.timings()["predict_gemm_form"]
        eng.design_batch(Xc, Xr, 3)                 # a prediction workspace larger than the prediction's own
        eng.design_batch(Xc[:5], Xr[:7], 3)         # ... and a smaller one
        assert eng.factor_is_current()
        after = (eng.copy_v(),) + eng.predict(Xs) + eng.predict(Xs, with_noise=False)
        assert same_bits(after, before) and eng.timings()["predict_gemm_form"] == form


def test_engines_without_a_usable_single_factor_refuse(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    name = "three_term"
    spec, theta, X, y = DR.problem(name)
    Xc, Xr = DR.points(name)
    Xc, Xr = Xc[:9], Xr[:20]
    with make_engine(spec, theta, X, y) as eng:
        def refused(label):
            rc, clean = poisoned_call(eng, Xc, Xr)
            assert rc == GMB_EINVAL and clean, f"{label}: status {rc}, outputs clean {clean}"

        refused("before gmb_factorize")
        eng.factorize()
        assert poisoned_call(eng, Xc, Xr)[0] == 0
        eng.set_theta(theta * 1.01)
        refused("after gmb_set_theta")
        eng.factorize()
        eng.set_dist_mode(eng.DIST_CAPACITY)
        refused("capacity mode")
        with pytest.raises(ValueError):
            eng.design_batch(Xc, Xr, 2)


# ---- 6. the front end ---------------------------------------------------------------------------------------------------------------------
def test_front_end_on_the_device(gpu):
    """``design_batch`` of the fitted example: the step-0 scores against the definition at the same theta, the picks' bookkeeping."""
    from test_gpu_frontend import example_gp

    gp = example_gp().fit(continuous_dims=["X", "Y"], MAP_kwargs={"maxeval": 30})
    picked = gp.design_batch(6, n_candidates=130, n_reference=300, seed=5)
    assert picked.shape == (6,) and set(picked.names) == {"X", "Y"} and gp.design_scores.shape == (130,)
    assert gp.design_picks[0] == int(np.argmax(gp.design_scores)) and gp.design_gains[0] == gp.design_scores.max()
    assert np.all(np.diff(gp.design_gains) <= 0) and 0 < gp.design_gains.sum() < gp.design_ivar0
    cols = [gp.dims.index(d) for d in gp.continuous_dims]
    Zc = np.column_stack([gp.design_candidates.z[d + "_z"].values() for d in gp.continuous_dims])
    full = gp._acquisition_problem(None, "UCB", True, None, None)[3]
    assert np.array_equal(full(Zc)[:, cols], Zc)
    spec, theta = gp.model.spec.as_dict(), gp._theta_fitted
    Xr = full(Zc[:40])
    D0, var_r = DR.posterior_rows(spec, theta, gp.model.X, gp.model.y, full(Zc), Xr)
    w = np.full(len(Xr), 1.0 / len(Xr))
    ref = DR.greedy(D0, DR.O.noise_diag(spec, np.asarray(theta, float), full(Zc)), w, 0)
    scores = gp.variance_reduction(Zc, Zc[:40])
    ratio = worst_ratio(scores, ref["score0"], ref["score0_bars"])
    print(f"DESIGN front end: score0 error / bar {ratio:.2e}, ivar0 {gp.design_ivar0:.6e} against {float(w @ var_r):.6e}")
    assert ratio <= 1.0 and abs(gp.design_ivar0 - float(w @ var_r)) <= DR.eps_c(D0)
