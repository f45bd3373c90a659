"""Leave-one-out and leave-group-out predictions from the resident factor on the MI355X: ``gmb_loo`` / ``gmb_leave_out`` and the
front end above them against the numpy yardstick of tests/leave_out_reference.py, which literally deletes the rows and predicts
them.  Needs a GPU (``-m gpu``).

Shapes: the three-term additive model (N = 300: three block columns, the last ragged; coregion tables, two outputs, hetero noise)
and a Matern-5/2 table with N = 700 = 5 * 128 + 60 (six block columns -- more than one chunk of the product form's reduction, which
takes two block columns per workgroup, and the size from which the joint matrix is factored by the tile kernel) at cond 3e3, and
at cond 4.5e5 for the conditioning case.  States: behind ``factorize`` (the solve form, by size and with the tile solve forced),
behind ``evaluate(theta, grad=True)`` (the product form over the resident U) and behind the same with ``set_predict_form(0)``.

Bars -- the project's standing GPU-against-oracle bars (tests/test_gpu_components.py):

* means: 1e-8 max|ref|;
* variances and covariances: 1e-9 max(1, max|ref|) (leave-out variances of the three-term problem reach 27 - 67);
* two GPU results that are the same quantity by different launches: 1e-10 relative (means), 1e-9 absolute (variances) for the two
  forms of ``gmb_loo``; 1e-10 relative for a one-row group against ``gmb_loo``, a covariance's diagonal against the variances and
  a scrambled group against the sorted one;
* a call repeated, and ``gmb_leave_out`` with and without ``cov``: bit-identical.

The yardstick's own closed form agrees with deletion to <= 9e-12 on these problems (tests/test_leave_out_cpu.py), three orders
inside the bars.  Measured errors are printed per test (``LEAVE-OUT ...``).
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import abi_forms as AF
import leave_out_reference as LR
from test_gpu_abi_forms import FORMS, mat_out, sync, take, take_vec, vec_out
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

STATES = ["solve", "solve_tiles", "product", "product_form0"]
RANGES = {"three_term": [(0, 300), (120, 260), (299, 300), (140, 140)], "matern": [(0, 700), (300, 560), (699, 700), (350, 350)]}


@contextlib.contextmanager
def engine_in(name, state):
    p = LR.problem(name)
    with make_engine(p.spec, p.theta, p.X, p.y) as eng:
        if state == "solve_tiles":
            eng.set_chol_scheme(eng.CHOL_TILES)
        if state.startswith("solve"):
            eng.factorize()
        else:
            eng.evaluate(p.theta, grad=True)
            if state == "product_form0":
                eng.set_predict_form(0)
        yield eng


def u_is_resident(eng, p):
    """The sibling state of the product form: behind the same evaluation a prediction takes the GEMM form."""
    eng.predict(p.X[:3])
    return eng.timings()["predict_gemm_form"] == 1


def groups_of(name):
    return LR.three_term_groups() if name == "three_term" else LR.matern_groups()


def mean_err(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
    print(f"LEAVE-OUT {what}: max |got - ref| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    return err / scale


def var_err(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), max(1.0, float(np.max(np.abs(ref))))
    print(f"LEAVE-OUT {what}: max |got - ref| = {err:.3e}, scale {scale:.3g}, ratio {err / scale:.2e}")
    return err / scale


def same_bits(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return len(a) == len(b) and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ---- 1. gmb_loo against deletion ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", ["three_term", "matern"])
def test_loo_against_deletion(gpu, name, state):
    p = LR.problem(name)
    with engine_in(name, state) as eng:
        for with_noise in (True, False):
            mean_r, var_r = LR.loo_reference(name, with_noise)
            full = None
            for start, stop in RANGES[name]:
                mean, var = eng.loo((start, stop), with_noise=with_noise)
                assert mean.shape == var.shape == (stop - start,)
                if stop == start:
                    continue
                what = f"{name} {state} loo [{start}, {stop}) noise={with_noise}"
                assert mean_err(mean, mean_r[start:stop], what + " mean") <= 1e-8
                assert var_err(var, var_r[start:stop], what + " var") <= 1e-9
                if full is None:
                    full = (mean, var)
                    assert same_bits(eng.loo(with_noise=with_noise), full), f"{what}: rows=None differs from the whole range"
                else:  # a sub-range is the whole range's rows (other tiles of the same sums)
                    assert mean_err(mean, full[0][start:stop], what + " mean against the whole range") <= 1e-10
                    assert float(np.max(np.abs(var - full[1][start:stop]))) <= 1e-9
        assert u_is_resident(eng, p) == (state == "product")


@pytest.mark.parametrize("name", ["three_term", "matern", "matern_illcond"])
def test_loo_product_form_against_solve_form_on_the_same_factor(gpu, name):
    p = LR.problem(name)
    with engine_in(name, "product") as eng:
        assert u_is_resident(eng, p)
        for with_noise in (True, False):
            product = eng.loo(with_noise=with_noise)
            assert eng.set_predict_form(0) != 0
            solve = eng.loo(with_noise=with_noise)
            eng.set_predict_form(-1)
            assert not same_bits(product, solve), "the two forms gave the same bits: the switch did nothing"
            assert mean_err(product[0], solve[0], f"{name} product against solve, mean noise={with_noise}") <= 1e-10
            err = float(np.max(np.abs(product[1] - solve[1])))
            print(f"LEAVE-OUT {name} product against solve, var noise={with_noise}: max |diff| = {err:.3e}")
            assert err <= 1e-9
            assert same_bits(eng.loo(with_noise=with_noise), product)


# ---- 2. gmb_leave_out against deletion ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["solve", "product"])
@pytest.mark.parametrize("name", ["three_term", "matern"])
def test_leave_out_against_deletion(gpu, name, state):
    p = LR.problem(name)
    with engine_in(name, state) as eng:
        for label, rows in groups_of(name).items():
            for with_noise in (True, False):
                mean_r, cov_r = p.by_deletion(rows, with_noise)
                mean, var, cov = eng.leave_out(rows, with_noise=with_noise, cov=True)
                what = f"{name} {state} {label} (m = {len(rows)}) noise={with_noise}"
                assert mean_err(mean, mean_r, what + " mean") <= 1e-8
                assert var_err(var, np.diag(cov_r), what + " var") <= 1e-9
                assert var_err(cov, cov_r, what + " cov") <= 1e-9
                assert np.array_equal(cov, cov.T), what + ": cov is not exactly symmetric"
                assert mean_err(np.diag(cov), var, what + " diag(cov) against var") <= 1e-10
                assert same_bits(eng.leave_out(rows, with_noise=with_noise), (mean, var)), what + ": mean / var depend on cov"
                assert same_bits(eng.leave_out(rows, with_noise=with_noise, cov=True), (mean, var, cov))


@pytest.mark.parametrize("name", ["three_term", "matern"])
def test_leave_out_in_a_scrambled_order_and_of_one_row(gpu, name):
    p = LR.problem(name)
    rows = groups_of(name)["random37" if name == "three_term" else "every5th"]
    perm = np.random.default_rng(7).permutation(len(rows))
    with engine_in(name, "solve") as eng:
        mean, var, cov = eng.leave_out(rows, cov=True)
        mean_s, var_s, cov_s = eng.leave_out(rows[perm], cov=True)
        assert mean_err(mean_s, mean[perm], f"{name} scrambled mean") <= 1e-10
        assert mean_err(var_s, var[perm], f"{name} scrambled var") <= 1e-10
        assert mean_err(cov_s, cov[np.ix_(perm, perm)], f"{name} scrambled cov") <= 1e-10
        last = p.N - 1
        for with_noise in (True, False):
            m1, v1, c1 = eng.leave_out([last], with_noise=with_noise, cov=True)
            ml, vl = eng.loo((last, last + 1), with_noise=with_noise)
            assert abs(m1[0] - ml[0]) <= 1e-10 * abs(ml[0]) and abs(v1[0] - vl[0]) <= 1e-10 * abs(vl[0]) and c1.shape == (1, 1)
            assert abs(c1[0, 0] - v1[0]) <= 1e-10 * abs(v1[0])


# ---- 3. conditioning ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["solve", "product"])
def test_ill_conditioned_table(gpu, state):
    """sigma = 0.02: cond(Sigma) 4.5e5.  The same bars."""
    name = "matern_illcond"
    p = LR.problem(name)
    rows = LR.matern_groups()["every5th"]
    with engine_in(name, state) as eng:
        mean_r, var_r = LR.loo_reference(name, True)
        mean, var = eng.loo()
        assert mean_err(mean, mean_r, f"{name} {state} loo mean") <= 1e-8
        assert var_err(var, var_r, f"{name} {state} loo var") <= 1e-9
        gm_r, gc_r = p.by_deletion(rows, True)
        gm, gv, gc = eng.leave_out(rows, cov=True)
        assert mean_err(gm, gm_r, f"{name} {state} every5th mean") <= 1e-8
        assert var_err(gv, np.diag(gc_r), f"{name} {state} every5th var") <= 1e-9
        assert var_err(gc, gc_r, f"{name} {state} every5th cov") <= 1e-9


# ---- 4. call forms ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["solve", "product"])
def test_call_forms(gpu, state):
    """Outputs in host and in device memory, ``ldc > m`` with the padding left alone, nothing written behind n / m elements."""
    name = "matern"
    rows = LR.matern_groups()["rows300_560"]
    m = len(rows)
    idx = np.ascontiguousarray(rows, dtype=np.int64)
    with engine_in(name, state) as eng:
        want_loo = eng.loo((300, 560))
        want = eng.leave_out(rows, cov=True)
        for form in FORMS:
            mean, var = vec_out(260, form), vec_out(260, form)
            sync()
            assert eng._lib.gmb_loo(eng._h, 300, 260, 1, mean.ptr, var.ptr, form.memspace) == 0
            got = (take_vec(mean, 260, f"{form.name} loo mean"), take_vec(var, 260, f"{form.name} loo var"))
            assert same_bits(got, want_loo), f"{form.name}: gmb_loo differs from the packed host call"
            mean, var, cov = vec_out(m, form), vec_out(m, form), mat_out(m, m, form, 5)
            sync()
            rc = eng._lib.gmb_leave_out(eng._h, idx.ctypes.data_as(C.c_void_p), m, 1, mean.ptr, var.ptr, cov.ptr, cov.ld, form.memspace)
            assert rc == 0
            got = (take_vec(mean, m, f"{form.name} mean"), take_vec(var, m, f"{form.name} var"), take(cov, m, m, f"{form.name} cov"))
            assert same_bits(got, want), f"{form.name}: gmb_leave_out differs from the packed host call"
            # var may be NULL when cov is not, cov may be NULL
            mean, cov = vec_out(m, form), mat_out(m, m, form, 5)
            sync()
            assert eng._lib.gmb_leave_out(eng._h, idx.ctypes.data_as(C.c_void_p), m, 1, mean.ptr, None, cov.ptr, cov.ld, form.memspace) == 0
            assert same_bits((take_vec(mean, m, "mean"), take(cov, m, m, "cov")), (want[0], want[2]))
            mean, var = vec_out(m, form), vec_out(m, form)
            sync()
            assert eng._lib.gmb_leave_out(eng._h, idx.ctypes.data_as(C.c_void_p), m, 1, mean.ptr, var.ptr, None, 0, form.memspace) == 0
            assert same_bits((take_vec(mean, m, "mean"), take_vec(var, m, "var")), want[:2])


# ---- 5. state contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ["solve", "product"])
def test_new_calls_leave_the_engine_as_found(gpu, state):
    name = "matern"
    p = LR.problem(name)
    Xs = p.X[::9] + 0.05
    groups = LR.matern_groups()
    with engine_in(name, state) as eng:
        def snapshot():
            snap = (eng.copy_factor(0, 128, 0, 128), eng.copy_factor(640, 60, 256, 444), eng.copy_factor(300, 200, 100, 100), eng.copy_v())
            snap += eng.predict(Xs)
            form = eng.timings()["predict_gemm_form"]
            snap += eng.predict_joint(Xs, with_noise=True, jitter=0.0)
            if state == "product":
                snap += (eng.copy_alpha(),)
            return snap, form

        assert eng.factor_is_current()
        before, form = snapshot()
        assert form == (1 if state == "product" else 0)
        calls = [("loo", lambda: eng.loo()), ("loo latent range", lambda: eng.loo((300, 560), with_noise=False)),
                 ("leave_out", lambda: eng.leave_out(groups["every5th"])),
                 ("leave_out cov", lambda: eng.leave_out(groups["rows300_560"], with_noise=False, cov=True))]
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


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def raw_calls(eng, N):
    """``(label, call)``: every call returns ``(status, outputs still poisoned)``."""
    lib, h = eng._lib, eng._h
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def loo(i0, n, null=False):
        mean, var = AF.padded(8, AF.SPARE, AF.FILL), AF.padded(8, AF.SPARE, AF.FILL)
        rc = lib.gmb_loo(h, i0, n, 1, None if null else ptr(mean), ptr(var), 0)
        return rc, AF.untouched(mean, 0, AF.FILL_BITS) and AF.untouched(var, 0, AF.FILL_BITS)

    def leave_out(idx, m=None, ldc=None, null=False):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        m = len(idx) if m is None else m
        k = max(len(idx), 1)
        mean, var = AF.padded(k, AF.SPARE, AF.FILL), AF.padded(k, AF.SPARE, AF.FILL)
        cov = AF.embed(np.full((k, k), AF.FILL), k, AF.FILL)
        rc = lib.gmb_leave_out(h, ptr(idx), m, 1, None if null else ptr(mean), ptr(var), ptr(cov), k if ldc is None else ldc, 0)
        return rc, AF.untouched(mean, 0, AF.FILL_BITS) and AF.untouched(var, 0, AF.FILL_BITS) and AF.untouched(cov, 0, AF.FILL_BITS, rows=0)

    return {"loo": loo, "leave_out": leave_out}


def test_bad_arguments_are_refused_and_write_nothing(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    p = LR.problem("three_term")
    N = p.N
    with engine_in("three_term", "solve") as eng:
        calls = raw_calls(eng, N)
        before = (eng.copy_v(),) + eng.loo() + eng.leave_out([5, 9, 2], cov=True)
        bad = [("range past N", lambda: calls["loo"](N - 3, 4)), ("start past N", lambda: calls["loo"](N + 1, 0)),
               ("negative start", lambda: calls["loo"](-1, 2)), ("negative count", lambda: calls["loo"](3, -2)),
               ("null mean", lambda: calls["loo"](0, 4, null=True)),
               ("duplicates", lambda: calls["leave_out"]([4, 7, 4])), ("index = N", lambda: calls["leave_out"]([1, N, 2])),
               ("negative index", lambda: calls["leave_out"]([1, -1])), ("m = 0", lambda: calls["leave_out"]([3, 4], m=0)),
               ("m > N", lambda: calls["leave_out"](np.arange(N + 1), m=N + 1)), ("ldc < m", lambda: calls["leave_out"]([3, 4, 5], ldc=2)),
               ("null mean (group)", lambda: calls["leave_out"]([3, 4], null=True))]
        for label, call in bad:
            rc, clean = call()
            assert rc == GMB_EINVAL, f"{label}: status {rc}"
            assert clean, f"{label}: outputs were written"
        assert calls["loo"](N, 0) == (0, True) and calls["loo"](17, 0) == (0, True)
        with pytest.raises(ValueError, match="appears twice"):
            eng.leave_out([4, 7, 4])
        with pytest.raises(ValueError, match="not a training row"):
            eng.leave_out([N])
        with pytest.raises(ValueError):
            eng.loo((N - 3, N + 1))
        assert eng.factor_is_current()
        assert same_bits((eng.copy_v(),) + eng.loo() + eng.leave_out([5, 9, 2], cov=True), before)


def test_engines_without_a_usable_single_factor_refuse(gpu):
    from gumbi_amd.engine import GMB_EINVAL

    p = LR.problem("three_term")
    with make_engine(p.spec, p.theta, p.X, p.y) as eng:
        calls = raw_calls(eng, p.N)

        def refused(label):
            for rc, clean in (calls["loo"](0, 8), calls["leave_out"]([1, 2, 3])):
                assert rc == GMB_EINVAL and clean, f"{label}: status {rc}, outputs clean {clean}"

        refused("before gmb_factorize")
        eng.factorize()
        assert calls["loo"](0, 8)[0] == 0
        eng.set_theta(p.theta * 1.01)
        refused("after gmb_set_theta")
        eng.factorize()
        assert calls["leave_out"]([1, 2, 3])[0] == 0
        eng.set_dist_mode(eng.DIST_CAPACITY)
        refused("capacity mode")
        with pytest.raises(ValueError):
            eng.loo()
        eng.set_dist_mode(eng.DIST_REPLICATED)
        eng.factorize()
        assert calls["loo"](0, 8)[0] == 0


# ---- 7. the front end -------------------------------------------------------------------------------------------------------------------
def test_front_end_on_the_device(gpu):
    """``leave_one_out`` / ``leave_group_out(unit=...)`` of the fitted example against an engine that is GIVEN the data without
    the rows, at the same theta."""
    from gumbi_amd.engine import Engine
    from test_gpu_frontend import example_gp

    gp = example_gp().fit(continuous_dims=["X", "Y"], MAP_kwargs={"maxeval": 30})
    X, y = np.asarray(gp.model.X, float), np.asarray(gp.model.y, float)
    n = len(y)

    def without(rows, joint):
        keep = np.setdiff1d(np.arange(n), rows)
        with Engine(0) as eng:
            eng.set_data(X[keep], y[keep])
            eng.set_kernel(gp.model.spec)
            eng.set_theta(gp._theta_fitted)
            eng.factorize()
            return eng.predict_joint(X[rows], with_noise=True, jitter=0.0) if joint else eng.predict(X[rows], with_noise=True)

    res = gp.leave_one_out()
    assert res["mean"].shape == (n,) and list(res["predictions"]) == ["d"]
    picked = [0, n // 2, n - 1]
    ref = [without([i], False) for i in picked]
    mu_r, var_r = np.array([r[0][0] for r in ref]), np.array([r[1][0] for r in ref])
    assert mean_err(res["mean"][picked], mu_r, "front end loo mean") <= 1e-8
    assert var_err(res["var"][picked], var_r, "front end loo var") <= 1e-9
    assert np.allclose(res["z_score"], (y - res["mean"]) / np.sqrt(res["var"]), rtol=1e-14, atol=0)

    groups = gp.leave_group_out(unit="Name", joint=True)
    names = gp.data.wide["Name"].to_numpy()
    assert [g["unit"] for g in groups] == list(dict.fromkeys(names))
    assert sorted(np.concatenate([g["rows"] for g in groups]).tolist()) == list(range(n))
    one = groups[2]
    assert np.array_equal(one["rows"], np.flatnonzero(names == one["unit"]))
    mean_r, cov_r = without(one["rows"], True)
    assert mean_err(one["mean"], mean_r, "front end unit mean") <= 1e-8
    assert var_err(one["cov"], cov_r, "front end unit cov") <= 1e-9
    assert var_err(one["var"], np.diag(cov_r), "front end unit var") <= 1e-9
    assert np.isfinite(one["nlpd"])
