"""``gmb_append`` / ``gmb_truncate`` (C ABI 16) on the MI355X: observations appended to and cut from the RESIDENT factor, against the
numpy oracle at the new size and against a fresh engine at the new size.  Needs a GPU (``-m gpu``).

Bars, the project's own (header of tests/test_gpu_parity.py):

* against the oracle (``dist_mode="direct"``): factor, v and NLML <= 1e-10 relative, mean <= 1e-8 relative, variance <= 1e-9
  absolute, NLML gradient <= 1e-8 of max(1, |g|);
* engine against engine: mean <= 1e-10 relative, variance <= 1e-11 absolute.

The bordered update in numpy agrees with a fresh factorisation to 1.3e-14 (L) and 1.3e-13 (v) on these tables
(tests/test_append_cpu.py), so the bars leave three orders of magnitude to the kernels.  The tables are ``O.synthetic_table`` with
sigma = 0.2; the engine is built at N, factorised, and given the LAST K rows of a table of N + K.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from test_gpu_parity import GOLD, make_engine, rel

pytestmark = pytest.mark.gpu

M_PRED = 64


@functools.lru_cache(maxsize=None)
def table(N, d=2, kind="ExpQuad", seed=2021):
    X, y, ls = O.synthetic_table(N, d, seed=seed, sigma=0.2)
    spec = O.make_spec(d, range(d), kind=kind)
    theta = O.pack_theta(spec, ls, 1.0, 0.2)
    Xs = np.random.default_rng(N).standard_normal((M_PRED, d))
    return spec, theta, X, y, Xs


@functools.lru_cache(maxsize=None)
def oracle_at(N, d=2, kind="ExpQuad", n=None):
    """Oracle results on the first n rows (default all) of the table of N."""
    spec, theta, X, y, Xs = table(N, d, kind)
    n = N if n is None else n
    L, v = O.factorize(spec, theta, X[:n], y[:n], dist_mode="direct")
    nlml = O.nlml(spec, theta, X[:n], y[:n], dist_mode="direct")
    pred = {wn: O.predict(spec, theta, X[:n], y[:n], Xs, with_noise=wn, dist_mode="direct") for wn in (True, False)}
    return L, v, nlml, pred


def check_oracle(eng, ref, Xs, what):
    L_r, v_r, nlml_r, pred_r = ref
    assert eng.factor_is_current(), what
    assert eng.N == len(v_r)
    e_L, e_v = rel(np.tril(eng.copy_factor()), L_r), rel(eng.copy_v(), v_r)
    e_n = abs(eng.nlml() - nlml_r) / abs(nlml_r)
    print(f"APPEND {what}: L {e_L:.2e} v {e_v:.2e} nlml {e_n:.2e}", end="")
    assert e_L <= 1e-10 and e_v <= 1e-10 and e_n <= 1e-10, what
    for wn in (True, False):
        mu, var = eng.predict(Xs, with_noise=wn)
        assert eng.timings()["predict_gemm_form"] == 0  # nothing derived from the old factor survives: the solve form
        e_m, e_s = rel(mu, pred_r[wn][0]), float(np.max(np.abs(var - pred_r[wn][1])))
        print(f" | noise={int(wn)} mean {e_m:.2e} var {e_s:.2e}", end="")
        assert e_m <= 1e-8 and e_s <= 1e-9, what
    print()


def check_engines(eng, other, Xs, what):
    for wn in (True, False):
        mu, var = eng.predict(Xs, with_noise=wn)
        mu_o, var_o = other.predict(Xs, with_noise=wn)
        e_m, e_s = rel(mu, mu_o), float(np.max(np.abs(var - var_o)))
        print(f"APPEND {what}: engine vs engine noise={int(wn)} mean {e_m:.2e} var {e_s:.2e}")
        assert e_m <= 1e-10 and e_s <= 1e-11, what


#: (N, K, d, kind): what each exercises
SHAPES = [(100, 5, 2, "ExpQuad"),      # I0 = 0, layout unchanged
          (120, 20, 2, "ExpQuad"),     # crosses a block boundary, re-layout, I0 = 0
          (300, 1, 2, "ExpQuad"),      # I0 = 2, one corner tile
          (383, 1, 2, "ExpQuad"),      # the y row moves to a block row of its own
          (384, 1, 2, "ExpQuad"),      # empty partial block
          (300, 200, 2, "ExpQuad"),    # corner of several tiles; the corner's recursion resumes over more than one column
          (1000, 16, 3, "Matern52"),   # the starting factor comes from the persistent tile kernel; the split rule gives 3 slices
          (4224, 3, 2, "ExpQuad"),     # 33 block columns
          (200, 3000, 2, "ExpQuad")]   # a LARGE append: 324 corner tiles over k = 128 -- the rule finds one slice, the corner update
                                       # is the trailing update's triangular GEMM, the corner's recursion 24 block columns deep


@pytest.mark.parametrize("N,K,d,kind", SHAPES)
def test_append_matches_oracle_and_a_fresh_engine(gpu, N, K, d, kind):
    spec, theta, X, y, Xs = table(N + K, d, kind)
    with make_engine(spec, theta, X[:N], y[:N]) as eng, make_engine(spec, theta, X, y) as fresh:
        eng.factorize()
        eng.append(X[N:], y[N:])
        check_oracle(eng, oracle_at(N + K, d, kind), Xs, f"({N}, {K})")
        fresh.factorize()
        check_engines(eng, fresh, Xs, f"({N}, {K})")
        # deterministic: the same call sequence on a second engine gives the same bits
        with make_engine(spec, theta, X[:N], y[:N]) as again:
            again.factorize()
            again.append(X[N:], y[N:])
            assert np.array_equal(again.copy_v(), eng.copy_v()) and again.nlml() == eng.nlml()


def test_repeated_appends(gpu):
    """Five appends of one row from N = 126 (through the block boundary at 128) against one append of five."""
    N, K = 126, 5
    spec, theta, X, y, Xs = table(N + K)
    with make_engine(spec, theta, X[:N], y[:N]) as one, make_engine(spec, theta, X[:N], y[:N]) as five:
        one.factorize()
        one.append(X[N:], y[N:])
        five.factorize()
        for j in range(K):
            five.append(X[N + j:N + j + 1], y[N + j:N + j + 1])
            assert five.factor_is_current() and five.N == N + j + 1
        check_oracle(five, oracle_at(N + K), Xs, "5 x 1")
        check_oracle(one, oracle_at(N + K), Xs, "1 x 5")
        check_engines(five, one, Xs, "5 x 1 vs 1 x 5")


def test_append_after_a_gradient_evaluation(gpu):
    """evaluate(theta, grad=True) leaves alpha, U = L^-T and Sigma^-1 behind: all of it is stale after the append."""
    N, K = 600, 10
    spec, theta, X, y, Xs = table(N + K)
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.evaluate(theta, grad=True)
        eng.predict(Xs)  # (the product form, where the evaluation left U behind)
        eng.append(X[N:], y[N:])
        with pytest.raises(ValueError):
            eng.copy_alpha()
        check_oracle(eng, oracle_at(N + K), Xs, "after evaluate")
        val, g = eng.nlml(grad=True)
        val_r, g_r = O.nlml_and_grad(spec, theta, X, y, dist_mode="direct")
        assert abs(val - val_r) <= 1e-10 * abs(val_r)
        assert np.max(np.abs(g - g_r)) <= 1e-8 * max(1.0, np.max(np.abs(g_r)))
        assert rel(eng.copy_alpha(), np.linalg.solve(O.sigma_matrix(spec, theta, X, dist_mode="direct"), y)) <= 1e-8


def _composite(N):
    spec = O.make_spec(4, [0, 1], idx_lin=[1], coreg=[(2, 3)], out_col=3, n_out=2, hetero_noise=True)
    rng = np.random.default_rng(7)
    X = np.column_stack([rng.standard_normal((N, 2)), rng.integers(0, 3, N).astype(float), rng.integers(0, 2, N).astype(float)])
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.2 * X[:, 2] - 0.4 * X[:, 3] + 0.2 * rng.standard_normal(N)
    return spec, np.array(GOLD["composite_N140/theta"]), X, y


def _additive(N):
    from test_oracle import additive_problem

    return additive_problem(n=N // 2, two_outputs=True, lin=True, hetero=True)


@pytest.mark.parametrize("form", ["composite", "additive"])
def test_model_forms(gpu, form):
    """Linear + coregion + two outputs with hetero noise (the composite golden spec) and an additive model, N = 200 + 30."""
    N, K = 200, 30
    spec, theta, X, y = (_composite if form == "composite" else _additive)(N + K)
    if form == "additive":  # (the table stacks the two outputs: shuffle, so that the appended rows hold both)
        perm = np.random.default_rng(1).permutation(len(y))
        X, y = X[perm], y[perm]
    Xs = X[::4].copy()
    Xs[:, 0] += 0.21
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.factorize()
        eng.append(X[N:], y[N:])
        L_r, v_r = O.factorize(spec, theta, X, y, dist_mode="direct")
        ref = (L_r, v_r, O.nlml(spec, theta, X, y, dist_mode="direct"),
               {wn: O.predict(spec, theta, X, y, Xs, with_noise=wn, dist_mode="direct") for wn in (True, False)})
        check_oracle(eng, ref, Xs, form)
        val, g = eng.nlml(grad=True)
        val_r, g_r = O.nlml_and_grad(spec, theta, X, y, dist_mode="direct")
        assert np.max(np.abs(g - g_r)) <= 1e-8 * max(1.0, np.max(np.abs(g_r)))


def test_periodic_model(gpu):
    from periodic_reference import Warped
    from test_gpu_periodic import case as periodic_case, make_engine as periodic_engine

    N, K = 200, 30
    spec, theta, X, y, periods = periodic_case("Matern52", 1, N + K, 2)
    w = Warped(spec, 1, periods)
    Xs = np.random.default_rng(5).standard_normal((M_PRED, 2))
    with periodic_engine(spec, 1, periods, theta, X[:N], y[:N]) as eng:
        eng.factorize()
        eng.append(X[N:], y[N:])
        L_r, v_r = O.factorize(w.spec, w.theta(theta), w.X(X), y, dist_mode="direct")
        ref = (L_r, v_r, w.nlml(theta, X, y), {wn: w.predict(theta, X, y, Xs, with_noise=wn) for wn in (True, False)})
        check_oracle(eng, ref, Xs, "Matern52+Periodic")


def test_joint_state_after_append(gpu):
    """predict_with_grad and predict_joint behind an append: their references at N + K."""
    import var_grad_reference as VR
    from test_joint_cpu import JointOracleEngine

    N, K = 300, 40
    spec, theta, X, y, Xs = table(N + K, 2, "Matern52")
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.factorize()
        eng.predict_joint(Xs, with_noise=False, jitter=1e-6)  # a joint state of the old factor
        eng.append(X[N:], y[N:])
        mean, var, dmean, dvar = eng.predict_with_grad(Xs)
        r_mean, r_var, r_dmean, r_dvar = VR.mean_var_grad(spec, theta, X, y, Xs)
        assert rel(mean, r_mean) <= 1e-8 and np.max(np.abs(var - r_var)) <= 1e-9
        assert np.max(np.abs(dmean - r_dmean)) <= 1e-8 * np.max(np.abs(r_dmean))
        assert np.max(np.abs(dvar - r_dvar)) <= 1e-8 * np.max(np.abs(r_dvar))
        ref = JointOracleEngine()
        ref.set_data(X, y)
        ref.spec = spec
        ref.set_theta(theta)
        for wn, jit in ((True, 0.0), (False, 1e-6)):
            m, cov = eng.predict_joint(Xs, with_noise=wn, jitter=jit)
            m_r, cov_r = ref.predict_joint(Xs, with_noise=wn, jitter=jit)
            assert np.array_equal(cov, cov.T)
            assert float(np.max(np.abs(cov - cov_r))) <= 1e-9 and rel(m, m_r) <= 1e-8


def test_truncate(gpu):
    """(300 + 200) -> truncate(300) predicts as the engine did before the append; truncate(250) matches a fresh engine at 250."""
    N, K = 300, 200
    spec, theta, X, y, Xs = table(N + K)
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.factorize()
        before = {wn: eng.predict(Xs, with_noise=wn) for wn in (True, False)}
        nlml0 = eng.nlml()
        eng.append(X[N:], y[N:])
        eng.truncate(N)
        assert eng.factor_is_current() and eng.N == N
        for wn in (True, False):
            mu, var = eng.predict(Xs, with_noise=wn)
            assert rel(mu, before[wn][0]) <= 1e-10 and np.max(np.abs(var - before[wn][1])) <= 1e-11
        assert abs(eng.nlml() - nlml0) <= 1e-10 * abs(nlml0)
        check_oracle(eng, oracle_at(N + K, n=N), Xs, "truncate(300)")
        eng.truncate(250)
        check_oracle(eng, oracle_at(N + K, n=250), Xs, "truncate(250)")
        with make_engine(spec, theta, X[:250], y[:250]) as fresh:
            fresh.factorize()
            check_engines(eng, fresh, Xs, "truncate(250)")
        eng.truncate(128)  # a whole number of blocks: nothing of the corner is left to factor, the y row is solved again
        check_oracle(eng, oracle_at(N + K, n=128), Xs, "truncate(128)")


def test_without_a_factor_only_the_data_changes(gpu):
    N, K = 300, 30
    spec, theta, X, y, Xs = table(N + K)
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.append(X[N:], y[N:])
        assert not eng.factor_is_current() and eng.N == N + K
        eng.factorize()
        check_oracle(eng, oracle_at(N + K), Xs, "append, then factorize")
        with make_engine(spec, theta, X, y) as fresh:  # exactly what set_data on the concatenated arrays leaves
            fresh.factorize()
            assert np.array_equal(fresh.copy_v(), eng.copy_v()) and fresh.nlml() == eng.nlml()
        eng.set_theta(theta)  # (drops the factor)
        eng.truncate(200)
        assert not eng.factor_is_current() and eng.N == 200
        eng.factorize()
        check_oracle(eng, oracle_at(N + K, n=200), Xs, "truncate, then factorize")


def test_not_positive_definite(gpu):
    """A NaN coordinate in appended row j: LinAlgError, the failing row is N + j of the new matrix, and truncate + factorize recovers."""
    N, K, j = 300, 5, 2
    spec, theta, X, y, Xs = table(N + K)
    Xn = X[N:].copy()
    Xn[j, 0] = np.nan
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.factorize()
        nlml0 = eng.nlml()
        with pytest.raises(np.linalg.LinAlgError):
            eng.append(Xn, y[N:])
        assert eng.notpd_index() == N + j
        assert not eng.factor_is_current() and eng.N == N + K
        eng.truncate(N)
        assert not eng.factor_is_current()
        eng.factorize()
        assert abs(eng.nlml() - nlml0) <= 1e-12 * abs(nlml0)
        check_oracle(eng, oracle_at(N + K, n=N), Xs, "recovered")


def test_refusals_and_no_ops(gpu):
    from gumbi_amd.engine import GMB_EINVAL, GMB_HOST, GMB_OK, Engine

    N, K = 200, 8
    spec, theta, X, y, Xs = table(N + K)
    Xn, yn = np.ascontiguousarray(X[N:]), np.ascontiguousarray(y[N:])
    px, py = Xn.ctypes.data_as(C.c_void_p), yn.ctypes.data_as(C.c_void_p)
    with Engine(0) as bare:  # no data, no theta
        assert bare._lib.gmb_append(bare._h, px, K, 2, py, GMB_HOST) == GMB_EINVAL
        assert bare._lib.gmb_truncate(bare._h, 1) == GMB_EINVAL
        bare.set_data(X[:N], y[:N])
        assert bare._lib.gmb_append(bare._h, px, K, 2, py, GMB_HOST) == GMB_EINVAL  # no kernel, no theta
    with make_engine(spec, theta, X[:N], y[:N]) as eng:
        eng.factorize()
        v0 = eng.copy_v()
        lib, h = eng._lib, eng._h
        assert lib.gmb_append(None, px, K, 2, py, GMB_HOST) == GMB_EINVAL
        assert lib.gmb_append(h, None, K, 2, py, GMB_HOST) == GMB_EINVAL
        assert lib.gmb_append(h, px, K, 2, None, GMB_HOST) == GMB_EINVAL
        assert lib.gmb_append(h, px, K, 1, py, GMB_HOST) == GMB_EINVAL   # ldx < D
        assert lib.gmb_append(h, px, -1, 2, py, GMB_HOST) == GMB_EINVAL
        assert lib.gmb_truncate(h, 0) == GMB_EINVAL and lib.gmb_truncate(h, N + 1) == GMB_EINVAL
        with pytest.raises(ValueError):
            eng.truncate(N + 1)
        with pytest.raises(ValueError):
            eng.append(X[N:, :1], y[N:])
        # the no-ops
        assert lib.gmb_append(h, px, 0, 2, py, GMB_HOST) == GMB_OK
        eng.append(X[:0], y[:0])
        eng.truncate(N)
        assert eng.factor_is_current() and eng.N == N
        assert np.array_equal(eng.copy_v(), v0)
        # capacity mode: no rank holds the factor
        eng.set_dist_mode(Engine.DIST_CAPACITY)
        with pytest.raises(ValueError):
            eng.append(Xn, yn)
        with pytest.raises(ValueError):
            eng.truncate(N - 1)
        eng.set_dist_mode(Engine.DIST_REPLICATED)
        eng.factorize()
        eng.append(Xn, yn)
        check_oracle(eng, oracle_at(N + K), Xs, "after the refusals")


def test_frontend_condition_on_and_sequential_batch(gpu):
    """``HipGP.condition_on`` and the greedy batch on the real engine: conditioning equals a fresh GP on the merged table with the
    same standardizer and hyper-parameters (engine against engine), and the batch leaves the engine as it found it."""
    import gumbi_amd as gmb
    from test_gpu_predict_grad import frontend_dataset

    ds = frontend_dataset(330, ["y"])
    wide = ds.wide
    gp = gmb.GP(gmb.DataSet(wide.iloc[:300].reset_index(drop=True), outputs=["y"]), outputs="y")
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 20})
    theta = gp._theta_fitted.copy()
    gp.condition_on(wide.iloc[300:])
    assert gp.engine.N == 330 and gp.engine.factor_is_current() and len(gp.model.y) == 330
    fresh = gmb.GP(gmb.DataSet(wide.reset_index(drop=True), outputs=["y"], stdzr=gp.stdzr), outputs="y")
    fresh.specify_model(continuous_dims=["a", "b"])
    fresh.build_model()
    fresh.find_MAP(theta=theta)
    assert np.array_equal(fresh.model.X, gp.model.X) and np.array_equal(fresh.model.y, gp.model.y)
    Xs = np.random.default_rng(2).uniform(-1.5, 1.5, (M_PRED, 2))
    check_engines(gp.engine, fresh.engine, Xs, "condition_on")
    before = gp.engine.predict(Xs)
    prop = gp.propose_continuous(acquisition="EI", num_restarts=4, raw_samples=64, seed=1, q=3, sequential=True)
    assert prop.shape == (3,) and len(gp.proposal_acquisition) == 3
    Z = np.column_stack([prop.z[d + "_z"].values() for d in ("a", "b")])
    lo, hi = gp.optimization_bounds
    assert np.all(Z >= lo - 1e-12) and np.all(Z <= hi + 1e-12)
    # (how far apart the picks lie is the model's business: a fantasy at the posterior mean of a NOISY model shrinks the variance
    #  at its pick by sigma^2 / (s^2 + sigma^2) at most, so picks may cluster where 300 observations have settled the surface)
    print("sequential batch:", Z.tolist(), gp.proposal_acquisition)
    assert gp.engine.N == 330 and gp.engine.factor_is_current() and len(gp.model.y) == 330
    after = gp.engine.predict(Xs)
    assert rel(after[0], before[0]) <= 1e-10 and np.max(np.abs(after[1] - before[1])) <= 1e-11


def test_frontend_condition_on_a_single_row(gpu):
    """One new measurement of a single-output model through the front end, on the real engine."""
    import gumbi_amd as gmb
    from test_gpu_predict_grad import frontend_dataset

    wide = frontend_dataset(257, ["y"]).wide
    gp = gmb.GP(gmb.DataSet(wide.iloc[:256].reset_index(drop=True), outputs=["y"]), outputs="y")
    gp.fit(continuous_dims=["a", "b"], MAP_kwargs={"maxeval": 15})
    theta = gp._theta_fitted.copy()
    gp.condition_on(wide.iloc[256:])
    assert gp.engine.N == 257 and gp.engine.factor_is_current() and gp.model.X.shape == (257, 2)
    fresh = gmb.GP(gmb.DataSet(wide.reset_index(drop=True), outputs=["y"], stdzr=gp.stdzr), outputs="y")
    fresh.specify_model(continuous_dims=["a", "b"])
    fresh.build_model()
    fresh.find_MAP(theta=theta)
    assert np.array_equal(fresh.model.X, gp.model.X) and np.array_equal(fresh.model.y, gp.model.y)
    check_engines(gp.engine, fresh.engine, np.random.default_rng(2).uniform(-1.5, 1.5, (M_PRED, 2)), "one row")


def _dist_refusal_worker(out):
    import os

    from test_gpu_distributed import _free_port

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    import torch
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        from gumbi_amd.distributed import DistributedEngine
        from gumbi_amd.engine import KernelSpec

        N, K = 300, 4
        spec, theta, X, y, Xs = table(N + K)
        eng = DistributedEngine(0, panel_blocks=2)
        eng.set_data(X[:N], y[:N])
        eng.set_kernel(KernelSpec(D=2, idx_cont=[0, 1]))
        eng.set_theta(theta)
        eng.factorize()

        def refused(call):
            try:
                call()
            except ValueError as err:
                return "distributed" in str(err)
            return False

        res = {"front": False}
        try:
            eng.append(X[N:], y[N:])
        except NotImplementedError:
            res["front"] = True
        raw = eng.eng  # the engine underneath: its last factorisation was gmb_dist_factorize
        res["append_after_dist_factorize"] = refused(lambda: raw.append(X[N:], y[N:]))
        res["truncate_after_dist_factorize"] = refused(lambda: raw.truncate(N - 1))
        eng.nlml(grad=True)  # leaves U = L^-T in the factor buffer: the factor is consumed as well
        res["consumed"] = not raw.factor_is_current()
        res["append_after_dist_gradient"] = refused(lambda: raw.append(X[N:], y[N:]))
        res["n"] = raw.N
        mu, _ = (eng.factorize(), eng.predict(Xs))[1]
        res["still_works"] = bool(np.all(np.isfinite(mu)))
        out.put(res)
        eng.close()
    except BaseException:
        import traceback

        out.put({"error": traceback.format_exc()[-3000:]})
        raise
    finally:
        dist.destroy_process_group()


def test_engines_whose_last_factorisation_was_distributed_refuse(gpu):
    """The two refusals test_refusals_and_no_ops cannot reach in its own process: an engine whose last factorisation was
    ``gmb_dist_*`` (one rank on the library's RCCL communicator, as tests/test_gpu_distributed.py runs it), and a CONSUMED factor.
    On a single engine ``factor_consumed`` is raised only while a gradient is in flight or after one failed half-way; the state a
    caller can hold it in is the one behind ``gmb_dist_nlml`` with a gradient -- where the distributed refusal applies as well, so
    the consumed-factor branch of ``resize_ready`` has no state of its own to be tested in."""
    import torch.multiprocessing as mp

    from test_gpu_distributed import _collect

    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    p = ctx.Process(target=_dist_refusal_worker, args=(out,))
    p.start()
    (res,) = _collect(out, 1, 300)
    p.join(timeout=60)
    assert "error" not in res, res
    assert p.exitcode == 0
    assert res["front"] and res["append_after_dist_factorize"] and res["truncate_after_dist_factorize"], res
    assert res["consumed"] and res["append_after_dist_gradient"] and res["n"] == 300 and res["still_works"], res
